"""The row-chunk partition behind the scores and ensemble_scores workspaces (aurora_amd/csrc/planes.h: chunk_rows,
chunks_per_plane), pinned to the sizes the library returned before the partition was shared.  No GPU: the two
*_workspace_bytes calls are host code.

The grids reach every branch: one chunk, several chunks, a chunk of more rows than n_lat, n_lon equal to the larger chunk
size (40960) and one above it, where the rows per chunk are held at the wave count (4); the member counts cross every
bucket edge (4 | 8 | 16 | 32 | 64) and with them both chunk sizes (40960 up to bucket 8, 16384 above); 1 and 65 members
are refused, so the size is 0."""
from aurora_amd.engine import lib

GRIDS = ((1, 1, 1), (3, 17, 32), (2, 721, 1440), (1, 9, 40960), (1, 5, 40961))    # (n_planes, n_lat, n_lon)
SCORES = (64, 192, 3200, 192, 128)
ENSEMBLE = {
    1: (0, 0, 0, 0, 0),
    2: (88, 264, 4400, 264, 176),
    4: (88, 264, 4400, 264, 176),
    5: (104, 312, 5200, 312, 208),
    8: (104, 312, 5200, 312, 208),
    9: (136, 408, 16592, 408, 272),
    16: (136, 408, 16592, 408, 272),
    17: (200, 600, 24400, 600, 400),
    32: (200, 600, 24400, 600, 400),
    33: (328, 984, 40016, 984, 656),
    64: (328, 984, 40016, 984, 656),
    65: (0, 0, 0, 0, 0),
}


def test_workspace_sizes_keep_their_values():
    assert tuple(lib.scores_workspace_bytes(*g) for g in GRIDS) == SCORES
    for n_members, want in ENSEMBLE.items():
        assert tuple(lib.ensemble_scores_workspace_bytes(n_members, *g) for g in GRIDS) == want, n_members
