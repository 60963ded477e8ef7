"""The row-chunk partition behind the scores, region_scores, conditional_scores and ensemble_scores workspaces
(aurora_amd/csrc/planes.h: chunk_rows, chunks_per_plane, chunk_plan), pinned to the sizes the library returned before the
partition was shared, and the refusals the four entries share (planes.hip: plan_chunks), pinned to the messages the library
gave before they were.  No GPU: the *_workspace_bytes calls are host code, and a refused call launches nothing.

The grids reach every branch: one chunk, several chunks, a chunk of more rows than n_lat, n_lon equal to the larger chunk
size (40960) and one above it, where the rows per chunk are held at the wave count (4); the member counts cross every
bucket edge (4 | 8 | 16 | 32 | 64) and with them both chunk sizes (40960 up to bucket 8, 16384 above); 1 and 65 members,
0 and 9 regions, 0 and 9 edges are refused, so the size is 0."""
import pytest

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
REGION = {                                      # by n_regions
    0: (0, 0, 0, 0, 0),
    1: (64, 192, 3200, 192, 128),
    3: (192, 576, 9600, 576, 384),
    8: (512, 1536, 25600, 1536, 1024),
    9: (0, 0, 0, 0, 0),
}
CONDITIONAL = {                                 # by n_edges
    0: (0, 0, 0, 0, 0),
    1: (80, 240, 4000, 240, 160),
    4: (200, 600, 10000, 600, 400),
    8: (360, 1080, 18000, 1080, 720),
    9: (0, 0, 0, 0, 0),
}


def test_workspace_sizes_keep_their_values():
    assert tuple(lib.scores_workspace_bytes(*g) for g in GRIDS) == SCORES
    for n_members, want in ENSEMBLE.items():
        assert tuple(lib.ensemble_scores_workspace_bytes(n_members, *g) for g in GRIDS) == want, n_members
    for n_regions, want in REGION.items():
        assert tuple(lib.region_scores_workspace_bytes(*g, n_regions) for g in GRIDS) == want, n_regions
    for n_edges, want in CONDITIONAL.items():
        assert tuple(lib.conditional_scores_workspace_bytes(*g, n_edges) for g in GRIDS) == want, n_edges


A = 4096                                        # a non-null, aligned address that is never followed: every call below returns first
ENTRIES = {                                     # name -> the raw entry on (n_planes, n_lat, n_lon), every pointer A
    "scores": lambda L, n, la, lo: L.aurora_hip_scores(A, A, A, n, la, lo, A, A, A, None),
    "region_scores": lambda L, n, la, lo: L.aurora_hip_region_scores(A, A, A, n, la, lo, A, A, A, 3, A, A, A, None),
    "conditional_scores": lambda L, n, la, lo: L.aurora_hip_conditional_scores(A, A, A, A, n, la, lo, A, 2, 0, A, A, A, None),
    "ensemble_scores": lambda L, n, la, lo: L.aurora_hip_ensemble_scores(A, A, 8, n, la, lo, A, A, A, A, None),
}


@pytest.mark.parametrize("name", ENTRIES)
def test_shared_refusals_keep_their_messages(name):
    """2^31 - 1 planes are refused on a grid of three row chunks (21 x 4096).  On a grid of one chunk (17 x 32) they are one
    launch of 2^31 - 1 workgroups, which the bound allows: that call would launch, so it is not made here."""
    L = lib.load()
    assert lib.scores_workspace_bytes(1, 21, 4096) == 3 * 64 and lib.ensemble_scores_workspace_bytes(8, 1, 21, 4096) == 3 * 104
    assert ENTRIES[name](L, 3, 0, 32) == -1
    assert L.aurora_hip_last_error().decode() == f"{name}: bad sizes (planes 3, grid 0 x 32)"
    assert ENTRIES[name](L, 2 ** 31 - 1, 21, 4096) == -1
    assert L.aurora_hip_last_error().decode() == f"{name}: too many planes for one launch (2147483647 planes x 3 row chunks)"
    assert ENTRIES[name](L, 0, 17, 32) == 0
