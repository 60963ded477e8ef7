"""The plane stage of the reduction tree (aurora_amd/csrc/planes.hip: finish_partials) behind aurora_hip_scores,
aurora_hip_region_scores and aurora_hip_conditional_scores.  After a call the workspace the caller lent still holds the
partials of the first launch, in the layout each file documents -- [plane][chunk][n_out sums] -- so the rule of planes.h is
checked as written: sums = partial 0, then += partial 1, 2, ... in fp64, bit for bit against the same fold in numpy.

Grids, three planes each: 17 x 32 is one chunk per plane (the finish is a copy), 21 x 4096 three chunks of ten rows (the last
holds one row), 5 x 40961 two chunks (the rows per chunk are held at the wave count; odd rows, so the 4-byte path)."""
import functools

import numpy as np
import pytest
import torch

from aurora_amd.engine import lib
from tests.verification_inputs import DEV, carve, weights

pytestmark = pytest.mark.gpu
N_PLANES = 3
GRIDS = {(17, 32): 1, (21, 4096): 3, (5, 40961): 2}           # (n_lat, n_lon) -> chunks per plane


@functools.lru_cache(maxsize=None)
def inputs(n_lat, n_lon):
    """Device planes p, t, c (seeded normals, a few NaNs in each) and a positive scale plane s; nothing writes to them."""
    g = np.random.default_rng(n_lat * 100000 + n_lon)
    p = g.standard_normal((N_PLANES, n_lat, n_lon)).astype(np.float32)
    t = (p + 0.5 * g.standard_normal(p.shape)).astype(np.float32)
    c = (0.3 * g.standard_normal(p.shape)).astype(np.float32)
    s = (0.5 + g.random(p.shape)).astype(np.float32)
    p[0, 0, 0], t[1, n_lat // 2, n_lon - 1], c[2, n_lat - 1, 1], p[2, n_lat - 1, n_lon // 2] = np.nan, np.nan, np.nan, np.inf
    return tuple(carve(a) for a in (p, t, c, s)), torch.from_numpy(weights(n_lat)).to(DEV)


def pointers(*fields):
    """The plane-pointer arrays of `fields`, one after the other, on the device, and the address of each array."""
    table = torch.tensor([f[k].data_ptr() for f in fields for k in range(N_PLANES)], dtype=torch.int64).to(DEV)
    return table, [table.data_ptr() + 8 * N_PLANES * i for i in range(len(fields))]


def check(n_lat, n_lon, n_out, nbytes, call):
    """call(sums, workspace) -> code.  The workspace is exactly `nbytes` long; sums must be its fold."""
    n_chunks = GRIDS[n_lat, n_lon]
    assert nbytes == N_PLANES * n_chunks * n_out * 8
    workspace = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    sums = torch.full((N_PLANES, n_out), float("nan"), dtype=torch.float64, device=DEV)
    assert call(sums, workspace) == 0, lib.load().aurora_hip_last_error().decode()
    torch.cuda.synchronize()
    partial = workspace.cpu().numpy().view(np.float64).reshape(N_PLANES, n_chunks, n_out)
    got = sums.cpu().numpy()
    v = partial[:, 0].copy()
    for k in range(1, n_chunks):
        v = v + partial[:, k]
    assert partial[..., 0].sum() > 0 and not np.isnan(got).any()               # the partials were written and count points
    assert np.array_equal(got.view(np.int64), v.view(np.int64))
    assert (partial != 0).any(axis=-1).all()                                   # every chunk of every plane has its share


@pytest.mark.parametrize("with_clim", [False, True])
@pytest.mark.parametrize("n_lat,n_lon", list(GRIDS))
def test_scores_sums_are_the_fold_of_the_partials(n_lat, n_lon, with_clim):
    (p, t, c, _), w = inputs(n_lat, n_lon)
    table, (pp, tp, cp) = pointers(p, t, c)
    check(n_lat, n_lon, 8, lib.scores_workspace_bytes(N_PLANES, n_lat, n_lon), lambda sums, ws: lib.load().aurora_hip_scores(
        pp, tp, cp if with_clim else None, N_PLANES, n_lat, n_lon, w.data_ptr(), sums.data_ptr(), ws.data_ptr(),
        torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("with_clim", [False, True])
@pytest.mark.parametrize("n_lat,n_lon", list(GRIDS))
def test_region_sums_are_the_fold_of_the_partials(n_lat, n_lon, with_clim):
    (p, t, c, _), w = inputs(n_lat, n_lon)
    table, (pp, tp, cp) = pointers(p, t, c)
    g = np.random.default_rng(7)
    rows = torch.from_numpy(g.integers(1, 8, n_lat, dtype=np.uint8)).to(DEV)      # every row in some of the three regions
    cols = torch.from_numpy(g.integers(0, 8, n_lon, dtype=np.uint8)).to(DEV)
    check(n_lat, n_lon, 24, lib.region_scores_workspace_bytes(N_PLANES, n_lat, n_lon, 3),
          lambda sums, ws: lib.load().aurora_hip_region_scores(
              pp, tp, cp if with_clim else None, N_PLANES, n_lat, n_lon, rows.data_ptr(), cols.data_ptr(), None, 3, w.data_ptr(),
              sums.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("with_maps", [False, True])
@pytest.mark.parametrize("n_lat,n_lon", list(GRIDS))
def test_conditional_sums_are_the_fold_of_the_partials(n_lat, n_lon, with_maps):
    (p, t, c, s), w = inputs(n_lat, n_lon)
    table, (pp, tp, cp, sp) = pointers(p, t, c, s)
    edges = torch.tensor([[-0.5, 0.5]] * N_PLANES, dtype=torch.float32, device=DEV)
    check(n_lat, n_lon, 15, lib.conditional_scores_workspace_bytes(N_PLANES, n_lat, n_lon, 2),
          lambda sums, ws: lib.load().aurora_hip_conditional_scores(
              pp, tp, cp if with_maps else None, sp if with_maps else None, N_PLANES, n_lat, n_lon, edges.data_ptr(), 2, 0,
              w.data_ptr(), sums.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream))
