"""`aurora_amd.conservative_regrid` on the device: every bit of the HIP path equals the numpy path (which
tests/test_conservative_regrid_host.py judges against a dense fp64 evaluation), on every path the kernel has.

The kernel's tile is 256 target columns (kThreads of csrc/conservative_regrid.hip) by 4 target rows, of up to 8 planes per
workgroup; the row sums of 1024 source columns are parked in LDS at a time."""
import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, _fields, conservative_regrid
from aurora_amd import conservative as C
from tests.conservative_inputs import GRIDS, batch, circle, every_field, lin, same_bits
from tests.verification_inputs import DEV, carve

pytestmark = pytest.mark.gpu

TILE_COLUMNS = 256
WIDE = (lin(80, -80, 9), circle(1500), lin(75, -75, 4), circle(600))     # 600 target columns: three column tiles


def on_device(b: Batch, offset_floats=None) -> Batch:
    """`b` on the device; with `offset_floats`, every fp32 field carved that many floats past an aligned start."""
    if offset_floats is None:
        return b.to(DEV)
    move = lambda v: carve(v, offset_floats=offset_floats) if v.dtype == torch.float32 else v.to(DEV)  # noqa: E731
    md = b.metadata
    return Batch({k: move(v) for k, v in b.surf_vars.items()}, {k: move(v) for k, v in b.static_vars.items()},
                 {k: move(v) for k, v in b.atmos_vars.items()},
                 aurora_amd.batch.derive_metadata(md, lat=md.lat.to(DEV), lon=md.lon.to(DEV)))


def regridded(b: Batch, grid, **kw) -> Batch:
    return conservative_regrid(b, lat=grid[2], lon=grid[3], **kw)


def assert_same(dev: Batch, host: Batch) -> None:
    for (_, k, d), (_, _, h) in zip(every_field(dev), every_field(host)):
        assert d.device == DEV and same_bits(d, h), k


# ---- parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRIDS))
def test_the_device_path_equals_the_numpy_path(name):
    """B = 2, T = 2, 3 levels: 18 planes and the static one, more than a workgroup's 8; a land mask of 50 %."""
    grid = GRIDS[name]
    b = batch(grid[0], grid[1], seed=21, B=2, T=2, land=0.5)
    for min_valid in (0.5, 1e-6):
        host = regridded(b, grid, min_valid=min_valid)
        dev = regridded(on_device(b), grid, min_valid=min_valid)
        assert_same(dev, host)
        assert torch.isfinite(host.surf_vars["2t"]).any()
    md = dev.metadata
    assert md.lat.device == md.lon.device == DEV and md.lat.dtype == torch.float64
    assert np.array_equal(md.lat.cpu().numpy(), grid[2]) and np.array_equal(md.lon.cpu().numpy(), grid[3])
    assert md.time == b.metadata.time and md.rollout_step == b.metadata.rollout_step


def test_a_row_over_three_column_tiles_and_the_seam():
    p = C.plan(*WIDE)
    assert len(WIDE[3]) > 2 * TILE_COLUMNS
    first = p.cols.first[0, 0]
    assert [(first + t) % 1500 for t in range(p.cols.count[0])] == [1499, 0, 1]
    b = batch(WIDE[0], WIDE[1], seed=22, B=1, T=1, land=0.1)
    assert_same(regridded(on_device(b), WIDE), regridded(b, WIDE))


def test_a_span_longer_than_the_lds_image():
    """6 source columns per target column: a tile of 256 target columns needs 1536 source columns, two LDS images."""
    grid = (lin(80, -80, 5), circle(2400), lin(60, -60, 3), circle(400))
    b = batch(grid[0], grid[1], seed=23, B=1, T=1, land=0.1)
    assert_same(regridded(on_device(b), grid), regridded(b, grid))


def test_more_than_eight_taps_per_column():
    """20 source columns under a target column: the taps past the eighth are read from the table, not from registers."""
    grid = (lin(80, -80, 40), circle(240), lin(60, -60, 3), circle(12))
    assert C.plan(*grid).cols.count.max() > 8 and C.plan(*grid).rows.count.max() > 8
    b = batch(grid[0], grid[1], seed=24, B=1, T=1, land=0.2)
    assert_same(regridded(on_device(b), grid), regridded(b, grid))


# ---- kernel paths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["poles 19x36 -> 8x14", "wide"])
def test_unaligned_planes_give_the_same_bits(name):
    grid = WIDE if name == "wide" else GRIDS[name]
    b = batch(grid[0], grid[1], seed=25, B=1, T=2, land=0.2)
    want = regridded(on_device(b), grid)
    assert all(v.data_ptr() % 16 == 0 for _, _, v in every_field(on_device(b)))
    shifted = on_device(b, offset_floats=1)
    assert all(v.data_ptr() % 16 == 4 for _, _, v in every_field(shifted))
    assert_same(regridded(shifted, grid), want.to("cpu"))
    # outputs carved likewise: the binding's call into planes one float past an aligned start
    from aurora_amd.engine import lib

    p = C.plan(*grid)
    key = tuple(a.tobytes() for a in (grid[0], grid[1], p.lat, p.lon))
    tables = C.device_tables(p, key, DEV)
    src = [shifted.surf_vars["2t"]]
    out = carve(torch.full((2, len(grid[2]), len(grid[3])), 7.0), offset_floats=1, fill=7.0)
    lib.conservative_regrid(src, out, tables, 0.5)
    assert out.data_ptr() % 16 == 4 and same_bits(out.view(1, 2, *out.shape[1:]), want.surf_vars["2t"])


def test_37_columns_regional():
    grid = (lin(60, 30, 11), lin(10, 46, 37), lin(58, 32, 5), lin(12, 44, 9))
    b = batch(grid[0], grid[1], seed=26, land=0.2)
    assert_same(regridded(on_device(b), grid), regridded(b, grid))


@pytest.mark.parametrize("dtype", [torch.float64, torch.bfloat16, torch.float16])
def test_other_source_precisions(dtype):
    grid = GRIDS["poles 19x36 -> 8x14"]
    b = batch(grid[0], grid[1], seed=27, B=2, T=1, land=0.2, dtype=dtype)
    assert_same(regridded(on_device(b), grid), regridded(b, grid))
    mixed = Batch(b.surf_vars, {k: v.float() for k, v in b.static_vars.items()}, b.atmos_vars, b.metadata)   # two launches
    assert_same(regridded(on_device(mixed), grid), regridded(mixed, grid))


# ---- independence and safety ----------------------------------------------------------------------------------------------------
def test_a_plane_alone_and_among_the_others_repeated_calls_and_the_source():
    grid = GRIDS["poles 19x36 -> 8x14"]
    b = on_device(batch(grid[0], grid[1], seed=28, B=2, T=2, land=0.3))
    before = {k: v.clone() for _, k, v in every_field(b)}
    first, second = regridded(b, grid), regridded(b, grid)
    assert_same(second, first.to("cpu"))
    alone = Batch({"msl": b.surf_vars["msl"][1:, 1:]}, {}, {}, b.metadata)
    assert same_bits(regridded(alone, grid).surf_vars["msl"], first.surf_vars["msl"][1:, 1:])
    for _, k, v in every_field(b):
        assert same_bits(v, before[k]), k


def test_guard_words_around_every_output_plane_are_untouched():
    from aurora_amd.engine import lib

    grid = WIDE
    b = on_device(batch(grid[0], grid[1], seed=29, B=1, T=2, land=0.1))
    want = regridded(b, grid).surf_vars["2t"]
    p = C.plan(*grid)
    tables = C.device_tables(p, tuple(a.tobytes() for a in (grid[0], grid[1], p.lat, p.lon)), DEV)
    n_rows, n_cols, guard = len(grid[2]), len(grid[3]), 64
    # the binding writes planes that follow each other, so the words around every plane are the neighbours' rims: each plane
    # is regridded by a call of its own into the middle of a guarded buffer
    for t in range(2):
        buf = torch.full((guard + n_rows * n_cols + guard,), -12345.0, device=DEV)
        out = buf[guard:guard + n_rows * n_cols].view(1, n_rows, n_cols)
        lib.conservative_regrid([b.surf_vars["2t"][:, t]], out, tables, 0.5)
        assert same_bits(out, want[:, t])
        assert bool((buf[:guard] == -12345.0).all()) and bool((buf[-guard:] == -12345.0).all())


# ---- hipGraph -------------------------------------------------------------------------------------------------------------------
def test_capture_replay_and_no_upload_on_the_second_call(monkeypatch):
    uploads = []

    def upload(a, device):
        uploads.append(a)
        return _fields._upload(a, device)

    monkeypatch.setattr(_fields, "tables", _fields.DeviceTables(upload=upload))
    grid = GRIDS["no poles 12x20 -> 7x12"]
    host = batch(grid[0], grid[1], seed=30, B=2, T=2, land=0.2)
    b = on_device(host)
    first = regridded(b, grid)                                                     # the eager call
    n = len(uploads)
    assert n == 3                                                                  # the tables in one array, and lat and lon
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = regridded(b, grid)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(uploads) == n
    assert second.metadata.lat is first.metadata.lat and second.metadata.lon is first.metadata.lon
    assert_same(second, first.to("cpu"))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = regridded(b, grid)
    assert len(uploads) == n
    other = batch(grid[0], grid[1], seed=31, B=2, T=2, land=0.2)
    for (_, _, dst), (_, _, src) in zip(every_field(b), every_field(other)):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    assert_same(captured, regridded(other, grid))
    assert not same_bits(captured.surf_vars["2t"], first.surf_vars["2t"])
    # a first call during capture is refused (the capture query is injected: nothing is captured here)
    monkeypatch.setattr(_fields, "tables", _fields.DeviceTables(capturing=lambda: True))
    with pytest.raises(RuntimeError, match="conservative_regrid: call once on this pair of grids before capturing a graph"):
        regridded(b, grid)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def test_scores_of_a_regridded_prediction():
    grid = GRIDS["poles 19x36 -> 8x14"]
    pred, truth = batch(grid[0], grid[1], seed=32, B=2), batch(grid[2], grid[3], seed=33, B=2)
    truth_dev = on_device(truth)
    lat, lon = truth_dev.metadata.lat, truth_dev.metadata.lon
    coarse = conservative_regrid(on_device(pred), lat=lat, lon=lon)
    assert coarse.metadata.lat is lat and coarse.metadata.lon is lon
    on_dev = aurora_amd.scores(coarse, truth_dev)
    host_coarse = conservative_regrid(pred, lat=truth.metadata.lat, lon=truth.metadata.lon)
    moved = aurora_amd.scores(on_device(host_coarse), truth_dev)                   # the CPU path's fields, scored alike
    on_host = aurora_amd.scores(host_coarse, truth)
    for k, v in on_host.bias.items():
        assert on_dev.bias[k].device == DEV
        assert torch.equal(on_dev.bias[k], moved.bias[k]), k
        # (scores() adds in another order on the host than on the device: a few fp32 ulps of the result at the most)
        assert torch.allclose(on_dev.bias[k].cpu().double(), v.double(), rtol=1e-6, atol=0), k
