"""`aurora_amd.region_scores` on the device: aurora_hip_region_scores against the numpy fp64 yardstick of
tests/test_region_scores_host.py (`yardstick_sums`; not `aurora_amd.regions._sums_host`, which is code under test).  The raw
tests build the row, column and mask bit tables themselves, from the yardstick's `membership`.

Bound (derived in tests/test_gpu_scores.py, restated in tests/test_gpu_conditional_scores.py, not tuned): both sides are within
N 2^-53 sum|term| of the exact sum; with N <= 721 x 1440, 2 N 2^-53 = 2.3e-10, so the count is exact, S1, S3, S4, S6 and S7
agree to 1e-9 relative, S2 to 1e-9 x S4 and S5 to 1e-9 x sum w |p' t'|; finalised: rmse to 1e-9 relative, mae to 2e-9 relative,
bias to 2e-9 x mae, acc to 3e-9 absolute.  Every plane and every region is compared."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, Metadata, Region, Regions, region_scores, rollout, scores
from aurora_amd import _fields
from aurora_amd.engine import lib
from tests import helpers
from tests.golden_cases import CASES
from tests.test_region_scores_host import (REL, assert_scores_match, assert_sums_match, coords, make_inputs, membership, regions_of,
                                           yardstick_of, yardstick_sums)
from tests.verification_inputs import DEV, carve, cos_weights

pytestmark = pytest.mark.gpu

def raw_specs(mask):
    """Eight regions as the yardstick's tuples -- tropical land, europe, land, global, tropics, extratropics, one point, a
    masked box of the southern Pacific: a masked band first (R = 1), then a wrapping box and a mask alone (R = 3); mask None:
    the same without any mask."""
    return [(((-20, 20),), None, mask), (((35, 75),), ((-12.5, 42.5),), None), (None, None, mask), (None, None, None),
            (((-20, 20),), None, None), (((-90, -20), (20, 90)), None, None), (((0, 0),), ((0, 0),), None),
            (((-90, -20),), ((145, -130),), mask)]


def grid(n_lat, n_lon):
    return np.linspace(90, -90, n_lat), np.linspace(0, 360, n_lon + 1)[:-1]


def bit_tables(lat, lon, specs, mask_offset=0):
    """Device uint8 tables of `specs` (bit r: region r): rows, columns and the mask plane (None if no region has a mask),
    the plane `mask_offset` bytes past the start of its buffer."""
    rows, cols = np.zeros(lat.shape[0], dtype=np.uint8), np.zeros(lon.shape[0], dtype=np.uint8)
    plane = np.zeros((lat.shape[0], lon.shape[0]), dtype=np.uint8)
    for r, (lats, lons, mask) in enumerate(specs):
        rows |= membership(lat, lon, (lats, None, None))[:, 0].astype(np.uint8) << r
        cols |= membership(lat, lon, (None, lons, None))[0].astype(np.uint8) << r
        plane |= (np.ones(plane.shape, dtype=np.uint8) if mask is None else mask.astype(np.uint8)) << r
    up = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    if all(m is None for _, _, m in specs):
        return up(rows), up(cols), None
    flat = torch.zeros(mask_offset + plane.size, dtype=torch.uint8)
    flat[mask_offset:] = torch.from_numpy(plane).reshape(-1)
    on_dev = flat.to(DEV)[mask_offset:].view(plane.shape)
    assert on_dev.data_ptr() % 4 == mask_offset % 4
    return up(rows), up(cols), on_dev


@functools.lru_cache(maxsize=None)
def raw_inputs(n_planes, n_lat, n_lon, clean=False):
    """Host planes p, t, c (pressure-like, d small against p), a seeded mask, and -- unless `clean` -- NaN and +-Inf in each
    operand and a whole row of NaN.  Made once per grid; nothing writes to them."""
    g = np.random.default_rng(n_lat * 10000 + n_lon)
    p = (101325 + 300 * g.standard_normal((n_planes, n_lat, n_lon))).astype(np.float32)
    t = (p + 2 * g.standard_normal(p.shape) + 0.5).astype(np.float32)
    c = (101325 + 100 * g.standard_normal(p.shape)).astype(np.float32)
    mask = g.standard_normal((n_lat, n_lon)) >= 0
    if not clean:
        mid = n_lat // 2
        p[0, 0, 0], p[0, mid, n_lon - 1], t[0, mid, 0], t[0, n_lat - 1, n_lon - 1] = np.nan, np.inf, -np.inf, np.nan
        c[0, mid, 1], c[0, mid - 1, n_lon - 2] = np.inf, np.nan
        t[1, mid] = np.nan                                                        # a whole row, on or next to the equator
    for a in (p, t, c, mask):
        a.setflags(write=False)
    return p, t, c, mask


@functools.lru_cache(maxsize=None)
def raw_yardstick(n_planes, n_lat, n_lon, with_clim, masked, clean=False):
    """(sums (n_planes, 8 regions, 8), sums of w |p' t'|) of `raw_inputs`: a region's sums do not depend on the others, so one
    table serves every R."""
    p, t, c, mask = raw_inputs(n_planes, n_lat, n_lon, clean)
    lat, lon = grid(n_lat, n_lon)
    return yardstick_sums(p, t, c if with_clim else None, cos_weights(lat), lat, lon, raw_specs(mask if masked else None), with_abs=True)


def call(p, t, c, tables, R, w_dev):
    out = lib.region_sums([p], [t], None if c is None else [c], *tables, R, w_dev)
    assert out.shape == (p.shape[0], R, 8) and out.dtype == torch.float64 and out.device == DEV
    return out


def w_of(n_lat):
    return torch.from_numpy(cos_weights(grid(n_lat, 1)[0])).to(DEV)


@pytest.mark.parametrize("n_planes,n_lat,n_lon,offset,mask_offset,full", [
    (3, 33, 64, 0, 0, True),
    (3, 33, 61, 0, 0, True),        # odd n_lon: byte loads, a partial last quad
    (2, 5, 8, 0, 0, True),
    (2, 130, 1024, 0, 0, True),     # four row chunks
    (3, 33, 64, 3, 0, True),        # planes 3 floats past a 16-byte boundary
    (3, 33, 64, 0, 1, True),        # the mask plane 1 byte past a 4-byte boundary
    (3, 721, 1440, 0, 0, False),    # 0.25 degrees: R = 8 with a mask and a climatology only
])
def test_raw_table_equals_the_yardstick(n_planes, n_lat, n_lon, offset, mask_offset, full):
    p, t, c, mask = raw_inputs(n_planes, n_lat, n_lon)
    lat, lon = grid(n_lat, n_lon)
    dev = [carve(a, offset) for a in (p, t, c)]
    assert all(x[k].data_ptr() % 16 == (4 * offset) % 16 for x in dev for k in range(n_planes)) or n_lon % 4
    w_dev = w_of(n_lat)
    keep = [x.clone() for x in dev]
    n_chunks = lib.region_scores_workspace_bytes(1, n_lat, n_lon, 1) // 64
    assert n_chunks == {130: 4, 721: 25}.get(n_lat, 1)
    for masked in ((False, True) if full else (True,)):
        specs = raw_specs(mask if masked else None)
        for R in ((1, 3, 8) if full else (8,)):
            tables = bit_tables(lat, lon, specs[:R], mask_offset)
            keep_tables = [x.clone() for x in tables if x is not None]
            assert (tables[2] is None) == (not masked)
            for with_clim in ((False, True) if full else (True,)):
                got = call(dev[0], dev[1], dev[2] if with_clim else None, tables, R, w_dev).cpu().numpy()
                y, abs5 = raw_yardstick(n_planes, n_lat, n_lon, with_clim, masked)
                what = f"{n_planes}x{n_lat}x{n_lon}+{offset}/{mask_offset} R={R} clim={with_clim} mask={masked}"
                print(what, "counts", got[..., 0].tolist())
                assert_sums_match(got, y[:, :R], abs5[:, :R] if with_clim else None, what)
            for x, k in zip([x for x in tables if x is not None], keep_tables):
                assert torch.equal(x, k)
    for x, k in zip(dev, keep):                                                   # the inputs are not modified
        assert torch.equal(x.view(torch.int32), k.view(torch.int32))
    if n_planes == 3:                           # the input is not trivial: every region holds valid points and none holds all
        y, _ = raw_yardstick(n_planes, n_lat, n_lon, True, True)                  # (the one point is invalid in planes 0 and 1)
        assert (y[:, [0, 1, 2, 3, 4, 5, 7], 0] >= 1).all() and y[:, 6, 0].tolist() == [0, 0, 1]
        assert (y[:, [0, 1, 2, 4, 5, 6, 7], 0] < y[:, 3:4, 0]).all()


@pytest.mark.parametrize("n_lat,n_lon", [(33, 61), (130, 1024)])
def test_repeatable_and_independent_of_planes_regions_and_climatology(n_lat, n_lon):
    """Two calls give equal bits; a plane alone equals itself among three; a region's eight sums have the same bits alone, first
    or last of 3, and among 8 (the four instantiations of the kernel), and slots 0-4 with or without a climatology (which is
    finite everywhere here, so validity is the same)."""
    p, t, c, mask = raw_inputs(3, n_lat, n_lon, clean=True)
    lat, lon = grid(n_lat, n_lon)
    dev = [carve(a) for a in (p, t, c)]
    w_dev = w_of(n_lat)
    specs = raw_specs(mask)
    eight = {clim: call(dev[0], dev[1], dev[2] if clim else None, bit_tables(lat, lon, specs), 8, w_dev) for clim in (False, True)}
    again = call(*dev, bit_tables(lat, lon, specs), 8, w_dev)
    alone = torch.cat([call(*(x[k:k + 1] for x in dev), bit_tables(lat, lon, specs), 8, w_dev) for k in range(3)])
    assert torch.equal(eight[True], again) and torch.equal(eight[True], alone)
    assert torch.equal(eight[True][..., :5], eight[False][..., :5]) and (eight[False][..., 5:] == 0).all()
    assert (eight[True][:, [0, 1, 2, 3, 4, 5, 7], 0] > 0).all() and (eight[True][:, 6, 0] == n_lat % 2).all()   # (even: no row on 0)
    y, abs5 = raw_yardstick(3, n_lat, n_lon, True, True, clean=True)
    assert_sums_match(eight[True].cpu().numpy(), y, abs5, "eight")
    for r in (0, 1, 2, 7):
        a, b = specs[(r + 3) % 8], specs[(r + 5) % 8]
        for clim in (False, True):
            cc = dev[2] if clim else None
            want = eight[clim][:, r]
            assert torch.equal(call(dev[0], dev[1], cc, bit_tables(lat, lon, [specs[r]]), 1, w_dev)[:, 0], want), (r, clim, "alone")
            assert torch.equal(call(dev[0], dev[1], cc, bit_tables(lat, lon, [specs[r], a]), 2, w_dev)[:, 0], want), (r, clim, "of 2")
            assert torch.equal(call(dev[0], dev[1], cc, bit_tables(lat, lon, [specs[r], a, b]), 3, w_dev)[:, 0], want), (r, clim, "first")
            assert torch.equal(call(dev[0], dev[1], cc, bit_tables(lat, lon, [a, b, specs[r]]), 3, w_dev)[:, 2], want), (r, clim, "last")
            assert torch.equal(call(dev[0], dev[1], cc, bit_tables(lat, lon, [a, b, a, b, specs[r]]), 5, w_dev)[:, 4], want), (r, clim, "of 5")


def test_bits_beyond_the_regions_of_the_call_are_ignored():
    p, t, c, mask = raw_inputs(3, 33, 64)
    lat, lon = grid(33, 64)
    dev = [carve(a) for a in (p, t, c)]
    w_dev = w_of(33)
    specs = raw_specs(mask)
    three = call(*dev, bit_tables(lat, lon, specs[:3]), 3, w_dev)
    assert torch.equal(call(*dev, bit_tables(lat, lon, specs), 3, w_dev), three)   # the tables of eight, three asked for


def test_alignment_does_not_change_a_single_bit():
    p, t, c, mask = raw_inputs(3, 33, 64)
    lat, lon = grid(33, 64)
    w_dev = w_of(33)
    specs = raw_specs(mask)
    a, b = [carve(x) for x in (p, t, c)], [carve(x, 1) for x in (p, t, c)]
    assert a[0].data_ptr() % 16 == 0 and b[0].data_ptr() % 16 == 4 and torch.equal(a[1].nan_to_num(), b[1].nan_to_num())
    for R in (1, 3, 8):
        base = call(*a, bit_tables(lat, lon, specs[:R]), R, w_dev)
        assert torch.equal(call(*b, bit_tables(lat, lon, specs[:R]), R, w_dev), base)
        for off in (1, 2, 3):
            assert torch.equal(call(*a, bit_tables(lat, lon, specs[:R], mask_offset=off), R, w_dev), base), (R, off)
        rows, cols, plane = bit_tables(lat, lon, specs[:R])
        shifted = torch.zeros(cols.numel() + 1, dtype=torch.uint8, device=DEV)
        shifted[1:] = cols
        assert shifted[1:].data_ptr() % 4 == 1
        assert torch.equal(call(*a, (rows, shifted[1:], plane), R, w_dev), base), (R, "column table")
        assert torch.equal(call(a[0], a[1], None, (rows, shifted[1:], plane), R, w_dev), call(b[0], b[1], None, (rows, cols, plane), R, w_dev))


@pytest.mark.parametrize("n_lat,n_lon", [(33, 64), (130, 1024)])
def test_row_skipping_is_invisible(n_lat, n_lon):
    """A tropics call on planes whose rows outside the tropics are NaN equals, bit for bit, the call on the unfilled planes,
    and the tropics of an 8-region call, in which every row is read."""
    p, t, c, mask = raw_inputs(3, n_lat, n_lon)
    lat, lon = grid(n_lat, n_lon)
    w_dev = w_of(n_lat)
    specs = raw_specs(mask)
    outside = torch.from_numpy(~((lat >= -20) & (lat <= 20)))
    assert 0 < (~outside).sum() < n_lat
    dev = [carve(a) for a in (p, t, c)]
    filled = [x.clone() for x in dev]
    for x in filled:
        x[:, outside.to(DEV)] = float("nan")
    whole = call(*dev, bit_tables(lat, lon, specs), 8, w_dev)
    for r in (4, 0):                                                              # tropics; tropical land
        tables = bit_tables(lat, lon, [specs[r]])
        for clim in (False, True):
            got = call(filled[0], filled[1], filled[2] if clim else None, tables, 1, w_dev)
            assert torch.equal(got, call(dev[0], dev[1], dev[2] if clim else None, tables, 1, w_dev))
            assert (got[:, 0, 0] > 0).all()
        assert torch.equal(got[:, 0], whole[:, r])
    assert (call(*filled, bit_tables(lat, lon, specs[3:4]), 1, w_dev)[:, 0, 0] == whole[:, 4, 0]).all()   # global sees the NaNs


# ---- the front end -------------------------------------------------------------------------------------------------------
def on_device(kind, n_lat, n_lon, seed=0):
    pred, truth, clim, specs = make_inputs(kind, n_lat, n_lon, seed)
    return (pred, truth, clim), tuple(b.to(DEV) for b in (pred, truth, clim)), specs


def twelve(specs):
    """Twelve regions (two launches): the seven of the host tests, then five of them again under other names."""
    one = regions_of(specs, mask_as=lambda m: torch.from_numpy(m).to(DEV))
    return {**one, **{f"{k} again": v for k, v in list(one.items())[2:7]}}, {**specs, **{f"{k} again": v for k, v in list(specs.items())[2:7]}}


@pytest.mark.parametrize("kind,n_lat,n_lon", [("randn", 33, 64), ("red_noise", 33, 61)])
def test_front_end_equals_the_cpu_path_the_yardstick_and_scores(kind, n_lat, n_lon):
    host, dev, specs = on_device(kind, n_lat, n_lon)
    for with_clim in (False, True):
        h = (*host[:2], host[2] if with_clim else None)
        d = (*dev[:2], dev[2] if with_clim else None)
        s = region_scores(d[0], d[1], regions_of(specs, mask_as=lambda m: torch.from_numpy(m).to(DEV)), climatology=d[2])
        assert s.rmse["2t"].device == DEV and s.rmse["z"].shape == (2, 3, 7) and s.table.dtype == torch.float64
        on_cpu = region_scores(h[0], h[1], regions_of(specs), climatology=h[2])
        got = s.cpu()
        assert got.layout == on_cpu.layout and got.regions == on_cpu.regions
        y, abs5 = yardstick_of(*h, specs, with_abs=True)
        for other in (on_cpu.table[..., :8].numpy(), y):
            assert_sums_match(got.table[..., :8].numpy(), other, abs5 if with_clim else None, f"{kind} clim={with_clim}")
        assert_scores_match(got, y, f"{kind} clim={with_clim}")
        assert_scores_match(got, on_cpu.table[..., :8].numpy(), f"{kind} clim={with_clim} against the CPU path")
        # the global region against aurora_amd.scores on the device
        whole, ref = got["global"], scores(*d).cpu()
        assert torch.equal(whole.table[:, 0], ref.table[:, 0]) and whole.layout == ref.layout
        assert_sums_match(whole.table[:, None, :8].numpy(), ref.table[:, None, :8].numpy(), abs5[:, :1] if with_clim else None, "scores")
        g, r = whole.table.numpy(), ref.table.numpy()
        assert (np.abs(g[:, 8] - r[:, 8]) <= REL * r[:, 8]).all() and (np.abs(g[:, 10] - r[:, 10]) <= 2 * REL * r[:, 10]).all()
        assert (np.abs(g[:, 9] - r[:, 9]) <= 2 * REL * r[:, 10]).all()
        if with_clim:
            assert (np.abs(g[:, 11] - r[:, 11]) <= 3 * REL).all()


def test_twelve_regions_in_two_launches_equal_each_region_alone():
    host, dev, specs = on_device("red_noise", 33, 61)
    regs, all_specs = twelve(specs)
    for with_clim in (False, True):
        clim = dev[2] if with_clim else None
        s = region_scores(dev[0], dev[1], regs, climatology=clim)
        assert len(s.regions) == 12 and s.table.shape == (10, 12, 12)
        for r, (name, region) in enumerate(regs.items()):
            alone = region_scores(dev[0], dev[1], {name: region}, climatology=clim)
            assert torch.equal(s.table[:, r, :8], alone.table[:, 0, :8]), (name, with_clim)
        y, abs5 = yardstick_of(host[0], host[1], host[2] if with_clim else None, all_specs, with_abs=True)
        assert_sums_match(s.table[..., :8].cpu().numpy(), y, abs5 if with_clim else None, "twelve")
        mixed = region_scores(dev[0], dev[1], regions_of(specs), climatology=clim)          # host masks, device fields
        assert torch.equal(mixed.table[..., :8], s.table[:, :7, :8])


def test_invalid_points_and_empty_regions():
    """NaN / Inf in each operand are in the inputs of every test above; here: a region with no valid point in one plane, and an
    all-False mask on the device, formed and scored without a synchronisation."""
    host, dev, specs = on_device("randn", 33, 64, seed=5)
    lat, _ = coords(host[0])
    tropics = torch.from_numpy((lat >= -20) & (lat <= 20)).to(DEV)
    pred = Batch({k: v.clone() for k, v in dev[0].surf_vars.items()}, {}, {k: v.clone() for k, v in dev[0].atmos_vars.items()},
                 dev[0].metadata)
    pred.surf_vars["2t"][0, -1, tropics] = float("inf")
    pred.atmos_vars["z"][1, -1, 2] = float("nan")
    regs = {"tropics": Region(lat=(-20, 20)), "global": Region(), "land": Region(mask=torch.from_numpy(specs["land"][2]).to(DEV))}
    s = region_scores(pred, dev[1], regs, climatology=dev[2])                     # (also the warm call of the tables)
    none = {**regs, "land": Region(mask=torch.zeros(33, 64, dtype=torch.bool, device=DEV))}
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        e = region_scores(pred, dev[1], none, climatology=dev[2])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    s, e = s.cpu(), e.cpu()
    assert s.count["2t"][0].tolist()[0] == 0 and s.count["2t"][1, 0] > 0 and s.count["2t"][0, 1] == 33 * 64 - 7 * 64 - 2
    assert (s.count["z"][1, 2] == 0).all() and (s.sums["z"][1, 2] == 0).all() and (s.sums["2t"][0, 0] == 0).all()
    for d in (s.rmse, s.bias, s.mae, s.acc):
        assert torch.isnan(d["2t"][0, 0]) and torch.isnan(d["z"][1, 2]).all() and not torch.isnan(d["2t"][1]).any()
    assert (e.table[:, 2, :8] == 0).all() and torch.isnan(e.table[:, 2, 8:]).all()
    assert torch.equal(e.table[:, :2].nan_to_num(), s.table[:, :2].nan_to_num())


def test_a_second_call_uploads_nothing():
    host, dev, specs = on_device("randn", 33, 64)
    uploads = []

    def upload(a, device):
        uploads.append(a)
        return _fields._upload(a, device)

    regions, _ = twelve(specs)
    regs = Regions(regions, tables=_fields.DeviceTables(upload=upload))
    lat, lon = coords(host[0])
    first = region_scores(dev[0], dev[1], regs)
    n = len(uploads)
    tables = regs.device_tables(lat, lon, DEV)
    assert 2 <= n <= 4 and len(tables) == 2 and all(a.dtype == np.uint8 and a.ndim == 1 for a in uploads)
    assert tables[0][2].shape == (33, 64) and tables[0][2].dtype == torch.uint8 and tables[0][3] == 8 and tables[1][3] == 4
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = region_scores(dev[0], dev[1], regs)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(uploads) == n
    for a, b in zip(tables, regs.device_tables(lat, lon, DEV)):
        assert a[0] is b[0] and a[1] is b[1] and a[2] is b[2]
    assert torch.equal(first.table[..., :8], second.table[..., :8])
    free = Regions({"tropics": Region(lat=(-20, 20)), "box": Region(lon=(10, 50))}, tables=_fields.DeviceTables(upload=upload))
    assert free.device_tables(lat, lon, DEV)[0][2] is None                        # no mask: no plane, a NULL goes down


def nodes_and_edges(graph: torch.cuda.CUDAGraph):
    """(number of nodes, [(from, to), ...]) of a captured graph that was made with keep_graph=True, asked of the HIP runtime
    the process has loaded."""
    with open("/proc/self/maps") as maps:
        hip = ctypes.CDLL(next(line.split()[-1] for line in maps if "libamdhip64" in line))
    size_p, nodes_p = ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_void_p)
    hip.hipGraphGetNodes.argtypes, hip.hipGraphGetEdges.argtypes = [ctypes.c_void_p, nodes_p, size_p], [ctypes.c_void_p, nodes_p, nodes_p, size_p]
    g, n, e = ctypes.c_void_p(graph.raw_cuda_graph()), ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(g, None, ctypes.byref(n)) == 0 and hip.hipGraphGetEdges(g, None, None, ctypes.byref(e)) == 0
    src, dst = (ctypes.c_void_p * e.value)(), (ctypes.c_void_p * e.value)()
    assert hip.hipGraphGetEdges(g, src, dst, ctypes.byref(e)) == 0
    return n.value, list(zip(src, dst))


def test_region_scores_are_capturable_in_a_hip_graph():
    _, (pred, truth, clim), specs = on_device("randn", 33, 64, seed=7)
    pred, truth = (Batch({k: v.clone() for k, v in b.surf_vars.items()}, {}, {k: v.clone() for k, v in b.atmos_vars.items()}, b.metadata)
                   for b in (pred, truth))
    _, (other_pred, other_truth, _), _ = on_device("randn", 33, 64, seed=8)
    regs = Regions(twelve(specs)[0])
    want_first = region_scores(pred, truth, regs, climatology=clim).cpu()          # (also the warm call)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)                                 # (kept: its nodes are counted below)
    with torch.cuda.graph(graph):
        s = region_scores(pred, truth, regs, climatology=clim)
    graph.replay()
    torch.cuda.synchronize()
    same = lambda a, b: torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num())  # noqa: E731
    assert same(s.table.cpu(), want_first.table)
    for group in ("surf_vars", "atmos_vars"):                                     # new values in the static inputs, in place
        for k in getattr(pred, group):
            getattr(pred, group)[k].copy_(getattr(other_pred, group)[k])
            getattr(truth, group)[k].copy_(getattr(other_truth, group)[k])
    graph.replay()
    torch.cuda.synchronize()
    replayed = s.table.cpu()
    assert not same(replayed, want_first.table)
    assert same(replayed, region_scores(pred, truth, regs, climatology=clim).table.cpu())
    # one chain: no node of the captured graph has two successors or two predecessors
    n_nodes, edges = nodes_and_edges(graph)
    print(f"the captured graph: {n_nodes} nodes, {len(edges)} edges")
    assert n_nodes >= 4 and len(edges) == n_nodes - 1                             # two launches of two kernels at the least
    assert len({a for a, _ in edges}) == len(edges) and len({b for _, b in edges}) == len(edges)
    # a cold call during capture is refused (the capture query is injected or patched: nothing is captured here)
    cold = Regions({"band": Region(lat=(-33.3, 44.4))}, tables=_fields.DeviceTables(capturing=lambda: True))
    with pytest.raises(RuntimeError, match="region_scores: call once .* before capturing a graph"):
        region_scores(pred, truth, cold)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="region_scores: call once .* before capturing a graph"):
            region_scores(pred, truth, Regions(twelve(specs)[0]))                 # known tables, a mask plane to be formed


def test_scoring_a_rollout_step_by_step_equals_the_host_path():
    case = CASES["small_b2"]
    model = getattr(aurora_amd, case["cls"])(**case["kwargs"])
    model.load_state_dict(helpers.case_state_dict(model, torch.float32), strict=True)
    model = model.to(DEV).eval()
    surf, static, atmos, lat, lon, times = helpers.case_inputs(case, model.config)
    f = lambda d: {k: v.float() for k, v in d.items()}  # noqa: E731
    batch = Batch(f(surf), f(static), f(atmos), Metadata(lat.float(), lon.float(), times, tuple(case["levels"])))
    truth = batch.crop(model.patch_size)
    truth_dev = truth.to(DEV)
    name = next(iter(truth.static_vars))
    land = truth.static_vars[name] >= truth.static_vars[name].median()
    assert 0 < int(land.sum()) < land.numel()
    boxes = {"global": Region(), "tropics": Region(lat=(-20, 20)), "extratropics": Region(lat=[(-90, -20), (20, 90)]),
             "europe": Region(lat=(35, 75), lon=(-12.5, 42.5))}
    regs = Regions({**boxes, "land": Region(mask=land.to(DEV)), "tropical land": Region(lat=(-20, 20), mask=land.to(DEV))})
    regs_host = {**boxes, "land": Region(mask=land), "tropical land": Region(lat=(-20, 20), mask=land)}
    got, preds = [], []
    with torch.inference_mode():
        for pred in rollout(model, batch.to(DEV), steps=2):
            got.append(region_scores(pred, truth_dev, regs, climatology=truth_dev))   # nothing is read back in the loop
            preds.append(pred)
    got = [s.cpu() for s in got]
    assert len(got) == 2
    for s, pred in zip(got, preds):
        host = region_scores(pred.to("cpu"), truth, regs_host, climatology=truth)
        assert s.regions == host.regions and list(s.rmse) == list(host.rmse)
        a, b = s.table.numpy(), host.table.numpy()
        assert np.array_equal(a[..., 0], b[..., 0]) and (a[..., 0] > 0).all()
        # both sides within the module's bound of the exact sums -> the finalised columns within twice that
        assert (np.abs(a[..., 8] - b[..., 8]) <= 4 * REL * b[..., 8]).all() and (np.abs(a[..., 10] - b[..., 10]) <= 4 * REL * b[..., 10]).all()
        assert (np.abs(a[..., 9] - b[..., 9]) <= 4 * REL * b[..., 10]).all()
        assert np.isnan(a[..., 11]).all() and np.isnan(b[..., 11]).all()          # truth as its own climatology
    assert not torch.equal(got[0].table.nan_to_num(), got[1].table.nan_to_num())


def test_device_path_argument_errors():
    (pred, truth, clim), dev, specs = on_device("randn", 33, 64)
    regs = {"tropics": Region(lat=(-20, 20))}
    with pytest.raises(ValueError, match="cpu.*cuda|cuda.*cpu"):
        region_scores(dev[0], truth, regs)
    with pytest.raises(ValueError, match="cpu.*cuda|cuda.*cpu"):
        region_scores(dev[0], dev[1], regs, climatology=clim)
    with pytest.raises(TypeError, match="^region_scores: truth variable '2t' is torch.float64; the device path scores float32 fields"):
        region_scores(dev[0], dev[1].type(torch.float64), regs)
    tr = Batch(dict(dev[1].surf_vars), {}, dict(dev[1].atmos_vars), dev[1].metadata)
    tr.surf_vars["2t"] = tr.surf_vars["2t"].transpose(-1, -2).contiguous().transpose(-1, -2)
    with pytest.raises(ValueError, match="^region_scores: the planes of truth variable '2t' are not row-major contiguous"):
        region_scores(dev[0], tr, regs)
    on_gpu = torch.from_numpy(specs["land"][2]).to(DEV)
    with pytest.raises(ValueError, match="^region_scores: the mask of region 'land' is on cuda:0 but the fields are on cpu"):
        region_scores(pred, truth, {"land": Region(mask=on_gpu)})
    with pytest.raises(ValueError, match="^region_scores: the mask of region 'land' is on meta but the fields are on cuda:0"):
        region_scores(dev[0], dev[1], {"land": Region(mask=torch.ones(33, 64, dtype=torch.bool, device="meta"))})
    with pytest.raises(ValueError, match="does not fit a 33 x 64 grid"):
        region_scores(dev[0], dev[1], {"land": Region(mask=on_gpu[:, :60])})
    with pytest.raises(AssertionError, match="col_bits must be a contiguous uint8 tensor"):
        lib.region_sums([dev[0].surf_vars["2t"]], [dev[1].surf_vars["2t"]], None, torch.zeros(33, dtype=torch.uint8, device=DEV),
                        torch.zeros(64, dtype=torch.int32, device=DEV), None, 1, w_of(33))
