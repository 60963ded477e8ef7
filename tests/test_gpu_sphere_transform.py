"""`aurora_amd.sphere_transform` on the device: aurora_hip_sphere_analysis and aurora_hip_sphere_synthesis against the
long-double yardsticks of tests/test_sphere_transform_host.py (checked there against a 50-digit evaluation) under the derived
bounds of that module's text; at production size against the numpy path under the same bounds.

Coefficients are checked through `lib.sphere_analysis`; fields through `lib.sphere_synthesis` fed the YARDSTICK's coefficients
rounded to fp64, so that neither stage hides the other's error.  Test fields are those of the spectra tests: mean 5e4 plus
noise with a k^-3 amplitude spectrum, rounded to fp32.  Every value of every plane of every case is compared; NaN (an invalid
plane) must coincide, `valid` and `pole_rows_dropped` are exact."""
import importlib

import numpy as np
import pytest
import torch

from aurora_amd import Batch, diagnostics, sphere_analysis, sphere_filter, sphere_synthesis
from aurora_amd.engine import lib
from tests.test_gpu_sphere_spectra import LAYOUTS
from tests.test_sphere_spectra_host import metadata
from tests.test_sphere_transform_host import (coefficient_bound, field_bound, parts, yardstick_analysis, yardstick_synthesis)
from tests.verification_inputs import DEV, carve, red_noise, red_noise_batch

ss = importlib.import_module("aurora_amd.sphere_spectra")
st = importlib.import_module("aurora_amd.sphere_transform")
pytestmark = pytest.mark.gpu


def tables(lat, lmax):
    return (torch.from_numpy(np.array(ss.analysis_table(lat, lmax))).to(DEV), torch.from_numpy(np.array(st.synthesis_table(lat, lmax))).to(DEV))


def check_analysis(p, lat, lmax, what, offset_floats=0, reference=None):
    """(n_planes, H, N) host array through lib.sphere_analysis against the yardstick (or `reference`: per-plane a[re / im], valid,
    dropped) under D: the coefficients as a complex host array, valid, dropped."""
    n_planes, H, N = p.shape
    pd = carve(p, offset_floats)
    a, valid, dropped = lib.sphere_analysis([pd], tables(lat, lmax)[0], lmax, ss.pole_rows(lat))
    assert np.array_equal(pd.cpu().numpy(), p, equal_nan=True)           # the inputs are not modified
    assert a.shape == (n_planes, lmax + 1, lmax + 1) and a.dtype == torch.complex128 and a.device == DEV
    assert valid.shape == (n_planes,) and valid.dtype == torch.bool and dropped.shape == (n_planes,) and dropped.dtype == torch.int32
    a, valid, dropped = a.cpu().numpy(), valid.cpu().numpy(), dropped.cpu().numpy()
    live = np.triu(np.ones((lmax + 1, lmax + 1), dtype=bool))
    for k in range(n_planes):
        want, want_valid, want_dropped = reference(k) if reference else yardstick_analysis(p[k], lat, lmax)
        assert bool(valid[k]) == want_valid and int(dropped[k]) == want_dropped, (what, k)
        if not want_valid:
            assert np.isnan(a[k].real).all() and np.isnan(a[k].imag).all(), (what, k)
            continue
        D = coefficient_bound(p[k], lat, lmax)
        err = np.hypot(a[k].real - np.asarray(want[0], dtype=np.float64), a[k].imag - np.asarray(want[1], dtype=np.float64))
        ratio = float((err[live] / D[live]).max())
        print(f"{what} plane {k}: coefficients max |device - yardstick| / bound = {ratio:.3e}")
        assert not np.isnan(err).any() and (err <= D).all() and (a[k][~live] == 0).all(), (what, k, ratio)
    return a, valid, dropped


def check_synthesis(b, lat, N, lmax, what, offset_floats=0, reference=None, valid=None):
    """(n_planes, lmax + 1, lmax + 1) complex fp64 host coefficients through lib.sphere_synthesis against the yardstick's field
    of the same coefficients (or `reference`) under the field bound: the fields as a host array."""
    n_planes, H = b.shape[0], len(lat)
    bd = torch.from_numpy(b).to(DEV)
    out = carve(np.zeros((n_planes, H, N), dtype=np.float32), offset_floats, fill=7.0)
    vd = None if valid is None else torch.from_numpy(np.asarray(valid)).to(DEV)
    y = lib.sphere_synthesis(bd, tables(lat, lmax)[1], N, vd, out=out)
    assert y.data_ptr() == out.data_ptr() and y.shape == (n_planes, H, N) and y.dtype == torch.float32
    assert np.array_equal(bd.cpu().numpy(), b, equal_nan=True)           # the inputs are not modified
    y = y.cpu().numpy()
    for k in range(n_planes):
        if valid is not None and not valid[k]:
            assert np.isnan(y[k]).all(), (what, k)
            continue
        bk = parts(b[k])
        want = reference(k) if reference else yardstick_synthesis(bk, lat, N, lmax)
        bound = field_bound(bk, None, lat, N, lmax, want)
        err = np.abs(y[k].astype(np.float64) - np.asarray(want, dtype=np.float64))
        ratio = float((err / bound).max())
        print(f"{what} plane {k}: field max |device - yardstick| / bound = {ratio:.3e}")
        assert not np.isnan(y[k]).any() and (err <= bound).all(), (what, k, ratio)
    return y


def yardstick_coefficients(p, lat, lmax):
    """The yardstick's coefficients of every plane, rounded to fp64: (n_planes, lmax + 1, lmax + 1) complex128."""
    a = [yardstick_analysis(x, lat, lmax)[0].astype(np.float64) for x in p]
    return np.stack([x[0] + 1j * x[1] for x in a])


def both(p, lat, lmax, what, offset_floats=0):
    a, valid, dropped = check_analysis(p, lat, lmax, what, offset_floats)
    y = check_synthesis(yardstick_coefficients(p, lat, lmax), lat, p.shape[-1], lmax, what, offset_floats)
    return a, y


@pytest.mark.parametrize("H", (65, 66, 67, 68))
def test_latitude_steps_of_four_and_tiles_of_sixteen(H):
    N = 130
    both(red_noise((2, H, N), seed=H), LAYOUTS["descending"](H), ss.largest_lmax(H, N), f"{H}x{N}")


@pytest.mark.parametrize("lmax", (15, 16, 17, 31, 32))
def test_degree_tiles_and_segments(lmax):
    H, N = 65, 130
    both(red_noise((2, H, N), seed=lmax), LAYOUTS["descending"](H), lmax, f"lmax={lmax}")


@pytest.mark.parametrize("H,N", [(2, 4), (3, 8), (9, 16), (9, 37)])
def test_tiny_and_odd_grids_fold_both_ways(H, N):
    """(9, 16) has the columns n = 0 and n = N/2 without a mirror column, (9, 37) only n = 0."""
    both(red_noise((3, H, N), seed=H + N), LAYOUTS["descending"](H), ss.largest_lmax(H, N), f"{H}x{N}")


@pytest.mark.parametrize("N", (1538, 4096))
def test_more_column_tiles_than_one_pass_and_the_widest_grid(N):
    """The inverse tile keeps 768 columns a pass: N = 1538 has 770 columns n = 0 .. N/2, two passes; 4096 is the widest grid."""
    H, lmax = 9, 4
    both(red_noise((2, H, N), seed=N), LAYOUTS["descending"](H), lmax, f"{H}x{N}")


@pytest.mark.parametrize("n_planes", (1, 7, 9, 17))
def test_plane_tiles(n_planes):
    H, N = 17, 40
    both(red_noise((n_planes, H, N), seed=n_planes), LAYOUTS["descending"](H), 8, f"{n_planes} planes")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_latitude_layouts(layout):
    H, N = 33, 72
    lat = LAYOUTS[layout](H)
    p = red_noise((2, H, N), seed=11)
    p[1, 0, 5] = np.nan                                                  # row 0: a pole in three of the layouts
    _, valid, dropped = check_analysis(p, lat, 16, layout)
    pole_first = abs(lat[0]) == 90.0
    assert valid.tolist() == [True, pole_first] and dropped.tolist() == [0, int(pole_first)]
    check_synthesis(yardstick_coefficients(p[:1], lat, 16), lat, N, 16, layout)


def test_planes_three_floats_past_a_16_byte_boundary_keep_their_bits():
    H, N = 33, 70
    lat = LAYOUTS["descending"](H)
    p = red_noise((3, H, N), seed=21)
    a0, y0 = both(p, lat, 16, "aligned")
    a3, y3 = both(p, lat, 16, "three floats on", offset_floats=3)
    assert carve(p, 3).data_ptr() % 16 == 12 and np.array_equal(a0, a3) and np.array_equal(y0, y3)


def test_invalid_values():
    H, N, lmax = 33, 72, 16
    lat = LAYOUTS["descending"](H)
    p = red_noise((5, H, N), seed=31)
    base, _, _ = check_analysis(p, lat, lmax, "before")
    p[1, 7, 3] = np.nan                                                  # a NaN plane among valid ones
    p[2, 0], p[2, H - 1] = np.nan, np.nan                                # NaN pole rows, as diagnostics("vo") leaves them
    p[4, 32, 0] = -np.inf                                                # -Inf in a pole row: dropped
    got, valid, dropped = check_analysis(p, lat, lmax, "after")
    assert valid.tolist() == [True, False, True, True, True] and dropped.tolist() == [0, 0, 2, 0, 1]
    assert np.array_equal(got[0], base[0]) and np.array_equal(got[3], base[3]) and not np.array_equal(got[2], base[2])
    # the synthesis of those coefficients: NaN for the invalid plane alone, finite poles, the neighbours keep their bits
    yb = lib.sphere_synthesis(torch.from_numpy(base).to(DEV), tables(lat, lmax)[1], N).cpu().numpy()
    y = lib.sphere_synthesis(torch.from_numpy(got).to(DEV), tables(lat, lmax)[1], N, torch.from_numpy(valid).to(DEV)).cpu().numpy()
    assert np.isnan(y[1]).all() and np.isfinite(y[[0, 2, 3, 4]]).all() and np.array_equal(y[0], yb[0]) and np.array_equal(y[3], yb[3])
    # valid given for finite coefficients: the plane marked invalid is NaN, the others as without it
    mask = np.array([True, True, False, True, True])
    ym = check_synthesis(base, lat, N, lmax, "masked", valid=mask)
    assert np.array_equal(ym[[0, 1, 3, 4]], yb[[0, 1, 3, 4]])


def test_a_plane_has_the_same_bits_alone_among_three_and_last_of_seven_and_calls_repeat():
    H, N, lmax = 67, 130, 33
    lat = LAYOUTS["descending"](H)
    p = carve(red_noise((7, H, N), seed=41))
    A, P = tables(lat, lmax)
    poles = ss.pole_rows(lat)
    ana = lambda sl: lib.sphere_analysis([p[sl]], A, lmax, poles)  # noqa: E731
    seven, again, alone, three, first = ana(slice(0, 7)), ana(slice(0, 7)), ana(slice(6, 7)), ana(slice(4, 7)), ana(slice(0, 3))
    b = seven[0]
    syn = lambda sl: lib.sphere_synthesis(b[sl].contiguous(), P, N)  # noqa: E731
    y7, y7again, y1, y3, yf = syn(slice(0, 7)), syn(slice(0, 7)), syn(slice(6, 7)), syn(slice(4, 7)), syn(slice(0, 3))
    torch.cuda.synchronize()
    raw = lambda t: (torch.view_as_real(t) if t.is_complex() else t).cpu().numpy().tobytes()  # noqa: E731
    for i in range(3):
        assert raw(seven[i]) == raw(again[i]), "two calls differ"
        assert raw(alone[i][0]) == raw(seven[i][6]) and raw(three[i][2]) == raw(seven[i][6]), "a plane depends on its neighbours"
        assert raw(first[i]) == raw(seven[i][:3])
    assert raw(y7) == raw(y7again) and raw(y1[0]) == raw(y7[6]) and raw(y3[2]) == raw(y7[6]) and raw(yf) == raw(y7[:3])


def test_a_replayed_graph_of_sphere_filter_gives_the_same_bytes():
    x, other = red_noise_batch(33, 64, seed=7).to(DEV), red_noise_batch(33, 64, seed=9).to(DEV)
    l = np.arange(13)
    h = np.exp(-l * (l + 1) * 0.1 ** 2)
    every = lambda b: torch.cat([v.reshape(-1) for v in (*b.surf_vars.values(), *b.atmos_vars.values())]).cpu()  # noqa: E731
    first = every(sphere_filter(x, response=h))                          # (the warm call: the tables are uploaded)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = sphere_filter(x, response=h)
    graph.replay()
    torch.cuda.synchronize()
    assert every(y).numpy().tobytes() == first.numpy().tobytes()
    for grp in ("surf_vars", "atmos_vars"):
        for k, v in getattr(x, grp).items():
            v.copy_(getattr(other, grp)[k])
    graph.replay()
    torch.cuda.synchronize()
    replayed = every(y)
    assert not torch.equal(replayed, first) and torch.equal(replayed, every(sphere_filter(x, response=h)))


def test_sphere_filter_on_the_device_against_the_cpu_path():
    """Both paths are within their bound of the rule's field of the rule's coefficients: the difference is within the sum."""
    x = red_noise_batch(33, 64, seed=3)
    lat, N, L = x.metadata.lat.numpy(), 64, 10
    dev, host = sphere_filter(x.to(DEV), lmax=L, lmin=2), sphere_filter(x, lmax=L, lmin=2)
    assert dev.surf_vars["2t"].device == DEV and dev.surf_vars["2t"].shape == (2, 1, 33, N) and dev.atmos_vars["z"].shape == (2, 1, 3, 33, N)
    assert dev.static_vars.keys() == x.static_vars.keys() and dev.surf_vars["2t"].dtype == torch.float32
    c = sphere_analysis(x, lmax=L)
    h = (np.arange(L + 1) >= 2).astype(np.float64)
    for k in ("2t", "msl", "z"):
        src = (x.surf_vars.get(k, x.atmos_vars.get(k)))[:, -1].numpy()
        d, w = (b.surf_vars.get(k, b.atmos_vars.get(k))[:, 0].cpu().numpy().astype(np.float64) for b in (dev, host))
        for idx in np.ndindex(*src.shape[:-2]):
            bound = field_bound(parts(c.coeff[k][idx].numpy() * h), coefficient_bound(src[idx], lat, L), lat, N, L, w[idx])
            ratio = float((np.abs(d[idx] - w[idx]) / (2 * bound)).max())
            print(f"{k}{idx}: max |device - cpu| / (sum of both bounds) = {ratio:.3e}")
            assert ratio <= 1, (k, idx)
    # coefficients, their power and a synthesis of coefficients changed in torch, on the device
    cd = sphere_analysis(x.to(DEV), lmax=L)
    assert cd.coeff["z"].device == DEV and cd.coeff["z"].shape == (2, 3, L + 1, L + 1) and cd.degree.device == DEV
    assert torch.equal(torch.view_as_real(cd.scaled(h).table).cpu(), torch.view_as_real(cd.cpu().scaled(h).table))   # the same bits on either device
    assert sphere_synthesis(cd.scaled(h)).surf_vars["2t"].cpu().numpy().tobytes() == dev.surf_vars["2t"].cpu().numpy().tobytes()
    assert cd.power()["2t"].shape == (2, L + 1)
    # vorticity of `diagnostics` carries NaN pole rows: dropped, counted, and the filtered field has finite poles
    g = torch.Generator().manual_seed(5)
    wind = lambda: (10.0 * torch.randn(2, 1, 3, 33, 64, generator=g)).to(DEV)  # noqa: E731
    b = Batch({}, {}, {"u": wind(), "v": wind()}, metadata(np.linspace(90, -90, 33), 64, B=2, levels=(100, 500, 850))).to(DEV)
    vo = diagnostics(b, ("vo",))
    assert torch.isnan(vo.atmos_vars["vo"][..., 0, :]).all()
    cv = sphere_analysis(vo, only="vo")
    assert cv.valid["vo"].all() and (cv.pole_rows_dropped["vo"] == 2).all()
    assert torch.isfinite(sphere_filter(vo, lmax=8).atmos_vars["vo"]).all()
    with pytest.raises(ValueError, match="cpu.*cuda|cuda.*cpu"):
        sphere_analysis(Batch({"a": x.surf_vars["2t"].to(DEV), "b": x.surf_vars["msl"]}, {}, {}, x.metadata))


def test_guard_words_around_every_output_and_the_workspaces():
    n, H, N, lmax = 3, 45, 90, 20
    lat = LAYOUTS["descending"](H)
    p = carve(red_noise((n, H, N), seed=51))
    A, P = tables(lat, lmax)
    want_a, want_valid, want_dropped = lib.sphere_analysis([p], A, lmax, 3)
    want_y = lib.sphere_synthesis(want_a, P, N, want_valid)
    need_a, need_s = lib.sphere_analysis_workspace_bytes(n, H, N, lmax), lib.sphere_synthesis_workspace_bytes(n, H, N, lmax)
    assert need_a > 0 and need_a % 16 == 0 and need_s > 0 and need_s % 16 == 0
    guard = 4096
    sizes = {"coeff": n * (lmax + 1) ** 2 * 16, "valid": n, "dropped": n * 4, "ws_a": need_a, "out": n * H * N * 4, "ws_s": need_s}
    bufs = {k: torch.full((guard + v + guard,), 0xA5, dtype=torch.uint8, device=DEV) for k, v in sizes.items()}
    at = {k: b.data_ptr() + guard for k, b in bufs.items()}
    ptrs = torch.tensor([p[k].data_ptr() for k in range(n)], dtype=torch.int64).to(DEV)
    L, tw, stream = lib.load(), lib.spectra_twiddle(N, DEV).data_ptr(), torch.cuda.current_stream().cuda_stream
    code = L.aurora_hip_sphere_analysis(ptrs.data_ptr(), n, H, N, lmax, 3, A.data_ptr(), tw, at["coeff"], at["valid"], at["dropped"],
                                        at["ws_a"], need_a, stream)
    assert code == 0, L.aurora_hip_last_error()
    code = L.aurora_hip_sphere_synthesis(at["coeff"], at["valid"], n, H, N, lmax, P.data_ptr(), tw, at["out"], at["ws_s"], need_s, stream)
    assert code == 0, L.aurora_hip_last_error()
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert (b[:guard] == 0xA5).all() and (b[guard + sizes[k]:] == 0xA5).all(), f"the calls wrote outside {k}"
    body = lambda k: bufs[k][guard:guard + sizes[k]]  # noqa: E731
    assert torch.equal(body("coeff").view(torch.float64).view(n, lmax + 1, lmax + 1, 2), torch.view_as_real(want_a))   # every element written
    assert torch.equal(body("valid").view(torch.bool), want_valid) and torch.equal(body("dropped").view(torch.int32), want_dropped)
    assert torch.equal(body("out").view(torch.float32).view(n, H, N), want_y)


def test_production_size():
    H, N, lmax = 721, 1440, 360
    lat = LAYOUTS["descending"](H)
    p = red_noise((2, H, N), seed=61)
    a, valid, dropped = st._analysis_host(p, lat, lmax)
    check_analysis(p, lat, lmax, "721x1440", reference=lambda k: (parts(a[k]), bool(valid[k]), int(dropped[k])))
    # (the numpy field before its rounding to fp32 stands in for the yardstick's, as the numpy spectra do at this size)
    y = st._field_host(a, lat, N, lmax)
    check_synthesis(a, lat, N, lmax, "721x1440", reference=lambda k: y[k])
