"""`aurora_amd.sphere_spectra` on the device: one aurora_hip_sphere_spectra call against the long-double yardstick of
tests/test_sphere_spectra_host.py (`yardstick_sphere_spectra`, checked there against a 50-digit evaluation) under the derived
bound `sphere_spectra_bound` of that module's text; at production size against the numpy path under the same bound.

Test fields are those of the zonal spectra: mean 5e4 plus noise with a k^-3 amplitude spectrum, rounded to fp32.  Every value
of every plane of every case is compared; NaN (an invalid plane) must coincide, `valid` and `pole_rows_dropped` are exact."""
import importlib

import numpy as np
import pytest
import torch

from aurora_amd import Batch, diagnostics, sphere_spectra
from aurora_amd.engine import lib
from tests.test_sphere_spectra_host import metadata, sphere_spectra_bound, yardstick_sphere_spectra
from tests.verification_inputs import DEV, carve, red_noise, red_noise_batch

ss = importlib.import_module("aurora_amd.sphere_spectra")
pytestmark = pytest.mark.gpu

LAYOUTS = {
    "descending": lambda H: np.linspace(90, -90, H),
    "ascending": lambda H: np.linspace(-90, 90, H),
    "without poles": lambda H: np.linspace(90 - 90 / H, -90 + 90 / H, H),
    "without the south pole": lambda H: np.linspace(90, -90 + 180 / H, H),
}


def device_table(lat, lmax):
    return torch.from_numpy(np.array(ss.analysis_table(lat, lmax))).to(DEV)


def run(p, t, lat, lmax, offset_floats=0):
    pd = carve(p, offset_floats)
    td = None if t is None else carve(t, offset_floats)
    out = lib.sphere_spectra_power([pd], None if td is None else [td], device_table(lat, lmax), lmax, ss.pole_rows(lat))
    assert np.array_equal(pd.cpu().numpy(), p, equal_nan=True)           # the inputs are not modified
    return out


def check_raw(p, t, lat, lmax, what, offset_floats=0, reference=None):
    """(n_planes, H, N) host arrays through lib.sphere_spectra_power against the yardstick (or `reference`: per-plane power,
    valid, dropped) under the bound."""
    n_planes, H, N = p.shape
    power, valid, dropped = run(p, t, lat, lmax, offset_floats)
    F = 1 if t is None else 3
    assert power.shape == (n_planes, F, lmax + 1) and power.dtype == torch.float64 and power.device == DEV
    assert valid.shape == (n_planes,) and valid.dtype == torch.bool and dropped.shape == (n_planes,) and dropped.dtype == torch.int32
    power, valid, dropped = power.cpu().numpy(), valid.cpu().numpy(), dropped.cpu().numpy()
    for k in range(n_planes):
        tk = None if t is None else t[k]
        want, want_valid, want_dropped = reference(k) if reference else yardstick_sphere_spectra(p[k], tk, lat, lmax)
        assert bool(valid[k]) == want_valid and int(dropped[k]) == want_dropped, (what, k)
        if not want_valid:
            assert np.isnan(power[k]).all(), (what, k)
            continue
        bound = sphere_spectra_bound(p[k], tk, lat, lmax)
        err = np.abs(power[k] - np.asarray(want, dtype=np.float64))
        ratio = float((err / bound).max())
        print(f"{what} plane {k}: max |device - yardstick| / bound = {ratio:.3e}")
        assert not np.isnan(power[k]).any() and (err <= bound).all(), (what, k, ratio)
    return power, valid, dropped


@pytest.mark.parametrize("with_truth", (False, True))
@pytest.mark.parametrize("H", (65, 66, 67, 68))
def test_latitude_steps_of_four(H, with_truth):
    N = 130
    lat = LAYOUTS["descending"](H)
    lmax = ss.largest_lmax(H, N)
    assert lmax == (32 if H < 67 else 33)
    p = red_noise((2, H, N), seed=H)
    check_raw(p, red_noise((2, H, N), seed=H + 100) if with_truth else None, lat, lmax, f"{H}x{N} truth={with_truth}")


@pytest.mark.parametrize("lmax", (15, 16, 17, 31, 32))
def test_degree_tiles_of_sixteen(lmax):
    H, N = 65, 130
    p, t = red_noise((2, H, N), seed=lmax), red_noise((2, H, N), seed=lmax + 50)
    check_raw(p, t, LAYOUTS["descending"](H), lmax, f"lmax={lmax}")


@pytest.mark.parametrize("H,N", [(2, 4), (3, 8), (9, 16), (9, 37)])
@pytest.mark.parametrize("with_truth", (False, True))
def test_tiny_grids(H, N, with_truth):
    lat = LAYOUTS["descending"](H)
    p = red_noise((3, H, N), seed=H + N)
    check_raw(p, red_noise((3, H, N), seed=H + N + 1) if with_truth else None, lat, ss.largest_lmax(H, N), f"{H}x{N}")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_latitude_layouts(layout):
    H, N = 33, 72
    lat = LAYOUTS[layout](H)
    p, t = red_noise((2, H, N), seed=11), red_noise((2, H, N), seed=12)
    p[1, 0, 5] = np.nan                                                  # row 0: a pole in three of the layouts
    _, valid, dropped = check_raw(p, t, lat, 16, layout)
    pole_first = abs(lat[0]) == 90.0
    assert valid.tolist() == [True, pole_first] and dropped.tolist() == [0, int(pole_first)]


@pytest.mark.parametrize("n_planes", (1, 7, 9, 17))
@pytest.mark.parametrize("with_truth", (False, True))
def test_plane_tiles(n_planes, with_truth):
    H, N = 17, 40
    p = red_noise((n_planes, H, N), seed=n_planes)
    t = red_noise((n_planes, H, N), seed=n_planes + 30) if with_truth else None
    check_raw(p, t, LAYOUTS["descending"](H), 8, f"{n_planes} planes truth={with_truth}")


def test_planes_three_floats_past_a_16_byte_boundary_keep_their_bits():
    H, N = 33, 70
    lat = LAYOUTS["descending"](H)
    p, t = red_noise((3, H, N), seed=21), red_noise((3, H, N), seed=22)
    aligned, _, _ = check_raw(p, t, lat, 16, "aligned")
    shifted, _, _ = check_raw(p, t, lat, 16, "three floats on", offset_floats=3)
    assert carve(p, 3).data_ptr() % 16 == 12 and np.array_equal(aligned, shifted)


def test_invalid_values():
    H, N = 33, 72
    lat = LAYOUTS["descending"](H)
    p, t = red_noise((5, H, N), seed=31), red_noise((5, H, N), seed=32)
    base, _, _ = check_raw(p, t, lat, 16, "before")
    p[1, 7, 3] = np.nan                                                  # a NaN plane among valid ones
    p[2, 0], t[2, H - 1, N - 1] = np.nan, np.nan                         # NaN pole rows, one of them in the truth alone
    t[3, 20, 36] = np.inf
    p[4, 32, 0] = -np.inf                                                # -Inf in a pole row: dropped
    got, valid, dropped = check_raw(p, t, lat, 16, "after")
    assert valid.tolist() == [True, False, True, False, True] and dropped.tolist() == [0, 0, 2, 0, 1]
    assert np.array_equal(got[0], base[0]) and not np.array_equal(got[2], base[2])     # the neighbours keep their bits
    _, valid1, dropped1 = check_raw(p, None, lat, 16, "without the truth")
    assert valid1.tolist() == [True, False, True, True, True] and dropped1.tolist() == [0, 0, 1, 0, 1]


def test_a_plane_has_the_same_bits_alone_among_three_and_last_of_seven_and_calls_repeat():
    H, N, lmax = 67, 130, 33
    lat = LAYOUTS["descending"](H)
    p, t = red_noise((7, H, N), seed=41), red_noise((7, H, N), seed=42)
    table, poles = device_table(lat, lmax), ss.pole_rows(lat)
    pd, td = carve(p), carve(t)
    for truth in (None, td):
        call = lambda sl: lib.sphere_spectra_power([pd[sl]], None if truth is None else [truth[sl]], table, lmax, poles)  # noqa: E731
        seven, again = call(slice(0, 7)), call(slice(0, 7))
        alone, three = call(slice(6, 7)), call(slice(4, 7))
        first = call(slice(0, 3))
        torch.cuda.synchronize()
        for i in range(3):
            assert seven[i].cpu().numpy().tobytes() == again[i].cpu().numpy().tobytes(), "two calls differ"
            assert torch.equal(alone[i][0], seven[i][6]) and torch.equal(three[i][2], seven[i][6]), "a plane depends on its neighbours"
            assert torch.equal(first[i], seven[i][:3])


def test_a_replayed_graph_gives_the_same_bytes():
    pred, truth = (b.to(DEV) for b in (red_noise_batch(33, 64, seed=7), red_noise_batch(33, 64, seed=8)))
    other = red_noise_batch(33, 64, seed=9).to(DEV)
    first = sphere_spectra(pred, truth).cpu()                            # (the warm call: the tables are uploaded)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = sphere_spectra(pred, truth)
    graph.replay()
    torch.cuda.synchronize()
    assert s.table.cpu().numpy().tobytes() == first.table.numpy().tobytes() and torch.equal(s.valid_table.cpu(), first.valid_table)
    for grp in ("surf_vars", "atmos_vars"):
        for k, v in getattr(pred, grp).items():
            v.copy_(getattr(other, grp)[k])
    graph.replay()
    torch.cuda.synchronize()
    replayed = s.table.cpu()
    assert not torch.equal(replayed, first.table) and torch.equal(replayed, sphere_spectra(pred, truth).table.cpu())


@pytest.mark.parametrize("with_truth", (False, True))
def test_guard_words_around_every_output_and_the_workspace(with_truth):
    n, H, N, lmax = 3, 45, 90, 20
    lat = LAYOUTS["descending"](H)
    p, t = carve(red_noise((n, H, N), seed=51)), carve(red_noise((n, H, N), seed=52))
    table = device_table(lat, lmax)
    want = lib.sphere_spectra_power([p], [t] if with_truth else None, table, lmax, 3)
    need = lib.sphere_spectra_workspace_bytes(n, H, N, lmax, with_truth)
    assert need > 0 and need % 16 == 0
    F, guard = 3 if with_truth else 1, 4096
    sizes = {"power": n * F * (lmax + 1) * 8, "valid": n, "dropped": n * 4, "workspace": need}
    bufs = {k: torch.full((guard + v + guard,), 0xA5, dtype=torch.uint8, device=DEV) for k, v in sizes.items()}
    at = {k: b.data_ptr() + guard for k, b in bufs.items()}
    assert all(b.data_ptr() % 16 == 0 for b in bufs.values())
    ptrs = torch.tensor([x[k].data_ptr() for x in (p, t) for k in range(n)], dtype=torch.int64).to(DEV)
    L = lib.load()
    code = L.aurora_hip_sphere_spectra(ptrs.data_ptr(), ptrs.data_ptr() + 8 * n if with_truth else None, n, H, N, lmax, 3,
                                       table.data_ptr(), lib.spectra_twiddle(N, DEV).data_ptr(), at["power"], at["valid"],
                                       at["dropped"], at["workspace"], need, torch.cuda.current_stream().cuda_stream)
    assert code == 0, L.aurora_hip_last_error()
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert (b[:guard] == 0xA5).all() and (b[guard + sizes[k]:] == 0xA5).all(), f"the call wrote outside {k}"
    body = lambda k: bufs[k][guard:guard + sizes[k]]  # noqa: E731
    assert torch.equal(body("power").view(torch.float64).view(n, F, lmax + 1), want[0])
    assert torch.equal(body("valid").view(torch.bool), want[1]) and torch.equal(body("dropped").view(torch.int32), want[2])


def numpy_reference(p, t, lat, lmax):
    power, valid, dropped = ss._power_host(p, t, lat, lmax)
    return lambda k: (power[k], bool(valid[k]), int(dropped[k]))


def test_production_size_with_a_truth():
    H, N, lmax = 721, 1440, 360
    lat = LAYOUTS["descending"](H)
    p, t = red_noise((2, H, N), seed=61), red_noise((2, H, N), seed=62)
    check_raw(p, t, lat, lmax, "721x1440", reference=numpy_reference(p, t, lat, lmax))


def test_production_size_of_the_720_row_grid():
    H, N, lmax = 720, 1440, 359
    lat = np.linspace(90, -89.75, H)
    p = red_noise((1, H, N), seed=63)
    check_raw(p, None, lat, lmax, "720x1440", reference=numpy_reference(p, None, lat, lmax))


def test_the_public_function_on_a_gpu_batch_and_kinetic_energy_from_diagnostics():
    pred, truth = red_noise_batch(33, 64, seed=3), red_noise_batch(33, 64, seed=4)
    s = sphere_spectra(pred.to(DEV), truth.to(DEV))
    assert s.power["2t"].device == DEV and s.power["2t"].shape == (2, 17) and s.power["z"].shape == (2, 3, 17)
    assert s.valid["z"].shape == (2, 3) and s.pole_rows_dropped["2t"].shape == (2,) and s.degree.device == DEV
    host = sphere_spectra(pred, truth)
    lat = pred.metadata.lat.numpy()
    for k in ("2t", "msl", "z"):
        x, y = pred.surf_vars.get(k, pred.atmos_vars.get(k))[:, -1].numpy(), truth.surf_vars.get(k, truth.atmos_vars.get(k))[:, -1].numpy()
        for idx in np.ndindex(*x.shape[:-2]):
            bound = sphere_spectra_bound(x[idx], y[idx], lat, 16)
            have = torch.stack([s.power[k][idx], s.truth_power[k][idx], s.error_power[k][idx]]).cpu().numpy()
            want = torch.stack([host.power[k][idx], host.truth_power[k][idx], host.error_power[k][idx]]).numpy()
            assert (np.abs(have - want) <= bound).all(), (k, idx)
    assert torch.equal(s.ratio["z"], s.power["z"] / s.truth_power["z"])
    # vorticity and divergence of `diagnostics` carry NaN pole rows: dropped, counted, and the energy is finite
    g = torch.Generator().manual_seed(5)
    wind = lambda: (10.0 * torch.randn(2, 1, 3, 33, 64, generator=g)).to(DEV)  # noqa: E731
    b = Batch({}, {}, {"u": wind(), "v": wind()}, metadata(np.linspace(90, -90, 33), 64, B=2, levels=(100, 500, 850))).to(DEV)
    d = diagnostics(b, ("vo", "d"))
    assert torch.isnan(d.atmos_vars["vo"][..., 0, :]).all()
    sd = sphere_spectra(d, only=("vo", "d"))
    assert sd.valid["vo"].all() and (sd.pole_rows_dropped["vo"] == 2).all() and (sd.pole_rows_dropped["d"] == 2).all()
    e = sd.kinetic_energy()
    assert e.shape == (2, 3, 17) and e.device == DEV and torch.isfinite(e).all() and (e[..., 0] == 0).all() and (e[..., 1:] > 0).all()
    assert torch.equal(e.cpu(), sd.cpu().kinetic_energy())               # the same bits on either device
    with pytest.raises(ValueError, match="cpu.*cuda|cuda.*cpu"):
        sphere_spectra(pred.to(DEV), truth)


def test_c_entry_refusals():
    n, H, N, lmax = 2, 17, 32, 8
    lat = LAYOUTS["descending"](H)
    p = carve(red_noise((n, H, N), seed=71))
    table, tw = device_table(lat, lmax), lib.spectra_twiddle(N, DEV)
    need = lib.sphere_spectra_workspace_bytes(n, H, N, lmax, False)
    ws = torch.empty(need + 16, dtype=torch.uint8, device=DEV)
    power = torch.empty(n, 1, lmax + 1, dtype=torch.float64, device=DEV)
    valid, dropped = torch.empty(n, dtype=torch.uint8, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV)
    ptrs = torch.tensor([p[k].data_ptr() for k in range(n)], dtype=torch.int64).to(DEV)
    L = lib.load()

    def call(**kw):
        a = dict(planes=ptrs.data_ptr(), H=H, N=N, lmax=lmax, table=table.data_ptr(), power=power.data_ptr(), ws=ws.data_ptr(),
                 nbytes=need)
        a.update(kw)
        code = L.aurora_hip_sphere_spectra(a["planes"], None, n, a["H"], a["N"], a["lmax"], 3, a["table"], tw.data_ptr(), a["power"],
                                           valid.data_ptr(), dropped.data_ptr(), a["ws"], a["nbytes"],
                                           torch.cuda.current_stream().cuda_stream)
        return code, L.aurora_hip_last_error()

    assert call()[0] == 0
    for kw, word in ((dict(planes=None), b"null"), (dict(table=None), b"null"), (dict(power=None), b"null"), (dict(ws=None), b"null"),
                     (dict(ws=ws.data_ptr() + 8), b"misaligned"), (dict(power=power.data_ptr() + 4), b"misaligned"),
                     (dict(nbytes=need - 16), b"workspace holds"), (dict(lmax=9), b"lmax must be in 0..8"),
                     (dict(lmax=-1), b"lmax must be in 0..8"), (dict(N=16), b"lmax must be in 0..7"),
                     (dict(H=1441, N=1442, lmax=720, nbytes=1 << 40), b"largest lmax that fits is 430")):
        code, msg = call(**kw)
        assert code == -1 and word in msg, (kw, msg)
    torch.cuda.synchronize()
