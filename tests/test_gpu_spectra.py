"""`aurora_amd.spectra` on the device: one aurora_hip_spectra call against the numpy fp64 yardstick of
tests/test_spectra_host.py (`yardstick_spectra`: np.fft.rfft and explicit loops, checked there against a long-double DFT).

Test fields have a realistic offset and tail: mean 5e4 plus noise with a k^-3 amplitude spectrum, rounded to fp32.

Bound (derived, not tuned; `spectra_bound` of tests/test_spectra_host.py evaluates it), with u = 2^-53:
  * A row's transform.  The kernel folds the row (p[j] = x[j] + x[N-j], m[j] = x[j] - x[N-j]: one rounding each, relative u)
    and accumulates at most N/2 + 1 products p[j] cos / m[j] sin recursively in the MFMA's fp64 accumulator, against table
    entries computed on the host to within 2 ulp.  Recursive summation of n terms is within n u sum|term|; here
    sum|term| <= sum_n |x[n]| for the cosine and for the sine sum (|p[j]|, |m[j]| <= |x[j]| + |x[N-j]|, |cos|, |sin| <= 1), so
    each of Re X, Im X is within (N/2 + 1 + 1 + 2 + 1) u sum|x| and |X^ - X| <= sqrt(2) (N/2 + 5) u sum|x| <= E,
        E_i = (N + 8) u sum_n |x_i[n]|.
  * A row's power.  | |X^|^2 - |X|^2 | <= 2 |X| E + E^2, so |P^_i[k] - P_i[k]| <= c_k (2 |X_i[k]| E_i + E_i^2) / N^2; the few
    roundings of squaring, adding and scaling (relative 4 u of P) are inside the slack between (N + 8) and sqrt(2) (N/2 + 5).
  * The error field is taken as X_pred - X_truth in the epilogue, so its E_i is E_i(pred) + E_i(truth): the transform errors
    of both rows, not (N + 8) u sum|pred - truth|.
  * The band mean carries the row bounds through with the same weights, plus (n_lat + 4) u S_b[k] for the weighted row
    reduction and the division (at most n_lat nonnegative terms in a fixed order).
The yardstick's own error is under a tenth of this bound (tests/test_spectra_host.py).  Every value of every plane of every
case is compared; NaN (an empty band) must coincide, and `rows` is exact."""
import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, Metadata, rollout, spectra
from aurora_amd.engine import lib
from aurora_amd.spectra import band_weights
from tests import helpers
from tests.golden_cases import CASES
from tests.test_spectra_host import spectra_bound, yardstick_spectra
from tests.verification_inputs import DEV, carve, planes_of, red_noise, red_noise_batch

pytestmark = pytest.mark.gpu


def lats(n_lat):
    return np.linspace(90, -90, n_lat) if n_lat > 1 else np.zeros(1)


def bands_for(n):
    return (((-90, 90), (-30, 30), (20, 90), (-90, -60), (1.0, 1.5), (0, 0), (45, 90), (-10, 80)))[:n]


def check_raw(p: np.ndarray, t, n_bands, what, offset_floats=0):
    """(n_planes, n_lat, N) host arrays through lib.spectra_power against the yardstick under the bound."""
    n_planes, n_lat, N = p.shape
    lat, bands = lats(n_lat), bands_for(n_bands)
    bw = torch.from_numpy(band_weights(lat, bands)).to(DEV)
    pd = carve(p, offset_floats)
    td = None if t is None else carve(t, offset_floats)
    power, rows = lib.spectra_power([pd], None if td is None else [td], bw)
    assert power.shape == (n_planes, 1 if t is None else 3, n_bands, N // 2 + 1) and power.dtype == torch.float64
    assert rows.shape == (n_planes, n_bands) and rows.dtype == torch.int64 and power.device == DEV
    power, rows = power.cpu().numpy(), rows.cpu().numpy()
    assert np.array_equal(pd.cpu().numpy(), p, equal_nan=True)           # the inputs are not modified
    worst = 0.0
    for k in range(n_planes):
        want, want_rows = yardstick_spectra(p[k], None if t is None else t[k], lat, bands)
        bound = spectra_bound(p[k], None if t is None else t[k], lat, bands, want)
        assert rows[k].tolist() == want_rows.tolist(), (what, k)
        assert np.array_equal(np.isnan(power[k]), np.isnan(want)), (what, k)
        ok = ~np.isnan(want)
        err = np.abs(power[k] - want)[ok]
        ratio = float((err / bound[ok]).max()) if ok.any() else 0.0
        worst = max(worst, ratio)
        print(f"{what} plane {k}: max |device - yardstick| / bound = {ratio:.3e}")
        assert (err <= bound[ok]).all(), (what, k, ratio)
    return power, rows, worst


@pytest.mark.parametrize("n_planes,n_lat,N,n_bands,with_truth,offset", [
    (3, 17, 32, 1, False, 0),
    (3, 17, 45, 3, True, 0),          # odd N
    (2, 1, 900, 2, True, 0),          # one row
    (2, 721, 1440, 1, True, 0),       # 0.25 degrees
    (2, 721, 1440, 8, False, 3),      # eight bands, planes three floats past a 16-byte boundary
    (2, 17, 3600, 2, True, 1),        # 0.1 degrees: three passes over the column tiles
    (2, 17, 900, 5, False, 0),
    (1, 1, 32, 1, True, 0), (4, 17, 2, 1, True, 0), (1, 40, 4096, 1, True, 0),
])
def test_raw_spectra_equal_the_yardstick(n_planes, n_lat, N, n_bands, with_truth, offset):
    p = red_noise((n_planes, n_lat, N), seed=n_lat + N)
    t = red_noise((n_planes, n_lat, N), seed=n_lat + N + 1) if with_truth else None
    check_raw(p, t, n_bands, f"{n_planes}x{n_lat}x{N} bands={n_bands} truth={with_truth}", offset)


def test_invalid_rows_as_on_the_host():
    """NaN / Inf anywhere in a row of pred or truth removes that row from every field; `rows` is exact; the other bands and
    planes keep their bits.  Every band but the deliberately empty one keeps more than half its rows."""
    n_lat, N = 40, 90
    p, t = red_noise((4, n_lat, N), seed=1), red_noise((4, n_lat, N), seed=2)
    base, base_rows, _ = check_raw(p, t, 5, "before masking")
    p[0, 3, 0] = np.nan
    p[0, 9, N - 1] = np.inf
    t[0, 12, 44] = -np.inf
    t[1, 30:36] = np.nan                                                # rows 30-35: a whole tile-straddling block
    p[2, 39, 45] = np.nan                                               # (N / 2: the unpaired column)
    got, rows, _ = check_raw(p, t, 5, "masked")
    assert rows[:, 0].tolist() == [37, 34, 39, 40] and (rows[:, 4] == 0).all()
    assert (rows[:, :4] * 2 > base_rows[:, :4]).all()
    assert np.array_equal(got[3], base[3], equal_nan=True)
    assert np.array_equal(got[1][:, 2], base[1][:, 2]) and not np.array_equal(got[1][:, 0], base[1][:, 0])   # band (20, 90)
    # a whole-NaN plane: NaN and rows 0 everywhere
    p[3] = np.nan
    got, rows, _ = check_raw(p, None, 2, "one plane all NaN")
    assert (rows[3] == 0).all() and np.isnan(got[3]).all()


@pytest.mark.parametrize("n_lat,n_lon", [(17, 32), (33, 45)])
def test_spectra_of_a_batch_equal_the_yardstick(n_lat, n_lon):
    """Surface and atmospheric variables through spectra() on a Batch; the history slice [:, -1] is passed as a view."""
    pred, truth = red_noise_batch(n_lat, n_lon, seed=3), red_noise_batch(n_lat, n_lon, seed=4)
    bands = bands_for(3)
    lat = lats(n_lat)
    for tr in (None, truth):
        s = spectra(pred.to(DEV), None if tr is None else tr.to(DEV), bands=bands)
        assert s.power["2t"].device == DEV and s.power["2t"].dtype == torch.float64 and (s.error_power is None) == (tr is None)
        assert s.power["z"].shape == (2, 3, 3, n_lon // 2 + 1) and s.rows["2t"].shape == (2, 3)
        s = s.cpu()
        tp = None if tr is None else {(k, idx): x for k, idx, x in planes_of(tr)}
        for k, idx, x in planes_of(pred):
            y = None if tp is None else tp[(k, idx)]
            want, want_rows = yardstick_spectra(x, y, lat, bands)
            bound = spectra_bound(x, y, lat, bands, want)
            got = [s.power[k][idx].numpy()] + ([] if tp is None else [s.truth_power[k][idx].numpy(), s.error_power[k][idx].numpy()])
            assert s.rows[k][idx].tolist() == want_rows.tolist()
            assert (np.abs(np.stack(got) - want) <= bound).all(), (k, idx)
        if tr is not None:
            assert torch.equal(s.ratio["z"], s.power["z"] / s.truth_power["z"])


def test_repeatable_independent_of_the_other_planes_and_of_alignment():
    n_lat, N = 70, 1440
    p, t = red_noise((7, n_lat, N), seed=5), red_noise((7, n_lat, N), seed=6)
    p[2, 5, 100] = np.nan
    bw = torch.from_numpy(band_weights(lats(n_lat), bands_for(3))).to(DEV)
    pd, td = carve(p), carve(t)
    po, to = carve(p, 1), carve(t, 1)                                # the same values one float (4 bytes) further on
    assert pd.data_ptr() % 16 == 0 and po.data_ptr() % 16 == 4
    for truth, truth_off in ((None, None), (td, to)):
        args = lambda sl=slice(None): ([pd[sl]], None if truth is None else [truth[sl]], bw)  # noqa: E731
        whole, again = lib.spectra_power(*args()), lib.spectra_power(*args())
        single = [lib.spectra_power(*args(slice(k, k + 1))) for k in range(7)]
        shifted = lib.spectra_power([po], None if truth_off is None else [truth_off], bw)
        torch.cuda.synchronize()
        for i in (0, 1):
            a, b, c, d = (x[i].cpu().numpy() for x in (whole, again, shifted, [torch.cat([s[0] for s in single]),
                                                                                 torch.cat([s[1] for s in single])]))
            assert np.array_equal(a, b, equal_nan=True), "two calls differ"
            assert np.array_equal(a, d, equal_nan=True), "a plane alone differs from the plane within seven"
            assert np.array_equal(a, c, equal_nan=True), "pointer alignment changes bits"
        assert whole[1][:, 0].tolist() == [70, 70, 69, 70, 70, 70, 70]


def test_spectra_are_capturable_in_a_hip_graph():
    pred, truth = (b.to(DEV) for b in (red_noise_batch(33, 64, seed=7), red_noise_batch(33, 64, seed=8)))
    other = red_noise_batch(33, 64, seed=9).to(DEV)
    bands = bands_for(2)
    first = spectra(pred, truth, bands=bands).cpu()                    # (the warm call: tables and weights are uploaded)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = spectra(pred, truth, bands=bands)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(s.table.cpu(), first.table) and torch.equal(s.rows_table.cpu(), first.rows_table)
    for grp in ("surf_vars", "atmos_vars"):
        for k, v in getattr(pred, grp).items():
            v.copy_(getattr(other, grp)[k])
    graph.replay()
    torch.cuda.synchronize()
    replayed = s.table.cpu()
    assert not torch.equal(replayed, first.table)
    assert torch.equal(replayed, spectra(pred, truth, bands=bands).table.cpu())


@pytest.mark.parametrize("with_truth", (False, True))
def test_the_workspace_is_as_large_as_what_the_call_touches(with_truth):
    """The C call with exactly aurora_hip_spectra_workspace_bytes, inside a larger buffer whose remainder is a guard."""
    n, n_lat, N, nb = 3, 45, 90, 3
    p, t = carve(red_noise((n, n_lat, N), seed=10)), carve(red_noise((n, n_lat, N), seed=11))
    bw = torch.from_numpy(band_weights(lats(n_lat), bands_for(nb))).to(DEV)
    want = lib.spectra_power([p], [t] if with_truth else None, bw)
    need = lib.spectra_workspace_bytes(n, n_lat, N, nb, with_truth)
    assert need > 0 and need % 8 == 0
    guard = 1 << 16
    buf = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    ptrs = torch.tensor([x[k].data_ptr() for x in (p, t) for k in range(n)], dtype=torch.int64).to(DEV)
    F = 3 if with_truth else 1
    power = torch.empty(n, F, nb, N // 2 + 1, dtype=torch.float64, device=DEV)
    rows = torch.empty(n, nb, dtype=torch.int64, device=DEV)
    tw = lib.spectra_twiddle(N, DEV)
    L = lib.load()
    code = L.aurora_hip_spectra(ptrs.data_ptr(), ptrs.data_ptr() + 8 * n if with_truth else None, n, n_lat, N, nb, bw.data_ptr(),
                                tw.data_ptr(), power.data_ptr(), rows.data_ptr(), buf.data_ptr(), need,
                                torch.cuda.current_stream().cuda_stream)
    assert code == 0, L.aurora_hip_last_error()
    torch.cuda.synchronize()
    assert (buf[need:] == 0xA5).all(), "the call wrote past its workspace"
    assert torch.equal(power, want[0]) and torch.equal(rows, want[1])
    assert L.aurora_hip_spectra(ptrs.data_ptr(), None, n, n_lat, N, nb, bw.data_ptr(), tw.data_ptr(), power.data_ptr(),
                                rows.data_ptr(), buf.data_ptr(), need - 8 if not with_truth else 8, None) == -1


def test_a_rollout_is_tracked_step_by_step_and_read_once():
    case = CASES["small_b2"]
    model = getattr(aurora_amd, case["cls"])(**case["kwargs"])
    model.load_state_dict(helpers.case_state_dict(model, torch.float32), strict=True)
    model = model.to(DEV).eval()
    surf, static, atmos, lat, lon, times = helpers.case_inputs(case, model.config)
    f = lambda d: {k: v.float() for k, v in d.items()}  # noqa: E731
    batch = Batch(f(surf), f(static), f(atmos), Metadata(lat.float(), lon.float(), times, tuple(case["levels"])))
    truth = batch.crop(model.patch_size)
    truth_dev = truth.to(DEV)
    bands = ((-90, 90), (0, 90))
    got, preds = [], []
    with torch.inference_mode():
        for pred in rollout(model, batch.to(DEV), steps=3):
            got.append(spectra(pred, truth_dev, bands=bands))           # nothing is read back in the loop
            preds.append(pred)
    got = [s.cpu() for s in got]
    lat_np = truth.metadata.lat.double().numpy()
    for s, pred in zip(got, preds):
        assert set(s.power) == set(pred.surf_vars) | set(pred.atmos_vars)
        tp = {(k, idx): x for k, idx, x in planes_of(truth)}
        for k, idx, x in planes_of(pred):
            want, want_rows = yardstick_spectra(x, tp[(k, idx)], lat_np, bands)
            bound = spectra_bound(x, tp[(k, idx)], lat_np, bands, want)
            have = np.stack([s.power[k][idx].numpy(), s.truth_power[k][idx].numpy(), s.error_power[k][idx].numpy()])
            assert s.rows[k][idx].tolist() == want_rows.tolist()
            assert np.array_equal(np.isnan(have), np.isnan(want)) and (np.abs(have - want)[~np.isnan(want)] <= bound[~np.isnan(want)]).all()
    assert not torch.equal(got[0].table, got[1].table)


def test_device_path_argument_errors():
    pred, truth = red_noise_batch(17, 32, seed=12), red_noise_batch(17, 32, seed=13)
    with pytest.raises(ValueError, match="cpu.*cuda|cuda.*cpu"):
        spectra(pred.to(DEV), truth)
    with pytest.raises(TypeError, match="float64"):
        spectra(pred.to(DEV).type(torch.float64))
    tr = truth.to(DEV)
    tr.surf_vars["2t"] = tr.surf_vars["2t"].transpose(-1, -2).contiguous().transpose(-1, -2)
    with pytest.raises(ValueError, match="contiguous"):
        spectra(pred.to(DEV), tr)
