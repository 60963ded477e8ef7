"""`aurora_amd.field_quantiles` on the CPU against yardsticks written here (THE RULE: aurora_amd/field_quantiles.py):
kind="count" against `np.quantile(valid.astype(float64), q)` -- within one fp32 unit in the last place, and exactly where g = 0,
the statement tests/test_ensemble_quantiles_host.py makes for the same expression -- and kind="area" against a plain-Python
evaluation: sort by (K, index), add the Python-int units until they reach the target; that comparison is exact.
tests/test_gpu_field_quantiles.py compares the kernel with the CPU path on the planes made here."""
import ctypes
import importlib
import struct
from datetime import datetime

import numpy as np
import pytest
import torch

import aurora_amd
from aurora_amd import Batch, Metadata, _fields, conditional_scores, event_scores, field_quantiles
from aurora_amd.batch import BandBatch
from aurora_amd.objects import area_units
from tests.verification_inputs import red_noise, red_noise_batch

mod = importlib.import_module("aurora_amd.field_quantiles")       # (the package's attribute of this name is the function)

Q3 = (0.5, 0.9, 0.99)
Q8 = (0.99, 0.0, 0.5, 0.5, 1.0, 0.25, 0.001, 0.75)               # unsorted, repeated, both ends


def lat_of(H, descending=True):
    lat = np.linspace(90, -90, H) if H > 1 else np.zeros(1)
    return lat if descending else lat[::-1].copy()


def batch_of(planes, atmos=None, lat=None) -> Batch:
    """planes: (B, H, W) values of the surface variable "x"; atmos: (B, C, H, W) of the atmospheric variable "a"."""
    planes = np.asarray(planes)
    B, H, W = planes.shape
    md = Metadata(lat=torch.as_tensor(lat_of(H) if lat is None else lat, dtype=torch.float64),
                  lon=torch.linspace(0, 360, W + 1, dtype=torch.float64)[:-1], time=tuple(datetime(2023, 1, 1, 6) for _ in range(B)),
                  atmos_levels=tuple(range(100, 100 + (0 if atmos is None else np.asarray(atmos).shape[1]))))
    a = {} if atmos is None else {"a": torch.as_tensor(np.asarray(atmos))[:, None]}
    return Batch({"x": torch.as_tensor(planes)[:, None]}, {}, a, md)


# ---- the yardsticks ----------------------------------------------------------------------------------------------------------
def key_of(v) -> int:
    u = struct.unpack("<I", struct.pack("<f", v))[0]
    return (~u & 0xffffffff) if u & 0x80000000 else (u | 0x80000000)


def area_yardstick(plane, q, unit):
    """(values, valid, W) of one plane in plain Python: the inverted CDF over Python-int units."""
    v = np.asarray(plane, dtype=np.float32)
    pts = sorted((key_of(float(v[i, j])), i * v.shape[1] + j, float(v[i, j]), int(unit[i]))
                 for i in range(v.shape[0]) for j in range(v.shape[1]) if np.isfinite(v[i, j]))
    W = sum(p[3] for p in pts)
    out = []
    for qi in q:
        if W == 0:
            out.append(np.float32("nan"))
            continue
        target = min(max(int(np.ceil(float(qi) * float(W))), 1), W)
        cum = 0
        for _, _, x, u in pts:
            cum += u
            if cum >= target:
                out.append(np.float32(x))
                break
    return np.array(out, dtype=np.float32), len(pts), W


def ulp(x: np.ndarray) -> np.ndarray:
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def check_count(plane, q):
    got, n, total = mod.plane_quantiles(plane, q, None)
    v = np.asarray(plane, dtype=np.float32)
    x = v[np.isfinite(v)].astype(np.float64)
    assert n == total == x.size and got.dtype == np.float32
    if n == 0:
        assert np.isnan(got).all()
        return
    want = np.quantile(x, q)
    assert np.all(np.abs(got.astype(np.float64) - want) <= np.maximum(ulp(got), ulp(want))), (got, want)
    s = np.sort(x)
    for i, qi in enumerate(q):
        h = (n - 1) * qi
        if h == np.floor(h):                                     # g = 0: the order statistic itself
            assert got[i] == np.float32(s[int(h)])


def check_area(plane, q, lat=None, unit=None):
    unit = area_units(lat_of(np.shape(plane)[0]) if lat is None else lat) if unit is None else unit
    got, n, W = mod.plane_quantiles(plane, q, unit)
    want, n_want, W_want = area_yardstick(plane, q, unit)
    assert (n, W) == (n_want, W_want) and got.dtype == np.float32
    assert got.tobytes() == want.tobytes(), (got, want)
    return got


def cases() -> dict:
    """name -> float32 plane: what this file and the GPU file take the quantiles of."""
    g = np.random.default_rng(5)
    special = g.standard_normal((7, 9)).astype(np.float32)
    special[0, 3], special[2, 0], special[5, 5], special[6, 7], special[3, 3] = np.nan, np.inf, -np.inf, np.nan, np.inf
    zeros = np.zeros((4, 6), dtype=np.float32)
    zeros[::2] = -0.0
    denormal = (g.integers(-40, 40, (5, 8)) * np.float64(1.4e-45)).astype(np.float32)    # multiples of the smallest denormal
    signs = np.concatenate([-np.geomspace(1e-30, 1e30, 20), np.geomspace(1e-30, 1e30, 20)]).astype(np.float32).reshape(5, 8)
    ties = np.full((6, 10), 2.0, dtype=np.float32)                # a plateau across every target between two other values
    ties[0, :5], ties[5, 5:] = 1.0, 3.0
    halves = np.ones((4, 16), dtype=np.float32)                   # j and hi of q = 0.5 land in different top-byte bins
    halves[:, ::2] = -1.0
    one = np.full((3, 5), np.nan, dtype=np.float32)
    one[1, 2] = -7.25
    two = one.copy()
    two[2, 4] = 1e-3
    return {"noise": red_noise((9, 12), seed=3), "special": special, "zeros": zeros, "denormal": denormal, "signs": signs,
            "ties": ties, "halves": halves, "constant": np.full((5, 7), 273.15, dtype=np.float32),
            "all_nan": np.full((3, 4), np.nan, dtype=np.float32), "one": one, "two": two,
            "one_point": np.array([[4.5]], dtype=np.float32), "white": g.standard_normal((8, 11)).astype(np.float32)}


# ---- the rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases()))
def test_count_is_numpy_linear_over_the_valid_points(name):
    for q in (Q3, Q8, (0.5,), (0.0, 1.0)):
        check_count(cases()[name], q)


@pytest.mark.parametrize("name", sorted(cases()))
def test_area_is_the_inverted_cdf_over_integer_units(name):
    plane = cases()[name]
    for q in (Q3, Q8, (0.5,), (0.0, 1.0)):
        check_area(plane, q)
        check_area(plane, q, lat=lat_of(plane.shape[0], descending=False))


def test_the_smallest_counts():
    for n, want in ((0, [np.nan] * 3), (1, [4.0] * 3), (2, [4.0, 5.0, 6.0])):
        plane = np.full((2, 3), np.nan, dtype=np.float32)
        plane.reshape(-1)[1:1 + n] = [4.0, 6.0][:n]
        got, valid, total = mod.plane_quantiles(plane, (0.0, 0.5, 1.0), None)
        assert valid == total == n and np.array_equal(got, np.array(want, dtype=np.float32), equal_nan=True)
        check_area(plane, (0.0, 0.5, 1.0), lat=np.array([10.0, -10.0]))


def test_signed_zeros_order_and_keep_their_sign():
    plane = np.array([[0.0, -0.0, 0.0, -0.0]], dtype=np.float32)
    got = check_area(plane, (0.0, 0.5, 0.51, 1.0))
    assert np.signbit(got).tolist() == [True, True, False, False]            # -0 sorts below +0
    check_count(plane, (0.0, 0.5, 1.0))


def test_q_ends_are_the_extremes_and_order_of_q_does_not_matter():
    plane = cases()["white"]
    for unit in (None, area_units(np.linspace(70, -70, 8))):                   # (no pole row: every point has area)
        got = mod.plane_quantiles(plane, Q8, unit)[0]
        assert got[1] == plane.min() and got[4] == plane.max() and got[2] == got[3]
        again = mod.plane_quantiles(plane, sorted(Q8), unit)[0]
        assert sorted(got.tolist()) == again.tolist()


def test_pole_rows_carry_no_area():
    lat = lat_of(5)
    unit = area_units(lat)
    assert unit[0] == unit[4] == 0 and unit[1:4].min() > 0
    plane = np.arange(20, dtype=np.float32).reshape(5, 4)                    # the poles hold the extremes
    got = check_area(plane, (0.0, 1.0), lat=lat)
    assert got.tolist() == [4.0, 15.0]                                       # ... which the area ignores
    assert mod.plane_quantiles(plane, (0.0, 1.0), None)[0].tolist() == [0.0, 19.0]
    # all valid points on pole rows: W = 0, NaN, while `valid` counts them
    only_poles = plane.copy()
    only_poles[1:4] = np.nan
    fq = field_quantiles(batch_of(only_poles[None], lat=lat), (0.5,))
    assert torch.isnan(fq.value["x"]).all() and fq.valid["x"].tolist() == [8] and fq.total["x"].tolist() == [0]
    assert field_quantiles(batch_of(only_poles[None], lat=lat), (0.5,), kind="count").value["x"].tolist() == [[9.5]]


def test_a_single_row_on_a_pole():
    """THE RULE with the unit of a pole row, 0: W = 0 gives NaN.  (Through the front end a lone row has the mean weight, 1, so
    its unit is 2^32 wherever it lies: `area_units` normalises by the mean of the rows at hand.)"""
    row = np.array([[1.0, 2.0, 3.0]], dtype=np.float32)
    got, valid, W = mod.plane_quantiles(row, (0.5,), np.zeros(1, dtype=np.int64))
    assert np.isnan(got).all() and valid == 3 and W == 0
    check_area(row, (0.5,), unit=np.zeros(1, dtype=np.int64))
    fq = field_quantiles(batch_of(row[None], lat=np.array([90.0])), (0.5,))
    assert fq.value["x"].tolist() == [[2.0]] and fq.total["x"].tolist() == [3 * 2 ** 32]


def test_the_front_end_lays_out_batches_and_levels():
    b = red_noise_batch(9, 12, seed=4, B=2)
    lat = _fields._host(b.metadata.lat)
    for kind, unit in (("area", area_units(lat)), ("count", None)):
        fq = field_quantiles(b, Q3, kind=kind)
        assert fq.q == Q3 and fq.kind == kind and fq.cpu().value.keys() == fq.value.keys() == {"2t", "msl", "z"}
        assert fq.value["2t"].shape == (2, 3) and fq.value["z"].shape == (2, 3, 3) and fq.value["z"].dtype == torch.float32
        assert fq.valid["z"].shape == (2, 3) and fq.valid["z"].dtype == fq.total["2t"].dtype == torch.int64
        for name, f in (("2t", b.surf_vars["2t"]), ("z", b.atmos_vars["z"])):
            last = f[:, -1].numpy()
            for idx in np.ndindex(*last.shape[:-2]):
                want, n, total = mod.plane_quantiles(last[idx], Q3, unit)
                assert fq.value[name][idx].numpy().tobytes() == want.tobytes()
                assert (int(fq.valid[name][idx]), int(fq.total[name][idx])) == (n, total) and n == 9 * 12
    only = field_quantiles(b, 0.5, only=("z",))
    assert only.value.keys() == {"z"} and only.value["z"].shape == (2, 3, 1) and only.q == (0.5,)
    assert field_quantiles(b, 0.5, only="msl").value.keys() == {"msl"}
    half = field_quantiles(Batch({k: v.double() for k, v in b.surf_vars.items()}, {}, {}, b.metadata), Q3)   # rounded to float32 first
    assert torch.equal(half.value["2t"], field_quantiles(b, Q3).value["2t"])


def test_thresholds_are_what_the_event_modules_take():
    b = red_noise_batch(9, 12, seed=6, B=2)
    other = red_noise_batch(9, 12, seed=7, B=2)
    fq = field_quantiles(b, (0.9, 0.5, 0.9, 0.99))
    thr = fq.thresholds()
    assert thr.keys() == {"2t", "msl", "z"} and thr["2t"].shape == (3,) and thr["z"].shape == (3, 3)
    for name, t in thr.items():
        assert t.dtype == np.float32 and np.all(np.diff(t, axis=-1) > 0)
        levels = 3 if name == "z" else None
        assert np.array_equal(_fields.threshold_rows("event_scores", name, t, levels), t.reshape(-1, 3))
        assert np.array_equal(t, np.unique(fq.value[name][0].numpy(), axis=-1) if name != "z" else
                              np.stack([np.unique(r) for r in fq.value[name][0].numpy()]))
    assert fq.thresholds(1)["2t"].tolist() != thr["2t"].tolist()
    assert event_scores(other, b, thr).hits["2t"].shape == (2, 3) and event_scores(other, b, thr).hits["z"].shape == (2, 3, 3)
    assert conditional_scores(other, b, thr) is not None
    # a plane without a value, and rows that lose different numbers of duplicates, are padded with NaN
    planes = np.stack([cases()["all_nan"], cases()["constant"][:3, :4]])
    levels = np.stack([cases()["constant"][:3, :4], cases()["white"][:3, :4]])[None].repeat(2, axis=0)
    t = field_quantiles(batch_of(planes, atmos=levels), (0.1, 0.9)).thresholds()
    assert np.isnan(t["x"]).all() and t["x"].shape == (1,) and t["a"].shape == (2, 2) and np.isnan(t["a"][0, 1])
    assert not np.isnan(t["a"][1]).any() and _fields.threshold_rows("objects", "a", t["a"], 2).shape == (2, 2)
    with pytest.raises(IndexError, match="field_quantiles: thresholds of batch element 2"):
        fq.thresholds(2)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refused_inputs_say_why():
    b = batch_of(cases()["white"][None])
    with pytest.raises(TypeError, match="field_quantiles: batch must be a Batch"):
        field_quantiles({"x": 1})
    with pytest.raises(ValueError, match="field_quantiles: q must be numbers"):
        field_quantiles(b, ("a",))
    with pytest.raises(ValueError, match="field_quantiles: 1 to 8 values of q, got 9"):
        field_quantiles(b, [0.5] * 9)
    with pytest.raises(ValueError, match="field_quantiles: 1 to 8 values of q, got 0"):
        field_quantiles(b, [])
    for bad in ((1.5,), (-0.1,), (float("nan"),)):
        with pytest.raises(ValueError, match=r"field_quantiles: q must be finite values in \[0, 1\]"):
            field_quantiles(b, bad)
    with pytest.raises(ValueError, match="field_quantiles: kind must be one of"):
        field_quantiles(b, kind="points")
    with pytest.raises(ValueError, match="field_quantiles: only names the variable 'y', which batch does not hold"):
        field_quantiles(b, only=("y",))
    with pytest.raises(ValueError, match="field_quantiles: batch has no surface or atmospheric variable"):
        field_quantiles(Batch({}, {}, {}, b.metadata))
    matrix = Batch(b.surf_vars, {}, {}, Metadata(lat=b.metadata.lat[:, None].expand(8, 11), lon=b.metadata.lon[None].expand(8, 11),
                                                 time=b.metadata.time, atmos_levels=()))
    with pytest.raises(ValueError, match="field_quantiles: batch has matrices for latitudes / longitudes"):
        field_quantiles(matrix)
    band = BandBatch.__new__(BandBatch)
    with pytest.raises(ValueError, match=r"field_quantiles: batch is a latitude band \(BandBatch\); gather the forecast first, band "
                                         "quantiles are not supported"):
        field_quantiles(band)
    wrong = Batch({"x": torch.zeros(1, 1, 8, 10)}, {}, {}, b.metadata)
    with pytest.raises(ValueError, match=r"field_quantiles: batch.surf_vars\['x'\] has shape \(1, 1, 8, 10\), which does not fit"):
        field_quantiles(wrong)
    # what the device path asks of its fields, worded as by the other front ends
    with pytest.raises(TypeError, match=r"field_quantiles: batch variable 'x' is torch.float64; the device path takes float32 fields "
                                        r"\(move the batches to the CPU for other precisions\)"):
        _fields.check_planes("field_quantiles", [("batch", ["x"], [torch.zeros(1, 8, 11, dtype=torch.float64)])], 8, 11, _fields.TAKES_TASK)
    meta = [torch.zeros(1, 8, 11, device="meta"), torch.zeros(1, 8, 11)]
    with pytest.raises(ValueError, match="field_quantiles: the fields are on .*; move the batches to the CPU or to one GPU first"):
        _fields.place("field_quantiles", [("batch", ["x", "y"], meta)], 8, 11, _fields.TAKES_TASK)


def test_the_c_entry_point_refuses_before_any_launch():
    from aurora_amd.engine import lib

    raw, header = lib.load(), (lib.library_path().parents[2] / "include" / "aurora_hip.h").read_text()
    for name in ("aurora_hip_field_quantiles", "aurora_hip_field_quantiles_workspace_bytes"):
        assert hasattr(raw, name) and name in lib.EXPORTED_SYMBOLS and f"{name}(" in header
    assert "field_quantiles.hip" in __import__("aurora_amd.build", fromlist=["SOURCES"]).SOURCES
    assert aurora_amd.field_quantiles is mod.field_quantiles and {"field_quantiles", "FieldQuantiles"} <= set(aurora_amd.__all__)
    err = lambda: raw.aurora_hip_last_error()  # noqa: E731
    need = raw.aurora_hip_field_quantiles_workspace_bytes(69, 3)
    assert 69 * (2 + 6 * 3) * 256 * 8 <= need <= 69 * ((2 + 6 * 3) * 256 * 8 + 512)     # histograms only: never plane-sized
    assert raw.aurora_hip_field_quantiles_workspace_bytes(0, 3) == 0 and raw.aurora_hip_field_quantiles_workspace_bytes(1, 9) == 0
    q = (ctypes.c_double * 8)(0.5, 0.9, 0.99, 0.0, 1.0, 0.5, 0.25, 0.75)
    args = lambda **kw: tuple({**dict(planes=16, n_planes=69, n_lat=9, n_lon=12, unit=16, q=ctypes.addressof(q), n_q=3, values=16,  # noqa: E731
                                     valid=16, total=16, ws=16, ws_size=need, stream=None), **kw}.values())
    bad_q = (ctypes.c_double * 2)(0.5, 1.25)
    for kw, text in ((dict(ws_size=need - 8), b"workspace"), (dict(n_q=0), b"n_q"), (dict(n_q=9), b"n_q"), (dict(q=None), b"null q"),
                     (dict(q=ctypes.addressof(bad_q), n_q=2), b"q[1] = 1.25 is not in [0, 1]"), (dict(n_lat=0), b"bad sizes"),
                     (dict(n_planes=-1), b"bad sizes"), (dict(n_lat=600000, n_lon=4096), b"2^30"),
                     (dict(n_lat=600000, n_lon=4096, unit=None), b"2^31 - 2"), (dict(values=None), b"null"), (dict(total=None), b"null"),
                     (dict(ws=20), b"aligned"), (dict(unit=20), b"aligned"), (dict(values=18), b"aligned")):
        assert raw.aurora_hip_field_quantiles(*args(**kw)) == -1 and text in err(), (kw, err())
    assert raw.aurora_hip_field_quantiles(*args(n_planes=0, planes=None, values=None, ws=None, ws_size=0)) == 0   # a no-op
