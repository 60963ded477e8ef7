"""What the verification wrappers of aurora_amd/engine/lib.py refuse, and in which words: one bad operand per call, the exception
type and the full message, copied from the literals of the wrappers' source.  Every refusal here is raised in Python before any
launch; the file pins the messages while the checks behind them are shared."""
import pytest
import torch

from aurora_amd.engine import lib
from tests.verification_inputs import DEV

pytestmark = pytest.mark.gpu
N_LAT, N_LON = 3, 5
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64


def f(*lead, dtype=F32, n_lat=N_LAT, n_lon=N_LON, device=DEV):
    return torch.zeros(*lead, n_lat, n_lon, dtype=dtype, device=device)


def vec(n, dtype):
    return torch.ones(n, dtype=dtype, device=DEV)


def mat(rows, cols=1, dtype=F32):
    return torch.zeros(rows, cols, dtype=dtype, device=DEV)


def wide():
    """(1, n_lat, n_lon) with every other value of a wider plane: the inner stride is 2."""
    return f(1, n_lon=2 * N_LON)[..., ::2]


def members(M=2, lead=1):
    return [[f(lead)] for _ in range(M)]


def labels(*lead, dtype=I32):
    return f(*(lead or (1,)), dtype=dtype)


def object_out(**kw):
    shapes = {"labels": (1, 1, N_LAT, N_LON), "count": (1, 1), "table": (1, 1, 4, 10), **kw}
    return tuple(torch.zeros(shapes[k], dtype=d, device=DEV) for k, d in (("labels", I32), ("count", I32), ("table", I64)))


def stats_state(**kw):
    return {k: torch.zeros(1, N_LAT * N_LON, dtype=dt, device=DEV) for k, (dt, per_thr) in lib.FIELD_STATS_STATE.items()
            if not per_thr} | kw


def regrid_tables():
    i32, f64 = (lambda *s: torch.zeros(*s, dtype=I32, device=DEV)), (lambda *s: torch.zeros(*s, dtype=F64, device=DEV))
    return (i32(2, 2), i32(2), f64(4), f64(2), i32(2, 2), i32(2), f64(4), f64(2))


W, U, INDEX = (lambda: vec(N_LAT, F64)), (lambda: vec(N_LAT, I64)), (lambda: torch.zeros(1, dtype=I64, device=DEV))
NEAREST = lambda: vec(2 * N_LAT + N_LON, F64)  # noqa: E731
WS = lambda: torch.zeros(1 << 16, dtype=F32, device=DEV)  # noqa: E731

# name -> (the call, the exception, the whole message)
CASES = {
    # ---- a device operand of a given dtype and shape
    "scores_sums row_w fp32": (lambda: lib.scores_sums([f(1)], [f(1)], None, vec(N_LAT, F32)), AssertionError,
                               "scores_sums: row_w must be a contiguous fp64 vector on the device"),
    "ensemble_scores_sums row_w matrix": (lambda: lib.ensemble_scores_sums(members(), [f(1)], mat(N_LAT, 1, F64)), AssertionError,
                                          "ensemble_scores_sums: row_w must be a contiguous fp64 vector on the device"),
    "conditional_sums row_w strided": (lambda: lib.conditional_sums([f(1)], [f(1)], None, None, mat(1), False, vec(2 * N_LAT, F64)[::2]),
                                       AssertionError, "conditional_sums: row_w must be a contiguous fp64 vector on the device"),
    "region_sums row_w on the host": (lambda: lib.region_sums([f(1)], [f(1)], None, vec(N_LAT, torch.uint8), vec(N_LON, torch.uint8), None,
                                                              1, torch.ones(N_LAT, dtype=F64)),
                                      AssertionError, "region_sums: row_w must be a contiguous fp64 vector on the device"),
    "event_rowsums thresholds fp64": (lambda: lib.event_rowsums([f(1)], [f(1)], mat(1, 1, F64), [1]), AssertionError,
                                      "event_rowsums: thresholds must be a contiguous (n_planes, T) fp32 matrix on the device"),
    "conditional_sums edges vector": (lambda: lib.conditional_sums([f(1)], [f(1)], None, None, vec(1, F32), False, W()), AssertionError,
                                      "conditional_sums: edges must be a contiguous (n_planes, E) fp32 matrix on the device"),
    "object_labels thresholds vector": (lambda: lib.object_labels([f(1)], vec(1, F32), U()), AssertionError,
                                        "object_labels: thresholds must be a contiguous (n_planes, T) fp32 matrix on the device"),
    "probability_rows thresholds on the host": (lambda: lib.probability_rows(members(), [f(1)], torch.zeros(1, 1)), AssertionError,
                                                "probability_rows: thresholds must be a contiguous (n_planes, T) fp32 matrix on the device"),
    "field_stats_update thresholds rows": (lambda: lib.field_stats_update([[f(1)]], None, None, mat(2), False, INDEX(), {}), AssertionError,
                                           "field_stats_update: thresholds must be a contiguous (1, T) fp32 matrix on the device"),
    "object_labels unit int32": (lambda: lib.object_labels([f(1)], mat(1), vec(N_LAT, I32)), AssertionError,
                                 "object_labels: unit must be a contiguous (n_lat,) int64 vector on the device of thresholds"),
    "object_pairs unit length": (lambda: lib.object_pairs(labels(), labels(), vec(N_LAT + 1, I64), 4, 4, 4), AssertionError,
                                 "object_pairs: unit must be a contiguous (n_lat,) int64 vector on the device of labels_a"),
    "field_quantile_values unit fp64": (lambda: lib.field_quantile_values([f(1)], [0.5], W()), AssertionError,
                                        "field_quantile_values: unit must be a contiguous (n_lat,) int64 vector on the device of the fields"),
    "nearest_event_maps tables length": (lambda: lib.nearest_event_maps(labels(), vec(N_LAT + N_LON, F64), False), AssertionError,
                                         "nearest_event_maps: tables must be a contiguous (2 n_lat + n_lon,) fp64 vector on the device of labels"),
    "spectra_power band_w vector": (lambda: lib.spectra_power([f(1)], None, W()), AssertionError,
                                    "spectra_power: band_w must be a contiguous (n_bands, n_lat) fp64 matrix on the device"),
    "region_sums row_bits int32": (lambda: lib.region_sums([f(1)], [f(1)], None, vec(N_LAT, I32), vec(N_LON, torch.uint8), None, 1, W()),
                                   AssertionError,
                                   "region_sums: row_bits must be a contiguous uint8 tensor of shape (3,), got torch.int32 (3,)"),
    "diagnostics row_table shape": (lambda: lib.diagnostics(N_LAT, N_LON, u=[f(1)], v=[f(1)], ws=[f(1)], row_table=mat(N_LAT, 3, F64)),
                                    AssertionError, "diagnostics: row_table must be a contiguous fp64 (3, 4) on the device of the fields"),
    "diagnostics level_w matrix": (lambda: lib.diagnostics(N_LAT, N_LON, q=[f(2)], tcwv=[f(1)], level_w=mat(2, 1, F64)), AssertionError,
                                   "diagnostics: level_w must be a contiguous fp64 vector on the device of the fields"),
    "object_pairs labels_a int64": (lambda: lib.object_pairs(labels(dtype=I64), labels(), U(), 4, 4, 4), AssertionError,
                                    "object_pairs: labels_a must be a contiguous (..., n_lat, n_lon) int32 tensor on the device"),
    "object_pairs labels_b shape": (lambda: lib.object_pairs(labels(), labels(2), U(), 4, 4, 4), AssertionError,
                                    "object_pairs: labels_b must be a contiguous int32 tensor of shape (1, 3, 5) on the device of labels_a"),
    "nearest_event_maps labels on the host": (lambda: lib.nearest_event_maps(f(1, dtype=I32, device="cpu"), NEAREST(), False), AssertionError,
                                              "nearest_event_maps: labels must be a contiguous (..., n_lat, n_lon) int32 tensor on the device"),
    "object_separation_table labels_a fp32": (lambda: lib.object_separation_table(f(1), f(1, dtype=F64), labels(), vec(1, I32), 4),
                                              AssertionError,
                                              "object_separation_table: labels_a must be a contiguous (..., n_lat, n_lon) int32 tensor on the device"),
    "object_separation_table key fp32": (lambda: lib.object_separation_table(labels(), f(1), labels(), vec(1, I32), 4), AssertionError,
                                         "object_separation_table: key must be a contiguous torch.float64 tensor of shape (1, 3, 5) on the "
                                         "device of labels_a"),
    "conservative_regrid table": (lambda: lib.conservative_regrid([f(1)], torch.zeros(1, 2, 2, device=DEV), regrid_tables()[:-1] + (vec(3, F64),),
                                                                  0.5),
                                  AssertionError, "conservative_regrid: a table has the wrong device, dtype or shape"),
    # ---- outputs given by the caller
    "object_labels out labels shape": (lambda: lib.object_labels([f(1)], mat(1), U(), max_objects=4, out=object_out(labels=(1, 1, N_LAT, 4))),
                                       AssertionError,
                                       "object_labels: labels must be a contiguous torch.int32 tensor of shape (1, 1, 3, 5) on the device of "
                                       "thresholds"),
    "object_labels out table rows": (lambda: lib.object_labels([f(1)], mat(1), U(), max_objects=8, out=object_out()), AssertionError,
                                     "object_labels: table must be a contiguous torch.int64 tensor of shape (1, 1, 8, 10) on the device of "
                                     "thresholds"),
    "object_pairs out count dtype": (lambda: lib.object_pairs(labels(), labels(), U(), 4, 4, 4,
                                                              out=(torch.zeros(1, 4, 4, dtype=I64, device=DEV), vec(1, I64))),
                                     AssertionError,
                                     "object_pairs: count must be a contiguous torch.int32 tensor of shape (1,) on the device of labels_a"),
    "nearest_event_maps out key fp32": (lambda: lib.nearest_event_maps(labels(), NEAREST(), False, out=(labels(), f(1))), AssertionError,
                                        "nearest_event_maps: key must be a contiguous torch.float64 tensor of shape (1, 3, 5) on the device of "
                                        "labels"),
    "object_separation_table out hausdorff shape": (lambda: lib.object_separation_table(
        labels(), f(1, dtype=F64), labels(), vec(1, I32), 4, out=(torch.zeros(1, 4, 3, dtype=I64, device=DEV), vec(2, I64))), AssertionError,
        "object_separation_table: hausdorff must be a contiguous int64 tensor of shape (1,) on the device of labels_a"),
    "field_quantile_values out values shape": (lambda: lib.field_quantile_values([f(1)], [0.25, 0.5], out=(mat(1, 3), vec(1, I64), vec(1, I64))),
                                               AssertionError,
                                               "field_quantile_values: values must be a contiguous torch.float32 tensor of shape (1, 2) on the "
                                               "device of the fields"),
    "ensemble_quantiles out shape": (lambda: lib.ensemble_quantiles(members(), None, [0.5], out=f(1, 2)), AssertionError,
                                     "ensemble_quantiles: out must be a contiguous torch.float32 tensor of (1, 1, 3, 5) on the device of the "
                                     "members"),
    "ensemble_quantiles rank_out dtype": (lambda: lib.ensemble_quantiles(members(), [f(1)], [0.5], rank_out=labels()), AssertionError,
                                          "ensemble_quantiles: rank_out must be a contiguous torch.int8 tensor of (1, 3, 5) on the device of "
                                          "the members"),
    "field_stats_update state dtype": (lambda: lib.field_stats_update([[f(1)]], None, None, None, False, INDEX(),
                                                                      stats_state(n=mat(1, N_LAT * N_LON, I64))), AssertionError,
                                       "field_stats_update: state 'n' must be contiguous torch.int32 of (1, 15) on the device"),
    # ---- a workspace given by the caller
    "object_labels workspace fp32": (lambda: lib.object_labels([f(1)], mat(1), U(), workspace=WS()), AssertionError,
                                     "object_labels: the workspace must be a contiguous uint8 tensor on the device of thresholds"),
    "object_pairs workspace fp32": (lambda: lib.object_pairs(labels(), labels(), U(), 4, 4, 4, workspace=WS()), AssertionError,
                                    "object_pairs: the workspace must be a contiguous uint8 tensor on the device of labels_a"),
    "nearest_event_maps workspace fp32": (lambda: lib.nearest_event_maps(labels(), NEAREST(), False, workspace=WS()), AssertionError,
                                          "nearest_event_maps: the workspace must be a contiguous uint8 tensor on the device of labels"),
    "field_quantile_values workspace fp32": (lambda: lib.field_quantile_values([f(1)], [0.5], workspace=WS()), AssertionError,
                                             "field_quantile_values: the workspace must be a contiguous uint8 tensor on the device of the "
                                             "fields"),
    # ---- the lists of planes
    "scores_sums list lengths": (lambda: lib.scores_sums([f(1), f(1)], [f(1)], None, W()), AssertionError,
                                 "scores_sums: the lists differ in length"),
    "region_sums list lengths": (lambda: lib.region_sums([f(1)], [f(1)], [], vec(N_LAT, torch.uint8), vec(N_LON, torch.uint8), None, 1, W()),
                                 AssertionError, "region_sums: the lists differ in length"),
    "scores_sums shapes": (lambda: lib.scores_sums([f(1)], [f(2)], None, W()), AssertionError,
                           "scores_sums: shapes differ ((2, 3, 5) against (1, 3, 5))"),
    "ensemble_scores_sums shapes": (lambda: lib.ensemble_scores_sums(members(lead=2), [f(1)], W()), AssertionError,
                                    "ensemble_scores_sums: shapes differ ((2, 3, 5) against (1, 3, 5))"),
    "conditional_sums centre shapes": (lambda: lib.conditional_sums([f(1)], [f(1)], [f(1, 1)], None, mat(1), False, W()), AssertionError,
                                       "conditional_sums: shapes differ ((1, 1, 3, 5) against (1, 3, 5))"),
    "scores_sums strided planes": (lambda: lib.scores_sums([wide()], [wide()], None, W()), AssertionError,
                                   "scores_sums: the planes of a prediction field are not row-major contiguous (strides (30, 10, 2))"),
    "spectra_power strided truth": (lambda: lib.spectra_power([f(1)], [wide()], mat(1, N_LAT, F64)), AssertionError,
                                    "spectra_power: the planes of a truth field are not row-major contiguous (strides (30, 10, 2))"),
    "scores_sums truth on the host": (lambda: lib.scores_sums([f(1)], [f(1, device="cpu")], None, W()), AssertionError,
                                      "scores_sums: every tensor must be on the device of row_w"),
    "ensemble_quantiles member on the host": (lambda: lib.ensemble_quantiles([[f(1)], [f(1, device="cpu")]], None, [0.5]), AssertionError,
                                              "ensemble_quantiles: every tensor must be on the device of the first member"),
    "field_stats_update sample on the host": (lambda: lib.field_stats_update([[f(1, device="cpu")]], None, None, None, False, INDEX(), {}),
                                              AssertionError, "field_stats_update: every tensor must be on the device of sample_index"),
    "scores_sums climatology fp64": (lambda: lib.scores_sums([f(1)], [f(1)], [f(1, dtype=F64)], W()), AssertionError,
                                     "scores_sums: climatology fields must be fp32, got torch.float64"),
    "probability_rows member fp64": (lambda: lib.probability_rows([[f(1)], [f(1, dtype=F64)]], [f(1)], mat(1)), AssertionError,
                                     "probability_rows: member 1 fields must be fp32, got torch.float64"),
    "scores_sums rows": (lambda: lib.scores_sums([f(1, n_lat=4)], [f(1, n_lat=4)], None, W()), AssertionError,
                         "scores_sums: a prediction field is (1, 4, 5), not (..., 3, 5)"),
    "event_rowsums thresholds count": (lambda: lib.event_rowsums([f(1)], [f(1)], mat(2), [1]), AssertionError,
                                       "event_rowsums: 1 planes but thresholds for 2"),
    "conditional_sums edges count": (lambda: lib.conditional_sums([f(1)], [f(1)], None, None, mat(2), False, W()), AssertionError,
                                     "conditional_sums: 1 planes but edges for 2"),
    "object_labels thresholds count": (lambda: lib.object_labels([f(2)], mat(1), U()), AssertionError,
                                       "object_labels: 2 planes but thresholds for 1"),
    "probability_rows thresholds count": (lambda: lib.probability_rows(members(), [f(1)], mat(3)), AssertionError,
                                          "probability_rows: 1 planes but thresholds for 3"),
    "field_stats_update second number": (lambda: lib.field_stats_update([[f(1)]], None, [[f(1)], [f(1)]], None, False, INDEX(), {}),
                                         AssertionError, "field_stats_update: the second operands differ from the samples in number"),
    "field_stats_update second shape": (lambda: lib.field_stats_update([[f(1)]], None, [[f(2)]], None, False, INDEX(), {}), AssertionError,
                                        "field_stats_update: a second operand differs from its sample"),
    "field_stats_update second strided": (lambda: lib.field_stats_update([[f(1)]], None, [[wide()]], None, False, INDEX(), {}), AssertionError,
                                          "field_stats_update: the planes of a second operand field are not row-major contiguous (strides "
                                          "(30, 10, 2))"),
    "diagnostics plane counts": (lambda: lib.diagnostics(N_LAT, N_LON, u=[f(1)], v=[f(2)], ws=[f(1)]), AssertionError,
                                 "diagnostics: v holds 2 planes, u 1"),
    "diagnostics entries": (lambda: lib.diagnostics(N_LAT, N_LON, u=[f(1)], v=[f(1)], ws=[None, f(1)]), AssertionError,
                            "diagnostics: ws with None entries must have an entry per u entry"),
    "diagnostics columns": (lambda: lib.diagnostics(N_LAT, N_LON, q=[f(2)], tcwv=[f(2)], level_w=vec(2, F64)), AssertionError,
                            "diagnostics: tcwv holds 2 planes for 1 columns"),
    "conservative_regrid plane count": (lambda: lib.conservative_regrid([f(2)], torch.zeros(1, 2, 2, device=DEV), regrid_tables(), 0.5),
                                        AssertionError, "conservative_regrid: the sources hold 2 planes, out 1"),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_refusal(name):
    call, kind, message = CASES[name]
    with pytest.raises(kind) as caught:
        call()
    assert type(caught.value) is kind and str(caught.value) == message
