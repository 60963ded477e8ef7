"""The host side of the verification binding (aurora_amd/engine/lib.py) without a device: where the pointer array of every list
of a call sits in the uploaded table, the one cache class behind the plane tables and the twiddles, and the refusals that come
before any device call.  CPU tensors have addresses too; the upload is injected as in `test_device_table_cache`."""
import numpy as np
import pytest
import torch

from aurora_amd import _fields
from aurora_amd.engine import lib, tables

N_LAT, N_LON = 3, 5
CPU = torch.device("cpu")
BASE = 0x7F0000001000


class Uploaded:
    def __init__(self, a, device):
        self.a, self.device = a, device

    def data_ptr(self):
        return BASE


@pytest.fixture
def uploads(monkeypatch):
    made = []

    def upload(a, device):
        made.append(Uploaded(a, device))
        return made[-1]

    monkeypatch.setattr(lib, "_plane_tables", tables.DeviceTables(upload=upload, capturing=lambda: False))
    return made


def test_table_layout(uploads):
    history = torch.zeros(2, 4, N_LAT, N_LON)[:, -1]                        # a sliced history view: leading stride 4 planes
    repeated = torch.zeros(1, N_LAT, N_LON).expand(3, N_LAT, N_LON)         # a stride-0 view: one plane three times
    first, last = [history, repeated], [torch.zeros(2, N_LAT, N_LON), torch.zeros(3, N_LAT, N_LON)]
    planes = lib._planes("layout", [("first", first), ("absent", None), ("last", last)], CPU, "the anchor", N_LAT, N_LON)
    want = lib._plane_addresses("layout", first, N_LAT, N_LON, "first") + lib._plane_addresses("layout", last, N_LAT, N_LON, "last")
    plane = 4 * N_LAT * N_LON
    assert want[:5] == [history.data_ptr(), history.data_ptr() + 4 * plane] + [repeated.data_ptr()] * 3
    assert want[5:] == [last[0].data_ptr(), last[0].data_ptr() + plane] + [last[1].data_ptr() + i * plane for i in range(3)]
    assert planes.n == 5 and planes.addresses == want
    ready = [0, history.data_ptr(), 0, 0, repeated.data_ptr()]              # ready addresses: 0 where a plane has none
    planes.add("ready", ready)
    planes.add("absent too", None)
    assert not uploads
    at = planes.upload()
    sent, = uploads
    assert sent.device == CPU and sent.a.dtype == np.int64 and sent.a.tolist() == want + ready
    assert at == {"first": BASE, "absent": None, "last": BASE + 8 * 5, "ready": BASE + 8 * 10, "absent too": None}
    again = lib._planes("layout", [("first", first), ("absent", None), ("last", last)], CPU, "the anchor", N_LAT, N_LON)
    again.add("ready", ready)
    again.add("absent too", None)
    assert again.upload() == at and len(uploads) == 1                       # the same addresses: the cached table


def test_like_names_the_list_the_others_are_compared_with(uploads):
    a, b = [torch.zeros(2, N_LAT, N_LON)], [torch.zeros(1, N_LAT, N_LON)]
    with pytest.raises(AssertionError) as e:
        lib._planes("fn", [("member 0", a), ("truth", b)], CPU, "row_w", N_LAT, N_LON, like=-1)
    assert str(e.value) == "fn: shapes differ ((2, 3, 5) against (1, 3, 5))"
    with pytest.raises(AssertionError) as e:
        lib._planes("fn", [("member 0", a), ("absent", None), ("truth", b)], CPU, "row_w", N_LAT, N_LON)
    assert str(e.value) == "fn: shapes differ ((1, 3, 5) against (2, 3, 5))"
    assert lib._planes("fn", [], CPU).n == 0 and lib._planes("fn", [("absent", None)], CPU).addresses == []
    assert not uploads


def test_one_cache_class():
    assert _fields.DeviceTables is tables.DeviceTables and isinstance(_fields.tables, tables.DeviceTables)
    assert type(lib._plane_tables) is tables.DeviceTables and lib._plane_tables.limit == 256
    assert type(lib._twiddles) is tables.DeviceTables and lib._twiddles.limit == 64
    assert not hasattr(lib, "_cached_table")


def f(*lead, dtype=torch.float32):
    return torch.zeros(*lead, N_LAT, N_LON, dtype=dtype)


# name -> (a call with a host operand where a device operand is needed, the whole message): refused before the library is loaded
HOST_OPERANDS = {
    "scores_sums": (lambda: lib.scores_sums([f(1)], [f(1)], None, torch.ones(N_LAT, dtype=torch.float64)),
                    "scores_sums: row_w must be a contiguous fp64 vector on the device"),
    "ensemble_scores_sums": (lambda: lib.ensemble_scores_sums([[f(1)], [f(1)]], [f(1)], torch.ones(N_LAT, dtype=torch.float64)),
                             "ensemble_scores_sums: row_w must be a contiguous fp64 vector on the device"),
    "event_rowsums": (lambda: lib.event_rowsums([f(1)], [f(1)], torch.zeros(1, 1), [1]),
                      "event_rowsums: thresholds must be a contiguous (n_planes, T) fp32 matrix on the device"),
    "object_labels": (lambda: lib.object_labels([f(1)], torch.zeros(1, 1), torch.ones(N_LAT, dtype=torch.int64)),
                      "object_labels: thresholds must be a contiguous (n_planes, T) fp32 matrix on the device"),
    "object_pairs": (lambda: lib.object_pairs(f(1, dtype=torch.int32), f(1, dtype=torch.int32), torch.ones(N_LAT, dtype=torch.int64), 4, 4, 4),
                     "object_pairs: labels_a must be a contiguous (..., n_lat, n_lon) int32 tensor on the device"),
    "nearest_event_maps": (lambda: lib.nearest_event_maps(f(1, dtype=torch.int32), torch.ones(2 * N_LAT + N_LON, dtype=torch.float64), False),
                           "nearest_event_maps: labels must be a contiguous (..., n_lat, n_lon) int32 tensor on the device"),
    "spectra_power": (lambda: lib.spectra_power([f(1)], None, torch.ones(1, N_LAT, dtype=torch.float64)),
                      "spectra_power: band_w must be a contiguous (n_bands, n_lat) fp64 matrix on the device"),
}


@pytest.mark.parametrize("name", sorted(HOST_OPERANDS))
def test_a_host_operand_is_refused_before_any_device_call(name, monkeypatch):
    monkeypatch.setattr(lib, "load", lambda: pytest.fail("the library was asked for"))
    call, message = HOST_OPERANDS[name]
    with pytest.raises(AssertionError) as e:
        call()
    assert str(e.value) == message
