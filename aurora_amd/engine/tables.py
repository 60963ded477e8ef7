"""The cache of small device tables: latitude weights and thresholds (aurora_amd/_fields.py), plane-pointer arrays and
spectra twiddles (aurora_amd/engine/lib.py).  tests/test_verification_messages.py::test_device_table_cache pins its policy."""

from __future__ import annotations

import threading
from collections import OrderedDict
from typing import Callable

import numpy as np
import torch


def _upload(a: np.ndarray, device: torch.device) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(device, non_blocking=True)


def _capturing() -> bool:
    return torch.cuda.is_current_stream_capturing()   # (looked up at every call: the tests of a cold call patch it)


class DeviceTables:
    """Device copies of small host tables, kept per content (a roll-out asks for the same weights and thresholds at every
    step).  A captured graph holds a table's raw address, so a table that was used during stream capture is never evicted;
    the others leave least recently used first once more than `limit` are kept.  A miss uploads from pinned memory without
    synchronising; during capture a miss is an error with the caller's message."""

    def __init__(self, limit: int = 64, upload: Callable = _upload, capturing: Callable[[], bool] = _capturing):
        self.limit, self._upload, self._capturing = limit, upload, capturing
        self._tables: "OrderedDict[tuple, list]" = OrderedDict()   # key -> [device copy, used in a captured graph]
        self._lock = threading.Lock()

    def get(self, key: tuple, device, make: Callable[[], np.ndarray], on_capture: str):
        key = (*key, str(device))
        capturing = self._capturing()
        with self._lock:
            hit = self._tables.get(key)
            if hit is not None:
                self._tables.move_to_end(key)
                hit[1] = hit[1] or capturing
                return hit[0]
        if capturing:
            raise RuntimeError(on_capture)
        table = self._upload(make(), device)
        with self._lock:
            self._tables[key] = [table, False]
            free = [k for k, v in self._tables.items() if not v[1]]
            for old in free[: max(0, len(free) - self.limit)]:
                del self._tables[old]
        return table
