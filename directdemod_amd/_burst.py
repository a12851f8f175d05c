"""
What the burst decoders' device wrappers share (adsb, ais, pocsag, acars, rs41, rds; sstv for the laps; device side:
dd_candidates.h): the type check of a device array, the candidate list asked for again at the true count when its capacity proved
too small, and the seconds per stage of a decode.
"""
import ctypes as C
import time

import numpy as np

from . import _hip
from ._hip import DevArray, check


def need(a, dtype, what):
    if not isinstance(a, DevArray) or a.dtype != dtype:
        raise TypeError("%s: a %s device array expected" % (what, dtype))


def candidates(entry, cap, call):
    """(the survivors as a device int64 array, how many) of the C entry named `entry`: call(list pointer, cap, count reference)
    makes the C call and returns its code; a list that proves too small is asked for again at the true count"""
    cap = int(cap)
    count = C.c_int64(0)
    while True:
        lst = DevArray(max(cap, 1), np.int64)
        rc = call(lst.ptr, cap, C.byref(count))
        if rc == _hip.DD_ERR_INVALID and count.value > cap:
            cap = count.value
            continue
        check(rc, entry)
        return lst, int(count.value)


def masks(entry, n, call):
    """uint8[n] on the host, the mask byte of every sample by the diagnostic C entry named `entry`: call(mask pointer) makes the C
    call and returns its code"""
    mask = DevArray(max(n, 1), np.uint8)
    check(call(mask.ptr), entry)
    return mask.to_host()[:n]


class Laps:
    """Seconds per stage: lap(name) synchronises the device and adds the time since the last lap, or since the object was made, to
    laps[name].  laps None: lap does nothing and touches no device, which is how the NumPy stages run."""

    def __init__(self, laps=None):
        self.laps = laps
        self._mark = time.perf_counter()

    def lap(self, name):
        if self.laps is not None:
            _hip.sync()
            now = time.perf_counter()
            self.laps[name] = self.laps.get(name, 0.0) + now - self._mark
            self._mark = now

    def finish(self, *names):
        """the laps, with 0.0 for every stage of `names` that never ran"""
        for name in names:
            self.laps.setdefault(name, 0.0)
        return self.laps
