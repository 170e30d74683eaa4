"""A stand-in for struct tarl_plan in the host-side argument tests: the entry points read N (and E) before any device
array, so the leading fields are enough to reach every check that runs before a HIP call."""
import ctypes


class FakePlan(ctypes.Structure):
    """Leading fields of struct tarl_plan (csrc/tarl_common.h): enough for the host-side checks, no device arrays."""
    _fields_ = [("N", ctypes.c_int64), ("E", ctypes.c_int64), ("G", ctypes.c_int64)] + \
               [(f"pad{i}", ctypes.c_int64) for i in range(32)]


def fake_plan(N, E):
    p = FakePlan()
    p.N, p.E = N, E
    return p
