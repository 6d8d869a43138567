"""CPU-only checks of the boundary of the data shifts: the library exports altro_hip_set_dynamics_range / _get_dynamics_knot /
_shift_dynamics / _shift_linear_costs, the binding has their methods, and without a device nothing computes -- a handle cannot be had
(ALTRO_HIP_ERR_NO_DEVICE, like every call around them) and the entry points refuse a null one without touching anything."""
import ctypes as C

import pytest

import altro_amd

SYMBOLS = ["altro_hip_set_dynamics_range", "altro_hip_get_dynamics_knot", "altro_hip_shift_dynamics", "altro_hip_shift_linear_costs"]
METHODS = ["set_dynamics_range", "get_dynamics_knot", "shift_dynamics", "shift_linear_costs"]
ERR_NO_DEVICE, ERR_BAD_ARGUMENT = -1, -2


def test_symbols_are_exported_and_listed():
    L = altro_amd.lib()
    for s in SYMBOLS:
        assert hasattr(L, s), s
        assert s in altro_amd.C_ABI_SYMBOLS, s
        assert getattr(L, s).argtypes is not None, s       # declared in lib(): a pointer is never passed as a C int


def test_methods_exist():
    for m in METHODS:
        assert callable(getattr(altro_amd.Batch, m, None)), m


def test_no_device_no_data():
    L = altro_amd.lib()
    null = C.c_void_p()
    # a null handle is refused by every one of them, device or not, and the message says so
    calls = [lambda: L.altro_hip_set_dynamics_range(null, None, None, None, 0, 0, 0), lambda: L.altro_hip_get_dynamics_knot(null, 0, None, None, None),
             lambda: L.altro_hip_shift_dynamics(null), lambda: L.altro_hip_shift_linear_costs(null)]
    for call in calls:
        assert call() == ERR_BAD_ARGUMENT
        assert b"null handle" in L.altro_hip_last_error()
    if L.altro_hip_device_count() > 0:
        return                                               # (with a device: tests/test_gpu_shift_data.py)
    h = C.c_void_p()
    assert L.altro_hip_batch_create(C.byref(h), 10, 12, 4, 2, altro_amd.F64, altro_amd.PLAN_AUTO, 0, 0, None) == ERR_NO_DEVICE
    assert not h.value
    with pytest.raises(altro_amd.AltroHipError, match="error -1"):
        altro_amd.Batch(10, 12, 4, 2)
