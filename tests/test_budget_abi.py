"""The budgeted correlated update's entry points, as far as they go without a device: the budget's host arithmetic and the argument
errors that are found before any device work."""
import ctypes as C
from pathlib import Path

import numpy as np

CPM_ERR_INVALID_ARGUMENT = -1


def test_update_budget_is_the_references_float_arithmetic(cpm):
    """(int)((percent / 100.f) * (float)n): float32 throughout, n rounded to float first (2^24 + 1 is not representable)."""
    lib = cpm.binding.load_library()
    table = [(n, pct) for n in (1, 2, 3, 100, 25600, 65536, 1048576, (1 << 24) + 1, 1000003)
             for pct in (0.0, 1.0, 5.0, 10.0, 25.0, 33.3, 50.0, 99.9, 100.0)]
    for n, pct in table:
        want = int(np.float32(pct) / np.float32(100) * np.float32(n))
        assert lib.cpm_update_budget(n, pct) == want, (n, pct)
    assert lib.cpm_update_budget(1048576, 0.0) == 0 and lib.cpm_update_budget(1048576, 100.0) == 1048576
    assert lib.cpm_update_budget(1, 99.9) == 0 and lib.cpm_update_budget(1, 100.0) == 1
    assert lib.cpm_update_budget((1 << 24) + 1, 100.0) == 1 << 24
    assert lib.cpm_update_budget(1000, -5.0) == 0


def test_new_symbols_are_declared_bound_and_exported(cpm):
    lib = cpm.binding.load_library()
    text = (Path(__file__).resolve().parent.parent / "include" / "cpm" / "cpm_ext.h").read_text()
    for name in ("cpm_update_budget", "cpm_selection_select_pending", "cpm_selection_finish_budget", "cpm_selection_counts"):
        assert hasattr(lib, name), name
        assert name in cpm.binding.EXT_SYMBOLS
        assert name + "(" in text


def test_argument_errors_before_any_device_work(cpm):
    """A null context is refused by every new entry point (CPM_ERR_INVALID_ARGUMENT) before anything touches a device.  That is all that can be
    asked without one: cpm_create fails with CPM_ERR_NO_DEVICE where no GPU is visible (test_abi.py::test_no_cpu_fallback), so no context
    exists here to reach the functions' own checks with.  Those -- null selection / keys / list, negative budget, finish without begin,
    finish twice, each refused with nothing enqueued -- are exercised in test_budget_gpu.py::test_argument_errors."""
    lib = cpm.binding.load_library()
    dummy = (C.c_uint32 * 4)()
    a, b = C.c_int32(7), C.c_int32(7)
    assert lib.cpm_selection_select_pending(None, None, dummy, 0, 4, None) == CPM_ERR_INVALID_ARGUMENT
    assert lib.cpm_selection_finish_budget(None, None, dummy, 1, dummy, None) == CPM_ERR_INVALID_ARGUMENT
    assert lib.cpm_selection_counts(None, None, C.byref(a), C.byref(b)) == CPM_ERR_INVALID_ARGUMENT
    assert (a.value, b.value) == (7, 7)       # nothing written
