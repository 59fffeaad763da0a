"""not gpu: the boundary of the shared translate seam (amps_recc_set_xlate_shared / _push_raw_shared / _debug_xlate_shared) refuses a
missing handle without touching a device, and the binding's channel-plan helpers give the AMPS reverse channel frequencies."""
import ctypes as C

import numpy as np
import pytest

from gr_amps_amd import capi


def test_the_three_entry_points_refuse_a_null_handle():
    L = capi.load()
    cen = (C.c_double * 1)(0.0)
    x = capi.XlateSharedCfg(C.sizeof(capi.XlateSharedCfg), 2, 1, 0, 400e3, 0.0, 0.0, 0.0, cen)
    assert C.sizeof(capi.XlateSharedCfg) == 56
    z = np.zeros(8, np.complex64)
    n = C.c_size_t(7)
    assert L.amps_recc_set_xlate_shared(None, C.byref(x)) == -22            # -EINVAL
    assert L.amps_recc_push_raw_shared(None, capi._hostptr(z), 8, capi.MEM_HOST) == -22
    assert L.amps_recc_debug_xlate_shared(None, capi._hostptr(z), 8, capi.MEM_HOST, capi._hostptr(z), 8, C.byref(n)) == -22
    assert {"amps_recc_set_xlate_shared", "amps_recc_push_raw_shared", "amps_recc_debug_xlate_shared"} <= set(capi.EXPORTS)


def test_reverse_channel_frequencies():
    assert capi.reverse_channel_hz(333) == 834.99e6 and capi.reverse_channel_hz(334) == 835.02e6
    assert capi.reverse_channel_hz(1) == 825.03e6
    assert capi.reverse_channel_hz(1023) == 825.0e6 and capi.reverse_channel_hz(991) == 824.04e6
    for bad in (800, 0, 990, 1024, -1):
        with pytest.raises(ValueError):
            capi.reverse_channel_hz(bad)


def test_control_channel_centres():
    a = capi.control_channel_centers("A", 834.69e6)
    assert len(a) == 21 and np.array_equal(np.asarray(a), -300e3 + 30e3 * np.arange(21))
    b = capi.control_channel_centers("B", 834.69e6)
    assert len(b) == 21 and b[0] == a[-1] + 30e3
    ab = capi.control_channel_centers("AB", 835.005e6)
    assert len(ab) == 42 and np.allclose(ab, -615e3 + 30e3 * np.arange(42), rtol=0, atol=1e-6) and max(np.abs(ab)) < 800e3
    with pytest.raises(ValueError):
        capi.control_channel_centers("C", 0.0)
