"""The burst mean of amps_recc_burst_power, restated in numpy float32: the reduction of one ring row in the order the gather kernel
states (gr_amps_amd/csrc/recc_block_ring.hip.h), which both received-power flags share.

  lane l   : a_l = 0 + e[l] + e[l + 64] + ...                       ascending, float32
  wave     : for o = 32, 16, 8, 4, 2, 1:  a = a + a[idx ^ o]         float32
  mean     = a[0] / float32(count)

The compiler lowers the kernel's fp32 division to the correctly rounded v_div_scale / v_div_fmas / v_div_fixup sequence under the
project's flags (-fno-fast-math), and IEEE addition is what it is, so numpy float32 reproduces the kernel bit for bit."""
import numpy as np


def gather_mean(entries):
    """float32 mean of `entries` (the ring entries j0 ... j0 + count - 1 of one row, count >= 1) in the gather kernel's order"""
    e = np.ascontiguousarray(entries, np.float32).reshape(-1)
    assert e.size >= 1
    a = np.zeros(64, np.float32)
    for k in range(0, e.size, 64):
        seg = e[k:k + 64]
        a[:seg.size] = a[:seg.size] + seg
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[idx ^ o]
    assert a.dtype == np.float32
    return np.float32(a[0] / np.float32(e.size))


def bits(x):
    """the uint32 pattern of a float32 value or array"""
    return np.ascontiguousarray(x, np.float32).view(np.uint32)
