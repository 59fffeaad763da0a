"""What tests/test_cpu_wideband_shift.py and tests/test_gpu_wideband_shift.py share: the mixer of amps_recc_set_wideband_shift stated in
numpy (binary32 as the kernels run it, and float64), its error bound, and a small tone block for the narrow banks."""
import functools
from fractions import Fraction

import numpy as np

import slicerbound as sb

U = sb.U32                                        # 2^-24
# What one mixed sample may differ by from x e^{-j 2 pi n step}, relative to |x| (xl_mix of gr_amps_amd/csrc/recc_xlate.hip.h):
#   the phase is the top 24 bits of the wrapped product, truncated: up to 2^-24 of a turn, 2 pi u rad, and so |dw| <= 2 pi u;
#   sincospif: each component within 2 ulp of a value <= 1 (ulp <= u below 1; +-1 and 0 are exact): |dw| <= 2 sqrt(2) u;
#   the complex product: each component is two products and a sum, every one rounded to nearest (relative u, of terms <= |x|) --
#   the kernel fuses the last two, numpy does not: three roundings at most, |dz| <= 3 sqrt(2) u |x|.
DELTA = (2.0 * np.pi + 5.0 * np.sqrt(2.0)) * U    # 13.35 u = 7.96e-7
SHIFTS = (6543.21, -11000.0)


def step_of(shift_hz, fs):
    """shift_hz / fs as a 0.64 fixed-point fraction of a turn, two's complement (xlate_steps_from, in exact rational arithmetic: the
    library's long double may differ in the last of the 64 bits, 2^-40 of what the mixer looks at)"""
    f = Fraction(float(shift_hz)) / Fraction(float(fs))
    f -= f.numerator // f.denominator
    return int(f * (1 << 64)) & ((1 << 64) - 1)


def quantised_hz(step, fs, negative):
    return float((Fraction(step, 1 << 64) - (1 if negative and step else 0)) * Fraction(float(fs)))


def _top24(n, step, n0=0):
    idx = (np.arange(n, dtype=np.uint64) + np.uint64(n0 & ((1 << 64) - 1)))
    with np.errstate(over="ignore"):
        return ((idx * np.uint64(step)) >> np.uint64(40)).astype(np.int64)


def phasor32(n, step, n0=0):
    """complex64 [n]: e^{-j 2 pi top24 / 2^24} with float32 cos / sin, the quarter turns exact as sincospif has them"""
    top = _top24(n, step, n0)
    quad, rest = top >> 22, top & ((1 << 22) - 1)
    ang = -2.0 * np.pi * rest.astype(np.float64) / float(1 << 24)
    w = (np.cos(ang) + 1j * np.sin(ang)) * np.array([1, -1j, -1, 1j])[quad]
    w = (w.real.astype(np.float32) + 1j * w.imag.astype(np.float32)).astype(np.complex64)
    return w


def mix32(x, step, n0=0):
    """the kernels' mixer in numpy: the top 24 bits of n step, float32 cos / sin, a complex64 product"""
    x = np.asarray(x, np.complex64)
    return (x * phasor32(x.shape[0], step, n0)).astype(np.complex64)


def mix64(x, step, n0=0):
    """x e^{-j 2 pi n step / 2^64} in float64, the phase reduced exactly before the cosine"""
    n = x.shape[0]
    idx = (np.arange(n, dtype=np.uint64) + np.uint64(n0 & ((1 << 64) - 1)))
    with np.errstate(over="ignore"):
        turns = idx * np.uint64(step)
    ph = (turns >> np.uint64(11)).astype(np.float64) / float(1 << 53)   # 53 bits of the fraction of a turn: exact in float64
    return np.asarray(x, np.complex128) * np.exp(-2j * np.pi * ph)


def frame_weights(x, h, D):
    """float64 [frames]: sum_i |h[i]| |x[n0 + i]| over each frame's samples -- what a relative error DELTA of every mixed sample can
    move any bin of that frame by"""
    h = np.abs(np.asarray(h, np.float64))
    L = h.size
    nfr = x.shape[0] // D
    xp = np.concatenate([np.zeros(L - D), np.abs(np.asarray(x[:nfr * D], np.complex128))])
    win = np.lib.stride_tricks.sliding_window_view(xp, L)[::D]
    assert win.shape[0] == nfr
    return win @ h


@functools.lru_cache(maxsize=None)
def narrow_tone_block(M, D):
    """about 300 frames at fs = M x 30 kHz: noise at 0.02 plus tones 3 kHz above the centres of bins 0, 1, M / 2 - 1, M / 2 and M - 1"""
    fs = M * 30e3
    rng = np.random.default_rng(41 + M + D)
    n = 300 * D + 37
    t = np.arange(n)
    x = 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for k, a in zip((0, 1, M // 2 - 1, M // 2, M - 1), (1.0, 0.8, 0.6, 0.9, 0.7)):
        f = (k if k < M // 2 else k - M) * 30e3 + 3e3
        x += a * np.exp(2j * np.pi * f * t / fs)
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x
