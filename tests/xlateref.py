"""Plain helpers for the translate seams' tests (tests/test_gpu_xlate_taps.py, tests/test_cpu_xlateref.py): the filter width that gives
a chosen length, the exact formula in float64 with an integer phase, and what a train of impulses reads back from the taps.  numpy and
Python integers only; nothing here touches the library."""
import numpy as np


def width_for(fs, n):
    """the transition width at which the design -- int(74 fs / (22 width)) made odd -- gives exactly n taps, for odd n: the middle of
    the interval (74 fs / (22 (n + 1)), 74 fs / (22 n)] that int() maps to n"""
    return 74.0 * fs / (22.0 * (n + 0.5))


def pad8(n):
    return (n + 7) // 8 * 8


def exact_hz(x, taps, fc, fs, decim):
    """the float64 formula of tests/test_gpu_xlate.py: y[k] = sum_i h[i] z[decim k - i], z[n] = x[n] e^{-j 2 pi fc n / fs}, the stream
    starting at sample 0.  Good while fc n / fs keeps its fraction: n of a few 10^5."""
    n = np.arange(x.size)
    z = x.astype(np.complex128) * np.exp(-2j * np.pi * fc * n / fs)
    full = np.convolve(z, np.asarray(taps, np.float64))[: x.size]
    return full[::decim][: x.size // decim]


def exact(x, taps, p, q, fs_index0, decim):
    """The same formula with the centre given as the dyadic fraction p / 2^q of the rate (p may be negative) and x[i] the sample of
    ABSOLUTE index fs_index0 + i.  The phase of sample n is ((p n) mod 2^q) / 2^q of a turn, in Python integers: exact at every n,
    where float64 fc n / fs has lost 2^-22 turn by n = 2^32.  Samples before x[0] count as zero, so a caller who wants outputs in mid
    stream passes ntaps - 1 samples of history and drops the outputs that reach into it; output k sits at x[decim k]."""
    m = (1 << q) - 1
    turns = np.array([((p * (fs_index0 + i)) & m) for i in range(len(x))], np.float64) / float(1 << q)
    z = np.asarray(x).astype(np.complex128) * np.exp(-2j * np.pi * turns)
    full = np.convolve(z, np.asarray(taps, np.float64))[: len(x)]
    return full[::decim][: len(x) // decim]


def bound(taps, xmax):
    """the suite's bound on |y_gpu - y_exact| per output sample (tests/test_gpu_xlate_shared.py, test_decim_8_meets_the_exact_formula):
    (ntaps + 16) 2^-24 sum|h| max|x| -- an fp32 fma chain of ntaps terms; the 16 covers the 24-bit phasor and the complex multiply"""
    return (len(taps) + 16) * 2.0 ** -24 * np.abs(np.asarray(taps, np.float64)).sum() * xmax


def impulse_stream(n, impulses):
    """complex64 [n]: a[m] at n0[m], zero elsewhere.  impulses: [(n0, a)], a = +-A or +-jA with A a power of two"""
    x = np.zeros(n, np.complex64)
    for n0, a in impulses:
        assert 0 <= n0 < n and x[n0] == 0
        x[n0] = a
    return x


def impulse_expected(h, decim, nout, impulses, quarter):
    """What nout outputs of the stage read back from impulses that do not overlap: y[k] = a (-j)^(quarter n0) h[decim k - n0] where
    0 <= decim k - n0 < len(h), and exactly zero elsewhere.  h: the float32 taps WITH their zero padding (len(h) = the kernel's ntp);
    quarter: the centre in quarters of the rate (0, 1, -1, 2), for which the phasor of sample n0 is exactly (-j)^(quarter n0).  a times
    a power of j times a float32 is exact in float32, so the result is compared with ==.  Impulses must be more than len(h) + decim
    apart (asserted): then at most one product enters each fma chain."""
    h = np.asarray(h, np.float32)
    pos = sorted(n0 for n0, _ in impulses)
    assert all(b - a > len(h) + decim for a, b in zip(pos, pos[1:])), "responses overlap"
    y = np.zeros(nout, np.complex64)
    rot = (1, -1j, -1, 1j)
    for n0, a in impulses:
        f = np.complex64(a) * np.complex64(rot[(quarter * n0) % 4])
        k0 = -(-n0 // decim)                                  # the first output at or after n0
        k = np.arange(k0, min(nout, (n0 + len(h) - 1) // decim + 1))
        if k.size:
            y[k] = f * h[decim * k - n0]
    return y + np.complex64(0)                                # -0 -> +0: the sign of a zero is not specified


def taps_from_impulses(y, ntp, decim, impulses):
    """The other direction, for a centre of 0 and impulses of every residue mod decim: the float32 tap i as output k of impulse
    (n0, a) with decim k - n0 == i reads it, y[k] / a (exact: a is a power of two, real).  Returns (taps [ntp], seen [ntp] bool)."""
    h = np.zeros(ntp, np.float32)
    seen = np.zeros(ntp, bool)
    for n0, a in impulses:
        assert np.imag(a) == 0
        k0 = -(-n0 // decim)
        k = np.arange(k0, min(len(y), (n0 + ntp - 1) // decim + 1))
        i = decim * k - n0
        new = ~seen[i]
        h[i[new]] = (y[k[new]].real / np.float32(np.real(a))).astype(np.float32)
        seen[i[new]] = True
    return h, seen


def ulps_apart(a, b):
    """distance of two float32 arrays in units in the last place, over the ordered integers of their bit patterns"""
    def key(v):
        i = np.asarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))
