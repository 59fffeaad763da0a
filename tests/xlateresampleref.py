"""Plain helpers for the rational translate stage's tests (tests/test_cpu_xlate_resample.py, tests/test_gpu_xlate_resample.py), beside
tests/xlateref.py: the float64 statement of the stage -- scipy.signal.upfirdn on the mixed stream -- the definition's own double
sum to hold it to, the phases of a prototype, the suite's bound over the longest phase, and what a train of real impulses reads
back from the prototype's taps.  numpy, scipy and Python integers only; nothing here touches the library."""
import numpy as np
from scipy.signal import upfirdn

import xlateref


def nout(n, L, M):
    """outputs delivered after n input samples in all: the k with floor(k M / L) <= n - 1, ceil(L n / M) of them"""
    return -(-L * n // M)


def prototype_ntaps(fs, width, L):
    """N_g: the design's length at the up-sampled rate, int(74 L fs / (22 width)) made odd"""
    n = int(74.0 * L * fs / (22.0 * width))
    return n if n & 1 else n + 1


def design(gain, fs, cutoff, width):
    """firdes.low_pass(gain, fs, cutoff, width, WIN_BLACKMAN) in float64, rounded to float32 at the end: the library's design formula
    restated (int(74 fs / (22 width)) made odd taps, windowed sinc normalised to DC gain `gain`), for prototypes longer than
    oracle.firdes_low_pass holds.  Equal to it to the last float32 bit or the one beside it (sin / cos of two maths libraries)."""
    n = int(74.0 * fs / (22.0 * width))
    n += 1 - (n & 1)
    i = np.arange(n, dtype=np.float64)
    k = i - (n - 1) // 2
    win = 0.42 - 0.5 * np.cos(2.0 * np.pi * i / (n - 1)) + 0.08 * np.cos(4.0 * np.pi * i / (n - 1))
    w0 = 2.0 * np.pi * cutoff / fs
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(k == 0, w0 / np.pi, np.sin(k * w0) / (k * np.pi)) * win
    return (t * gain / t.sum()).astype(np.float32)


def phases(g, L):
    """[L][ntp]: h_p[i] = g[L i + p], zero beyond len(g); ntp = ceil(len(g) / L) padded to a multiple of 8.  Keeps g's dtype."""
    g = np.asarray(g)
    ntp = xlateref.pad8(-(-len(g) // L))
    h = np.zeros((L, ntp), g.dtype)
    for p in range(L):
        part = g[p::L]
        h[p, :len(part)] = part
    return h


def mixed(x, fc, fs):
    """z[n] = x[n] e^{-j 2 pi fc n / fs} in float64, the stream starting at sample 0"""
    n = np.arange(len(x))
    return np.asarray(x).astype(np.complex128) * np.exp(-2j * np.pi * fc * n / fs)


def exact(x, g, fc, fs, L, M):
    """the float64 statement of the stage: upfirdn(g, z, up=L, down=M), cut to the outputs whose last input has arrived"""
    y = upfirdn(np.asarray(g, np.float64), mixed(x, fc, fs), up=L, down=M)
    return y[: nout(len(x), L, M)]


def brute(x, g, fc, fs, L, M):
    """the definition's own double sum: k M = L q + p, y[k] = sum_i h_p[i] z[q - i], samples before the stream's start zero"""
    h = phases(np.asarray(g, np.float64), L)
    z = mixed(x, fc, fs)
    y = np.zeros(nout(len(x), L, M), np.complex128)
    for k in range(len(y)):
        q, p = divmod(k * M, L)
        for i in range(h.shape[1]):
            if 0 <= q - i < len(z):
                y[k] += h[p, i] * z[q - i]
    return y


def bound(g, L, xmax):
    """xlateref.bound taken over the longest phase: (ntp + 16) 2^-24 max_p sum|h_p| max|x|"""
    h = phases(np.asarray(g, np.float64), L)
    return (h.shape[1] + 16) * 2.0 ** -24 * np.abs(h).sum(axis=1).max() * xmax


def impulse_expected(g, L, M, n_out, impulses):
    """What n_out outputs read back from real impulses (n0, a) at centre 0: y[k] = a g[k M - L n0] where 0 <= k M - L n0 < len(g),
    exactly zero elsewhere; also which g[j] were read.  Impulses must be further apart than a phase is long (asserted), so at most
    one product enters each fma chain and a (a power of two) times a float32 is exact.  Returns (y complex64, seen bool [len(g)])."""
    g = np.asarray(g, np.float32)
    ntp = xlateref.pad8(-(-len(g) // L))
    pos = sorted(n0 for n0, _ in impulses)
    assert all(b - a > ntp + M for a, b in zip(pos, pos[1:])), "responses overlap"
    y = np.zeros(n_out, np.complex64)
    seen = np.zeros(len(g), bool)
    for n0, a in impulses:
        assert np.imag(a) == 0
        k = np.arange(-(-L * n0 // M), min(n_out, (L * n0 + len(g) - 1) // M + 1))
        j = k * M - L * n0
        y[k] = np.float32(np.real(a)) * g[j]
        seen[j] = True
    return y + np.complex64(0), seen                             # -0 -> +0: the sign of a zero is not specified
