"""tests/xlateref.py held to the restated reference (oracle.firdes_low_pass, oracle.freq_xlating_fir) and to the library's host
arithmetic (amps_recc_xlate_shared_plan) before the GPU tests of tests/test_gpu_xlate_taps.py lean on it.  No GPU."""
import os

import numpy as np
import pytest

import oracle
import xlateref
from gr_amps_amd import capi

TOL_ORACLE = 6.0e-5        # tests/test_gpu_xlate.py: the restated block against a float result, noise * 0.5 through the 299 taps of gain 3

# (decim, sps) -> rate = 20 kHz * sps * decim: the smallest supported samples per symbol at every decimation, and the shipped rates
RATES = [20e3 * 3 * d for d in (1, 2, 4, 5, 6, 8, 10, 12, 16, 20)] + [400e3, 1.0e6, 2.4e6, 3.2e6]
LENGTHS = [3, 7, 9, 15, 17, 23, 25, 31, 33, 39, 41, 47, 297, 303, 1017, 1023, 1273, 1279, 2393, 2399]


@pytest.mark.parametrize("fs", RATES, ids=lambda r: "%gk" % (r / 1e3))
def test_width_for_gives_the_length_asked_for(fs):
    built = os.path.exists(capi.LIB_PATH)
    for n in LENGTHS:
        w = xlateref.width_for(fs, n)
        assert oracle.firdes_low_pass(3, fs, 10e3, w).size == n, (fs, n)
        if built and n <= 1279:                               # a length every shared kernel takes: each of these rates has a plan
            plan = capi.subband_plan(fs, w)
            assert plan and all(p[2] == n for p in plan), (fs, n, plan)


def test_pad8_and_ulps():
    assert [xlateref.pad8(n) for n in (1, 7, 8, 9, 2399)] == [8, 8, 8, 16, 2400]
    a = np.array([1.0, -1.0, 0.0, 1e-20], np.float32)
    assert np.array_equal(xlateref.ulps_apart(a, a), [0, 0, 0, 0])
    assert np.array_equal(xlateref.ulps_apart(a, np.nextafter(a, np.float32(2))), [1, 1, 1, 1])
    assert xlateref.ulps_apart(np.float32(0.0), np.float32(-0.0)) == 0
    assert xlateref.ulps_apart(np.float32(1.0), np.float32(2.0)) == 1 << 23


@pytest.mark.parametrize("p,q,decim", [(3, 3, 2), (-3, 3, 2), (3, 5, 2), (1, 1, 4), (0, 1, 1)])
def test_exact_meets_the_restated_block(p, q, decim):
    """the integer-phase formula against the restated GNU Radio block (composite taps and rotator, fp32) on 6000 samples of the
    input tests/test_gpu_xlate.py uses, within that file's bound; and against the plain float64 formula, which at these indices is
    the same number to rounding"""
    fs = 400e3
    rng = np.random.default_rng(7)
    n = 6000
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) * np.float32(0.5)
    taps = oracle.firdes_low_pass(3, fs, 10e3, 4.5e3)
    assert taps.size == 299
    fc = fs * p / 2.0 ** q
    e = xlateref.exact(x, taps, p, q, 0, decim)
    ref = oracle.freq_xlating_fir(x, taps, fc, fs, decim)
    assert e.shape == ref.shape == (n // decim,)
    assert np.abs(e - ref).max() <= TOL_ORACLE, np.abs(e - ref).max()
    assert np.abs(e - xlateref.exact_hz(x, taps, fc, fs, decim)).max() <= 1e-11
    assert np.abs(e).max() > 0.5


def test_exact_in_mid_stream_and_beyond_2_to_the_32():
    """a window of the stream with its history equals the same outputs of the whole stream; and the phase is exact where float64
    fc n / fs is not: at n = 2^32 + 5 and p / 2^q = 3 / 2^20 the integer phase is (3 n mod 2^20) / 2^20 to the last bit"""
    rng = np.random.default_rng(8)
    n, decim = 4000, 5
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    taps = oracle.firdes_low_pass(3, 300e3, 10e3, xlateref.width_for(300e3, 47))
    whole = xlateref.exact(x, taps, 37, 9, 0, decim)
    first = 2000                                              # a multiple of decim; 50 >= ntaps - 1 samples of history, also one
    part = xlateref.exact(x[first - 50:], taps, 37, 9, first - 50, decim)
    assert np.abs(part[10:] - whole[first // decim:]).max() <= 1e-12
    base = (1 << 32) + 5
    one = np.ones(1, np.complex64)
    got = xlateref.exact(one, np.ones(1), 3, 20, base, 1)[0]
    turns = ((3 * base) % (1 << 20)) / float(1 << 20)
    assert got == np.exp(-2j * np.pi * turns) and 0 < turns < 1


def test_impulse_expected_is_the_convolution():
    """on impulses the read-back IS the exact formula: every value equal, the zeros exact, at the four centres"""
    decim, ntp = 6, 16
    h = np.zeros(ntp, np.float32)
    h[:9] = oracle.firdes_low_pass(3, 360e3, 10e3, xlateref.width_for(360e3, 9))
    imp = [(3, 4.0), (30, -2.0), (61, 0.5j), (92, -8.0j), (119, 1.0), (148, 2.0)]       # every residue mod 6
    n = 180
    x = xlateref.impulse_stream(n, imp)
    for quarter in (0, 1, -1, 2):
        want = xlateref.exact(x, h, quarter, 2, 0, decim)
        got = xlateref.impulse_expected(h, decim, n // decim, imp, quarter)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(h).max()
        assert np.array_equal(got == 0, np.abs(want) < 1e-30)
    back, seen = xlateref.taps_from_impulses(xlateref.impulse_expected(h, decim, n // decim, imp[:1] + imp[1:2] + imp[4:], 0), ntp, decim,
                                             imp[:1] + imp[1:2] + imp[4:])
    assert np.array_equal(back[seen], h[seen]) and seen.sum() >= 8
    with pytest.raises(AssertionError):
        xlateref.impulse_expected(h, decim, 30, [(3, 1.0), (25, 1.0)], 0)                # 22 apart: the responses could overlap
