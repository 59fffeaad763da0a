"""A second, independent statement of the four slicer specs of include/amps_recc_numerics.h, per sample, in float64 numpy -- written
from the header's text alone; it shares nothing with oracle/fused_model.c or the kernels.

Precondition that makes it EXACT.  On integer-valued samples with |xr|, |xi| <= 2^10 every product is an integer below 2^21 and every
sum of two products (and every boxcar sum of up to 16 of those) an integer below 2^26: each is representable in binary32 and in
binary64 alike, so no operation rounds in either format, a fused multiply-add equals the multiply followed by the add, and IEEE 754
gives a zero result the same sign in both (x + (-x) = +0; (-0) + (-0) = -0; every other sum of zeros is +0).  The float64
evaluation below therefore IS the binary32 result of specs B, C and D on such input, the sign of zero included -- which is what
decides their bits there.  tests/valuecases.py's classes V1, V2 and V4 are of this kind; check_domain() asserts it.

Spec A evaluates an arctangent polynomial that rounds on any input, so it is held differently (check_spec_a): the sign bit and the
stated tolerance of every d[n] against float64 libm, exact values on the axes and at zero samples, and the boxcar and the comparison
-- which are plain binary32 additions -- restated on the d[n] under test."""
import numpy as np

PI_F = np.float32(float.fromhex("0x1.921fb6p+1"))        # AMPS_PI_F
PI_2_F = np.float32(float.fromhex("0x1.921fb6p+0"))      # AMPS_PI_2_F
DEMOD_TOL_RAD = 1.0e-5                                   # AMPS_DEMOD_TOL_RAD


def check_domain(x):
    v = x.view(np.float32).astype(np.float64)
    assert np.array_equal(v, np.rint(v)) and np.abs(v).max() <= 1024, "valueref is exact on integer samples up to 2^10 only"


def _parts(x):
    v = x.view(np.float32).reshape(-1, 2).astype(np.float64)
    return v[:, 0], v[:, 1]


def _delayed(a, k):
    """a[n - k]; samples before the stream are +0"""
    return np.concatenate([np.zeros(k, a.dtype), a[:len(a) - k]]) if k else a


def sine_product(x, k):
    """Im(x[n] conj(x[n-k])) as the header writes it: fmaf(xi, pr, -(xr * pi))"""
    xr, xi = _parts(x)
    pr, pi = _delayed(xr, k), _delayed(xi, k)
    return xi * pr + (-(xr * pi))


def cosine_product(x, k):
    """Re(x[n] conj(x[n-k])): fmaf(xr, pr, xi * pi)"""
    xr, xi = _parts(x)
    pr, pi = _delayed(xr, k), _delayed(xi, k)
    return xr * pr + xi * pi


def boxcar(d, sps):
    """the header's boxcar, in d's own dtype: the window [n-sps+1, n] is a leading single if its first index is odd, then every
    aligned pair d[2m] + d[2m+1], then a trailing single if n is even; S = ((first + second) + third) + ...; indices before the
    stream hold +0"""
    n, pad = len(d), sps + 1
    dp = np.concatenate([np.zeros(pad, d.dtype), d])
    S = np.empty(n, d.dtype)
    for parity in (0, 1):                                # the cut of the window depends on the parity of n only
        idx = np.arange(parity, n, 2) + pad
        terms, m = [], -(sps - 1)
        while m <= 0:
            if (parity + m) % 2 == 0 and m + 1 <= 0:
                terms.append(dp[idx + m] + dp[idx + m + 1])
                m += 2
            else:
                terms.append(dp[idx + m])
                m += 1
        acc = terms[0]
        for t in terms[1:]:
            acc = acc + t
        S[parity::2] = acc
    return S


def spec_b(x, sps):
    """(d, S, g): g = !signbit(a - b), a = xi[n] xr[n-sps], b = xr[n] xi[n-sps]; ones for the first sps samples.  Taps: d = 0, S = the
    statistic (0 while there is no partner)"""
    xr, xi = _parts(x)
    a, b = xi * _delayed(xr, sps), xr * _delayed(xi, sps)
    s = a - b
    g = (~np.signbit(s)).astype(np.uint8)
    g[:sps] = 1
    s[:sps] = 0.0
    return np.zeros(len(s)), s, g


def spec_c(x, sps):
    """(d', S', g): g = !signbit(S'), S' the ordered boxcar over d' = Im(x conj(x[n-1]))"""
    d = sine_product(x, 1)
    S = boxcar(d, sps)
    return d, S, (~np.signbit(S)).astype(np.uint8)


def _window_sum(w, sps):
    cs = np.concatenate([[0], np.cumsum(w.astype(np.int64))])
    i = np.arange(len(w))
    return cs[i + 1] - cs[np.maximum(i - sps + 1, 0)]


def spec_d(x, sps):
    """(it, ic, g): three sign bits per sample, the wrap bits and the winding number K, as the header lists them"""
    xi = _parts(x)[1]
    it, ic = sine_product(x, 1), sine_product(x, sps)
    sx, st, sc = np.signbit(xi), np.signbit(it), np.signbit(ic)
    sx1 = _delayed(sx, 1)                                # before the stream: +0, sx = 0
    sxs = _delayed(sx, sps)
    wp = ~sx & sx1 & st
    wm = sx & ~sx1 & ~st
    up = ~sx & sxs & sc
    um = sx & ~sxs & ~sc
    K = (up.astype(np.int64) + _window_sum(wm, sps)) - (um.astype(np.int64) + _window_sum(wp, sps))
    g = ((K > 0) | ((K == 0) & ~sc)).astype(np.uint8)
    g[:sps] = 1
    return it, ic, g


SPEC = {1: spec_b, 2: spec_c, 3: spec_d}


def taps32(x, sps, sid):
    """specs B, C, D on the exact domain: (d, S) as binary32 bit patterns (uint32, so -0 != +0) and the bits g"""
    check_domain(x)
    d, S, g = SPEC[sid](x, sps)
    d32, S32 = d.astype(np.float32), S.astype(np.float32)
    assert np.array_equal(d32.astype(np.float64), d) and np.array_equal(S32.astype(np.float64), S)      # nothing rounded
    return d32.view(np.uint32), S32.view(np.uint32), g


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_spec_a(x, sps, d, S, g):
    """spec A's taps (d, S, g of a device or of the model) on an exact-domain row x.  Returns the counts the caller may print."""
    check_domain(x)
    n = len(d)
    re, im = cosine_product(x, 1)[:n], sine_product(x, 1)[:n]
    xr, xi = _parts(x)
    zero = ((xr == 0) & (xi == 0))[:n]
    either = zero | np.concatenate([[True], zero[:-1]])  # x[n] or x[n-1] is zero (the sample before the stream is)
    d = np.ascontiguousarray(d, np.float32)
    # a zero sample: mn = 0 -> q = 0 -> a = 0, no branch taken (-0 is not < 0), and copysign hands on the sign of im: d = +-0
    assert np.array_equal(u32(d)[either], u32(np.copysign(np.float32(0), im[either])))
    ok = ~either
    want = np.arctan2(im, re)
    assert np.array_equal(np.signbit(d[ok]), np.signbit(want[ok]))
    err = np.abs(d[ok].astype(np.float64) - want[ok])
    assert err.max() <= DEMOD_TOL_RAD, err.max()
    # on the axes q = 0 and the result is one of six constants, exactly
    for mask, val in ((ok & (im == 0) & (re > 0), np.float32(0)), (ok & (im == 0) & (re < 0), PI_F), (ok & (re == 0), PI_2_F)):
        assert np.array_equal(u32(d)[mask], u32(np.copysign(val, im[mask]).astype(np.float32)))
    # the boxcar and the comparison, in binary32, on the d under test
    S_want = boxcar(d, sps)
    assert S_want.dtype == np.float32
    assert np.array_equal(u32(S), u32(S_want))
    assert np.array_equal(g, (S_want >= 0).astype(np.uint8))
    return {"plus_pi": int((u32(d) == u32(PI_F)).sum()), "minus_pi": int((u32(d) == u32(-PI_F)).sum()),
            "minus_zero": int((u32(d) == u32(np.float32(-0.0))).sum()), "zero_sample": int(either.sum()), "worst_err": float(err.max())}
