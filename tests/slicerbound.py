"""The float64 statement of the wideband slicers' bits, and the perturbation bound that says where a binary32 slicer may differ
from it -- TEST INFRASTRUCTURE (tests/test_gpu_wideband_bits.py; the bound's own check: tests/test_cpu_slicer_bound.py).

y64 is one channel's frames from the float64 filter-bank model (oracle/channelizer.py), eps = max |y32 - y64| over the row, y32
what the slicer actually read.  The statistic of each spec of include/amps_recc_numerics.h, frames before the stream being 0:
  A, D  S[n] = the sum of the last sps libm phase steps arg(y[k] conj(y[k-1]));
  B     S[n] = Im(y[n] conj(y[n-sps]));
  C     S[n] = the sum of the last sps Im(y[k] conj(y[k-1])).
The bit is S >= 0; specs B and D slice ones while no partner exists (n < sps).  A binary32 bit may differ from it only where the
perturbation can reach the decision:
  A, D  delta_k = asin(eps / |y_k|) (pi where |y_k| <= eps) bounds the change of arg y_k, so step k moves by at most
        r_k = delta_k + delta_{k-1}.  Allowed where |S| <= sum of r_k over the window + 1e-4 rad (+ sps x 4e-6 rad for spec A's
        arctangent polynomial), or where a step of the window lies within r_k + 1e-4 of +-pi (its principal value may jump by 2 pi);
  B, C  a product y_a conj(y_b) moves by at most eps (|y_a| + |y_b|) + eps^2 and its binary32 evaluation (two products, one
        subtraction; spec C's sum of sps of them) is off by at most 4 u (|y_a| + eps)(|y_b| + eps) per product, u = 2^-24.
"""
import numpy as np

U32 = 2.0 ** -24
TOL_RAD = 1.0e-4         # binary32 rounding of the conj-products in the phase of a step (README: spec D vs float64 libm)
ATAN_STEP_RAD = 4.0e-6   # spec A: |d[n] - atan2(im, re)| <= 4e-6 rad per step (include/amps_recc_numerics.h)
# The filter bank's error per bin, |y32 - y64| <= FFT_C 2^-24 log2(1024) ||Y64(frame)||_2: the usual FFT error bound, taken per frame
# (tests/test_gpu_channelizer.py: test_channelizer_per_bin_error_on_a_wrapped_band).  Measured on the MI355X, worst case over every bin
# and frame: 0.136 (D = 512) / 0.137 (D = 768) on that test's tone block, 0.162 / 0.224 on the burst block of
# tests/test_gpu_wideband_bits.py.  FFT_C = 2.4x the worst of the four (no looser than 4x).
FFT_C = 0.54


def _delay(v, j, fill=0.0):
    """v delayed by j frames, `fill` before the stream"""
    return np.concatenate([np.full(j, fill, v.dtype), v[:len(v) - j]])


def _window(v, sps):
    """sum of the last sps entries (fewer at the stream start)"""
    cs = np.concatenate([[0.0], np.cumsum(v, dtype=np.float64)])
    idx = np.arange(len(v))
    return cs[idx + 1] - cs[np.maximum(idx - sps + 1, 0)]


def statistic(y64, sps, spec):
    """float64 statistic S[n] of slicer spec 0..3 (A, B, C, D) on one channel's frames"""
    y = np.asarray(y64, np.complex128)
    if spec in (0, 3):
        t = y * np.conj(_delay(y, 1))
        return _window(np.where(t == 0, 0.0, np.angle(t)), sps)
    if spec == 1:
        return (y * np.conj(_delay(y, sps))).imag
    return _window((y * np.conj(_delay(y, 1))).imag, sps)


def float64_bits(y64, sps, spec):
    """the bits the statement gives: S >= 0, ones while specs B / D have no partner"""
    g = (statistic(y64, sps, spec) >= 0).astype(np.uint8)
    if spec in (1, 3):
        g[:sps] = 1
    return g


def allowed(y64, eps, sps, spec):
    """bool [n]: where a slicer that read y32 with |y32 - y64| <= eps may differ from float64_bits"""
    y = np.asarray(y64, np.complex128)
    a = np.abs(y)
    S = statistic(y, sps, spec)
    if spec in (0, 3):
        delta = np.full(len(y), np.pi)
        big = a > eps
        delta[big] = np.arcsin(np.minimum(eps / a[big], 1.0))
        r = delta + _delay(delta, 1, np.pi)
        t = y * np.conj(_delay(y, 1))
        step = np.where(t == 0, 0.0, np.angle(t))
        near_pi = (np.pi - np.abs(step) <= r + TOL_RAD).astype(np.float64)
        bound = _window(r, sps) + TOL_RAD + (sps * ATAN_STEP_RAD if spec == 0 else 0.0)
        ok = (np.abs(S) <= bound) | (_window(near_pi, sps) > 0)
    else:
        j = sps if spec == 1 else 1
        ap = _delay(a, j)
        per = eps * (a + ap) + eps * eps + 4.0 * U32 * (a + eps) * (ap + eps)
        ok = np.abs(S) <= (per if spec == 1 else _window(per, sps))
    if spec in (1, 3):
        ok[:sps] = False          # defined as ones: no freedom there
    return ok


def unexplained(bits, y64, eps, sps, spec):
    """indices where `bits` differ from the float64 statement and the bound does not explain it; also the count of explained ones"""
    bits = np.asarray(bits, np.uint8)
    n = len(bits)
    want = float64_bits(y64[:n], sps, spec)
    diff = bits != want
    ok = allowed(y64[:n], eps, sps, spec)
    return np.nonzero(diff & ~ok)[0], int((diff & ok).sum())
