"""The perturbation bound of tests/slicerbound.py (what the wideband bit tests allow between a binary32 slicer and the float64
statement) on the CPU model: it must accept the model's own bits on perturbed binary32 data, and catch one flipped bit where the
statistic is far from zero.  No GPU."""
import numpy as np
import pytest

import oracle
import slicerbound as sb


def _channel(n, sps, seed):
    """float64 frames of one channel: an FSK burst at 20 dB between stretches of noise, a quiet start (the stream start's edge)"""
    rng = np.random.default_rng(seed)
    sym = rng.integers(0, 2, n // sps + 1) * 2 - 1
    f = np.repeat(sym, sps)[:n] * 8e3
    ph = 2 * np.pi * np.cumsum(f) / (20e3 * sps) + rng.uniform(0, 2 * np.pi)
    on = (np.arange(n) > n // 4) & (np.arange(n) < 3 * n // 4)
    y = on * np.exp(1j * ph) + 0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)
    y[:5] *= 1e-3
    return y


@pytest.mark.parametrize("spec", [0, 1, 2, 3])
@pytest.mark.parametrize("sps", [2, 3])
def test_bound_accepts_the_model_and_catches_a_flipped_bit(sps, spec):
    n = 64 * 300
    y64 = _channel(n, sps, seed=10 * sps + spec)
    rng = np.random.default_rng(spec)
    # what a filter bank's rounding does to the slicer's input, exaggerated: a perturbation of up to 2e-3 on every frame
    y32 = (y64 + 2e-3 * rng.uniform(-0.7, 0.7, n) + 2e-3j * rng.uniform(-0.7, 0.7, n)).astype(np.complex64)
    eps = np.abs(y32.astype(np.complex128) - y64).max()
    f = oracle.Fused(0, sps, slicer=spec)
    f.push(y32)
    g = f.taps()[2]
    assert len(g) == n
    bad, explained = sb.unexplained(g, y64, eps, sps, spec)
    assert len(bad) == 0, (bad[:10], sb.statistic(y64, sps, spec)[bad[:10]])
    assert explained <= 0.02 * n                     # the bound is not a blanket: differences stay rare
    assert sb.allowed(y64, eps, sps, spec).mean() < 0.1
    # one flipped bit where |S| is large is caught, in the burst and in the noise
    S = sb.statistic(y64, sps, spec)
    ok = sb.allowed(y64, eps, sps, spec)
    for lo, hi in ((n // 4 + 64, 3 * n // 4 - 64), (n // 8, n // 4 - 64)):
        i = lo + int(np.argmax(np.where(ok[lo:hi], 0.0, np.abs(S[lo:hi]))))
        assert not ok[i]
        h = g.copy()
        h[i] ^= 1
        bad, _ = sb.unexplained(h, y64, eps, sps, spec)
        assert list(bad) == [i]
    # and the stream start's ones of specs B and D are held exactly
    if spec in (1, 3):
        h = g.copy()
        h[sps - 1] = 0
        assert list(sb.unexplained(h, y64, eps, sps, spec)[0]) == [sps - 1]
