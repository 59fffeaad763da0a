"""Degenerate sample VALUES for the slicer tests (tests/test_cpu_sample_values.py, tests/test_gpu_sample_values.py): seeded generators
of complex64 rows on which ties, exact zeros, negative zeros, antipodal steps, subnormal products and products near overflow are the
rule -- on Gaussian noise plus FM bursts, which every other generator of the suite draws, each of them has probability zero.

  V1 lattice      integer components in {-2..2}, 5 % of the zero components negated
  V2 axis walk    {1, i, -1, -i} x amplitude 1..3: every phase step is exactly 0, +-pi/2 or pi, both zero signs on the vanishing part
  V3 zero runs    a 20 dB noise-then-carrier row with runs of exact zeros cut into it, straddling lane / word / tile boundaries
  V4 constants    x = 1, x = -1 - 0j, x = 1 - 1j, and real-only streams with xi = +0 / xi = -0: every conj-product sine is a zero;
                  one real-only pattern makes every one of them -0
  V5 scales       one noise-then-carrier row times 2^k, k = -75 .. +59 (exact in binary32)
  V6 poison       NaN, +-Inf, +-FLT_MAX: outside the contract of include/amps_recc_numerics.h; only containment is asserted

Negative zeros are written through float32 views: arithmetic on complex numbers does not preserve them."""
import numpy as np

from gr_amps_amd import synth

LANE, WORD, TILE, HALO = 8, 64, 512, 1024       # samples per lane / packed word / wave tile / inter-push halo (amps_recc_numerics.h)
ROW = 8192                                      # samples per row of the bit and tap tests: 16 tiles
SCALES = (-75, -63, -50, -20, 0, 20, 50, 59)
FLT_MAX = np.finfo(np.float32).max


def _c64(re, im):
    a = np.empty((len(re), 2), np.float32)
    a[:, 0] = re
    a[:, 1] = im
    return a.view(np.complex64)[:, 0]


def _parts(x):
    """float32 views of a complex64 row: (real, imaginary), writable"""
    v = x.view(np.float32).reshape(-1, 2)
    return v[:, 0], v[:, 1]


def _negate_some_zeros(comp, rng, frac=0.05):
    z = np.nonzero(comp == 0)[0]
    pick = z[rng.random(z.size) < frac]
    comp[pick] = np.float32(-0.0)


def lattice(n=ROW, seed=1):
    """V1: xr, xi uniform in {-2..2}; a random 5 % of the zero components are -0.0"""
    rng = np.random.default_rng(seed)
    x = _c64(rng.integers(-2, 3, n), rng.integers(-2, 3, n))
    for comp in _parts(x):
        _negate_some_zeros(comp, rng)
    return x


def axis_walk(n=ROW, seed=2):
    """V2: amplitude (1..3) x one of {1, i, -1, -i}, drawn per sample; the vanishing component is +0 or -0 with equal probability"""
    rng = np.random.default_rng(seed)
    amp = rng.integers(1, 4, n).astype(np.float32)
    axis = rng.integers(0, 4, n)
    zero = np.where(rng.integers(0, 2, n) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    sign = np.where(axis >= 2, np.float32(-1), np.float32(1))
    on_real = axis % 2 == 0
    return _c64(np.where(on_real, sign * amp, zero), np.where(on_real, zero, sign * amp))


def carrier_row(n, sps, seed, snr_db=20.0, first=2000):
    """noise at snr_db below a unit carrier for `first` samples, then the start of a seizure burst (dotting, word sync, words): the
    first n samples of a one-burst synth.make_channel_block row"""
    burst = (synth.BURST_PREFIX_BITS + 7 + 7 * 240) * 2 * sps
    x, truth = synth.make_channel_block(first + burst + 2 * sps + 1, 1, seed=seed, sps=sps, snr_db=snr_db, first=first, jitter=False)
    assert len(truth) == 1 and truth[0][0] == first
    return np.ascontiguousarray(x[:n])


def run_lengths(sps):
    return [1, 2, sps - 1, sps, sps + 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1024 + sps]


def place_runs(sps, n=ROW):
    """[(start, length)] for run_lengths(sps): run i straddles a lane (8), word (64) or tile (512) boundary, in turn -- the boundary
    falls inside the run (a run of one sample ends at it) -- and consecutive runs are more than 2 sps + 8 samples apart.  The layout
    is pushed as far towards the end of the row as it fits, so that the long runs lie where a ragged push schedule has its later,
    smaller pieces."""
    for cur0 in range(n - n % TILE, -1, -TILE):
        out, cur = [], cur0 + 40
        for i, L in enumerate(run_lengths(sps)):
            size = (LANE, WORD, TILE)[i % 3]
            before = max(1, L // 2)
            B = -(-(cur + before) // size) * size
            out.append((B - before, L))
            cur = B - before + L + 2 * sps + 9
        if cur + 64 < n:
            return out
    raise ValueError("the runs do not fit into %d samples" % n)


def zero_runs(sps, n=ROW, seed=3, negative=False, leading=False):
    """V3: (row, runs).  carrier_row with exact zeros written over [start, start + length) of every run of place_runs; negative: every
    run is -0.0 - 0.0j instead of +0.0 + 0.0j; leading: the stream also begins with a run (of sps + 2 samples)."""
    x = carrier_row(n, sps, seed)
    runs = place_runs(sps, n)
    if leading:
        assert runs[0][0] > 2 * sps + 2
        runs = [(0, sps + 2)] + runs
    re, im = _parts(x)
    z = np.float32(-0.0 if negative else 0.0)
    for s, L in runs:
        re[s:s + L] = z
        im[s:s + L] = z
    return x, runs


def near_runs(runs, sps, n):
    """mask of the samples within sps of a zero run (the run itself included): every window there holds an exact zero"""
    m = np.zeros(n, bool)
    for s, L in runs:
        m[max(0, s - sps):s + L + sps] = True
    return m


def constants(n=ROW, seed=4):
    """V4: {name: row}"""
    rng = np.random.default_rng(seed)
    k = (rng.integers(1, 4, n) * (rng.integers(0, 2, n) * 2 - 1)).astype(np.float32)
    full = lambda v: np.full(n, v, np.float32)
    # (+a, -0), (-a, -0), (-a, +0), (+a, +0), ...: the one real-only pattern on which BOTH products of every sine vanish with the signs
    # that make fmaf(xi, pr, -(xr * pi)) = (-0) + (-0) = -0, sample after sample -- so a boxcar sum of them is -0 too
    amp = rng.integers(1, 4, n).astype(np.float32)
    cyc_re = np.tile(np.array([1, -1, -1, 1], np.float32), n // 4 + 1)[:n]
    cyc_im = np.tile(np.array([-0.0, -0.0, 0.0, 0.0], np.float32), n // 4 + 1)[:n]
    return {
        "negzero_sines": _c64(amp * cyc_re, cyc_im),
        "one": _c64(full(1.0), full(0.0)),
        "minus_one_negzero": _c64(full(-1.0), full(-0.0)),
        "one_minus_i": _c64(full(1.0), full(-1.0)),
        "real_only_poszero": _c64(k, full(0.0)),
        "real_only_negzero": _c64(k, full(-0.0)),
    }


def scaled(x, k):
    """x 2^k, exact: ldexp on the float32 parts (the rows used stay inside the normal range)"""
    out = np.ldexp(x.view(np.float32), k).astype(np.float32)
    assert np.array_equal(np.ldexp(out.astype(np.float64), -k), x.view(np.float32).astype(np.float64)), "scaling was not exact"
    return out.view(np.complex64)


def scales(sps, n=ROW, seed=5):
    """V5: {k: carrier_row x 2^k}.  |x| <= 1.5 or so, so k = +59 stays inside the stated |x| < 2^60; products of two samples leave the
    normal range at k = -75 and -63 and sit on AMPS_MX_FLOOR = 2^-100 at k = -50"""
    base = carrier_row(n, sps, seed)
    assert np.abs(base.view(np.float32)).max() < 2.0
    return {k: scaled(base, k) for k in SCALES}


def classes(sps, n=ROW):
    """{class: {name: row}} for V1 .. V5 at one samples-per-symbol"""
    return {
        "V1": {"lattice": lattice(n)},
        "V2": {"axis": axis_walk(n)},
        "V3": {"plus": zero_runs(sps, n)[0], "minus": zero_runs(sps, n, negative=True)[0], "leading": zero_runs(sps, n, leading=True)[0]},
        "V4": constants(n),
        "V5": {"2^%d" % k: row for k, row in scales(sps, n).items()},
    }


EXACT_CLASSES = ("V1", "V2", "V4")      # integer-valued: tests/valueref.py is exact on them

POISON = {
    "nan": (np.nan, np.nan),
    "inf": (np.inf, -np.inf),
    "flt_max": (FLT_MAX, -FLT_MAX),
}


def poison(x, kind, start, length=100):
    """V6: a copy of row x with [start, start + length) overwritten: alternating signs, on both components"""
    a, b = POISON[kind]
    y = x.copy()
    re, im = _parts(y)
    alt = np.arange(length) % 2 == 0
    re[start:start + length] = np.where(alt, a, b).astype(np.float32)
    im[start:start + length] = np.where(alt, b, a).astype(np.float32)
    return y
