"""-m gpu: the three FIR kernels of recc_xlate.hip.h -- xlate_fir_kernel (per-row form), xlate_shared_kernel (shared form, staged) and
xlate_shared_wide_kernel (shared form, decimations 5 ... 20) -- read back tap by tap, at every filter length at which their loops take
another path.

B1  Impulses A delta[n - n0], A a power of two, further apart than a response is long: at centre 0 the phasor is (1, 0) and one product
    enters each fma chain, so y[k] = A h32[D k - n0] EXACTLY, and exactly zero where D k - n0 is negative, a pad tap or beyond the
    filter.  At centres +-rate / 4 and rate / 2 the phasor is a power of -j (sincospif is exact at multiples of one half) and the rest
    is the same.  Every read-back of a tap -- whatever n0, tile, push, centre, sample format -- must be the same float32; the filter
    read back must be oracle.firdes_low_pass to one ulp (two roundings of the same double formula) and its padding zero.
B2  The float64 formula within the suite's bound (ntaps + 16) 2^-24 sum|h| max|x| at the shortest, a middle and the longest filter of
    every kernel, at centres that wrap the phase accumulator in every way.
B3  The absolute sample index beyond 2^32: the 64-bit phase against an integer-phase reference, and push boundaries that do not
    reach the bits there either.
B4  Nothing outside the block reaches a result: the block as an interior slice of NaN (a zero pad tap times NaN is NaN).
C   A filter the design formula cannot make is refused (-EINVAL) and leaves the stage as it was."""
import ctypes as C
import errno
import functools

import numpy as np
import pytest

import oracle
import xlateref as xr
from gr_amps_amd import capi

pytestmark = pytest.mark.gpu

SPS = 3                                  # the smallest samples per symbol a handle takes: the lowest rate, the widest reach of width_hz
QUARTERS = (0, 1, -1, 2)                 # centres in quarters of the rate: phasors that are powers of -j
WIDE_D = (5, 6, 10, 12, 16, 20)
FC32, SC16, SC8 = capi.SAMPLES_FC32, capi.SAMPLES_SC16, capi.SAMPLES_SC8


def _rate(D):
    return 20e3 * SPS * D


def _is_wide(D):
    return D in WIDE_D


def _tile_in(D):
    """input samples per tile: 256 outputs of the wide kernel, 2048 inputs of the other two"""
    return 256 * D if _is_wide(D) else 2048


def _amp(m, real=False):
    """+-2^e, e in -3 ... 3, times a power of j unless real"""
    a = 2.0 ** ((5 * m) % 7 - 3) * (-1) ** m
    return a if real else a * (1, 1j, -1, -1j)[(m // 2) % 4]


def _step(D, ntp):
    """impulse spacing: more than ntp + D, and 1 mod D, so that consecutive impulses take consecutive residues"""
    return (ntp + 2 * D) // D * D + D + 1


def _base(D, ntp, shift=0):
    """D impulses of real amplitude, one of every residue mod D, placed so that the tile edge falls among them where the stream allows;
    -> (impulses, stream length with every response complete and a ragged end)"""
    s = _step(D, ntp)
    first = max(0, _tile_in(D) - (D // 2) * s - 1) + shift
    imp = [(first + m * s, _amp(m, real=True)) for m in range(D)]
    assert sorted(n0 % D for n0, _ in imp) == list(range(D))
    return imp, imp[-1][0] + ntp + 2 * D + 3


def _count_run(D, ntp, ntaps, cnt):
    """a stream of exactly cnt outputs (and D - 1 samples left over) whose LAST output reads the filter's centre tap, or as deep a tap
    as the stream is long; further impulses back to the start of the stream"""
    s = _step(D, ntp)
    n0 = D * (cnt - 1) - min(ntaps // 2, D * (cnt - 1))
    imp = [(n, _amp(m + 1)) for m, n in enumerate(range(n0, -1, -s))]
    return imp, D * cnt + D - 1


def _counts(D):
    t = _tile_in(D) // D                                          # outputs per tile
    return (1, t - 1, t, t + 1, t + 2, 2 * t + 1)                 # wide: 1, 255, 256, 257, 258, 513 -- last outputs 0, 254 ... 257, 512


def _same(got, want, what):
    got = got + np.complex64(0)                                   # the sign of a zero is not specified
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("%s: %d of %d outputs differ, the first at %d: got %r, want %r"
                             % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]]))


def _design(D, ntaps):
    fs = _rate(D)
    want = oracle.firdes_low_pass(3, fs, 10e3, xr.width_for(fs, ntaps))
    assert want.size == ntaps
    return want


def _check_taps(h, D, ntaps, seen):
    assert seen.all(), "the impulses read %d of %d taps" % (seen.sum(), seen.size)
    want = _design(D, ntaps)
    apart = xr.ulps_apart(h[:ntaps], want)
    assert apart.max() <= 1, "tap %d read back as %r, the design gives %r" % (apart.argmax(), h[apart.argmax()], want[apart.argmax()])
    assert not h[ntaps:].any(), "a pad tap is not zero"
    assert np.abs(h).max() > 0.04                                 # a filter of DC gain 3 was read, not zeros: its peak is 3 * 20 kHz / rate


def _shared_handle(D, ntaps, quarters, max_out):
    fs = _rate(D)
    r = capi.Recc(n_channels=len(quarters), sps=SPS, max_samples=max_out, max_bursts=4)
    try:
        r.set_xlate_shared(fs, [q * fs / 4 for q in quarters], D, width_hz=xr.width_for(fs, ntaps))
    except BaseException:
        r.close()
        raise
    return r


def _shared_once(r, x):
    r.reset()
    return r.debug_xlate_shared(x)


def _read_back_shared(r, D, ntaps, quarters=QUARTERS):
    """the base run on a fresh stream: the taps as row 0 (centre 0) reads them, checked against the design; every row of the run
    against what those taps give at its centre"""
    ntp = xr.pad8(ntaps)
    imp, n = _base(D, ntp)
    y = _shared_once(r, xr.impulse_stream(n, imp))
    assert y.shape == (len(quarters), n // D) and quarters[0] == 0
    h, seen = xr.taps_from_impulses(y[0], ntp, D, imp)
    _check_taps(h, D, ntaps, seen)
    for c, q in enumerate(quarters):
        _same(y[c], xr.impulse_expected(h, D, n // D, imp, q), "base run, centre %d/4 of the rate" % q)
    return h


def _shared_case(D, ntaps):
    ntp = xr.pad8(ntaps)
    runs = [_count_run(D, ntp, ntaps, cnt) for cnt in _counts(D)] + [_base(D, ntp, shift) for shift in (1, D + 3)]
    with _shared_handle(D, ntaps, QUARTERS, max(n for _, n in runs + [_base(D, ntp)]) // D + 1) as r:
        h = _read_back_shared(r, D, ntaps)
        for imp, n in runs:
            y = _shared_once(r, xr.impulse_stream(n, imp))
            for c, q in enumerate(QUARTERS):
                _same(y[c], xr.impulse_expected(h, D, n // D, imp, q), "%d outputs, centre %d/4 of the rate" % (n // D, q))


# ---- B1
def test_the_lengths_reach_every_head_column():
    """H % D = the head column's last row, H = ntp - 1: the lengths of the wide cases reach every value a multiple of 8 can give, among
    them 0 (D = 5 at 16 taps only) and H / D == 0"""
    lengths = (8, 16, 24, 32, 40, 48, 2400)
    for D in WIDE_D:
        assert {(ntp - 1) % D for ntp in lengths} == {(8 * k - 1) % D for k in range(1, 301)}, D
    assert (16 - 1) % 5 == 0 and all((ntp - 1) % D for D in WIDE_D for ntp in lengths if (D, ntp) != (5, 16))
    assert all((8 - 1) // D == 0 for D in WIDE_D if D > 8)        # ntp < D: the head column is the whole filter


@pytest.mark.parametrize("ntp", [8, 16, 24, 32, 40, 48, 2400])
@pytest.mark.parametrize("D", WIDE_D)
def test_wide_kernel_reads_every_tap_back(gpu, D, ntp):
    _shared_case(D, ntp - 1)


@pytest.mark.parametrize("D", WIDE_D)
def test_wide_kernel_reads_a_padded_filter_back(gpu, D):
    """17 taps padded to 24: seven pad taps at the end of the last whole columns"""
    _shared_case(D, 24 - 7)


@pytest.mark.parametrize("ntp", [8, 16, 304, 1280])
@pytest.mark.parametrize("D", [1, 2, 4, 8])
def test_staged_kernel_reads_every_tap_back(gpu, D, ntp):
    _shared_case(D, ntp - 1)


def _cpg(n_channels, tiles, want=4096):
    """xlate_shared_cpg of recc_xlate.hip.h: channels per workgroup of the staged kernel"""
    groups = min(n_channels, max(1, -(-want // tiles)))
    return -(-n_channels // groups)


def test_staged_kernel_reads_the_same_taps_in_every_channel_of_a_group(gpu):
    """2100 input tiles and three channels: two channels per workgroup and a last group of one.  Impulses at the first tile edge, deep
    in the block and in its last tile; centres 0, rate / 4 and rate / 2"""
    import torch
    D, ntaps, tiles, quarters = 8, 303, 2100, (0, 1, 2)
    ntp = xr.pad8(ntaps)
    n = tiles * 2048
    assert _cpg(3, tiles) == 2 and _cpg(3, 2047) == 1 and _cpg(3, 4096) == 3      # two groups, the second one short
    base, _ = _base(D, ntp)
    imp = base + [(n0 + 1000 * 2048 + 8, _amp(m)) for m, (n0, _) in enumerate(base)] + [(n - ntp - 2 * D - 7 - m * _step(D, ntp), _amp(m)) for m in range(3)]
    x = torch.from_numpy(xr.impulse_stream(n, imp)).to(gpu)
    with _shared_handle(D, ntaps, quarters, n // D) as r:
        h = _read_back_shared(r, D, ntaps, quarters)
        y = _shared_once(r, x)
    assert y.shape == (3, n // D)
    for c, q in enumerate(quarters):
        _same(y[c], xr.impulse_expected(h, D, n // D, imp, q), "channel %d" % c)


def _rows_raw(r, block, ld, nsamp, fmt=FC32):
    """amps_recc_debug_xlate_as on rows of pitch ld (samples): a host array, or (device pointer, keep-alive) of a device block"""
    cap = nsamp + 8
    out = np.zeros((r.n_channels, cap), np.complex64)
    no = C.c_size_t(0)
    if isinstance(block, np.ndarray):
        ptr, mem = capi._hostptr(block), capi.MEM_HOST
    else:
        ptr, mem = C.c_void_p(block[0]), capi.MEM_DEVICE
    rc = capi.load().amps_recc_debug_xlate_as(r._h, ptr, ld, nsamp, fmt, mem, capi._hostptr(out), cap, C.byref(no))
    assert rc == 0, rc
    return out[:, :no.value].copy()


def _pitched(rows, ld, fill):
    """[C][ld] host block holding the rows, the pad columns filled"""
    b = np.full((len(rows), ld), fill, np.complex64)
    for c, x in enumerate(rows):
        b[c, :x.size] = x
    return b


@pytest.mark.parametrize("ntp", [8, 304, 1024])
@pytest.mark.parametrize("D", [1, 2, 4])
def test_per_row_kernel_reads_every_tap_back(gpu, D, ntp):
    """three rows, the impulses of each at other places, a row pitch beyond the samples (pad columns of 1 + j: one of them used is no
    power of two times a tap), the four centres one configuration after the other"""
    ntaps, fs = ntp - 1, _rate(D)
    sets = [_base(D, ntp, shift) for shift in (0, 1, D + 3)]
    n = max(m for _, m in sets)
    runs = [_count_run(D, ntp, ntaps, cnt) for cnt in _counts(D)]
    h = None
    with capi.Recc(n_channels=3, sps=SPS, max_samples=max([n] + [m for _, m in runs]) // D + 1, max_bursts=4) as r:
        for q in QUARTERS:
            r.set_xlate(rate_hz=fs, center_hz=q * fs / 4, decim=D, width_hz=xr.width_for(fs, ntaps))
            y = _rows_raw(r, _pitched([xr.impulse_stream(n, imp) for imp, _ in sets], n + 13, 1 + 1j), n + 13, n)
            assert y.shape == (3, n // D)
            if h is None:
                h, seen = xr.taps_from_impulses(y[0], ntp, D, sets[0][0])
                _check_taps(h, D, ntaps, seen)
            for c, (imp, _) in enumerate(sets):
                _same(y[c], xr.impulse_expected(h, D, n // D, imp, q), "row %d, centre %d/4 of the rate" % (c, q))
            for imp, m in runs:
                r.reset()
                rows = [xr.impulse_stream(m, [(n0, a * 2.0 ** c) for n0, a in imp]) for c in range(3)]
                y = _rows_raw(r, _pitched(rows, m + 5, 1 + 1j), m + 5, m)
                for c in range(3):
                    _same(y[c], xr.impulse_expected(h, D, m // D, [(n0, a * 2.0 ** c) for n0, a in imp], q), "%d outputs, row %d" % (m // D, c))


def _carry_stream(D, ntp):
    """pushes of H - 3 samples (fewer than the history), then a few tiles, then the rest; one impulse inside the first push and one
    inside the last H samples of the second, both read by the following push through the carry alone"""
    H, s = ntp - 1, _step(D, ntp)
    first, second = H - 3, 2 * _tile_in(D) + 5
    end2 = first + second
    at = [2, end2 - 5] + [end2 - 5 - m * s for m in range(1, 4)] + [end2 - 5 + m * s for m in range(1, 4)]
    at = sorted(a for a in at if a - 2 > ntp + D or a == 2)
    imp = [(a, _amp(m + 2)) for m, a in enumerate(at)]
    n = at[-1] + ntp + 2 * D + 1
    assert first < H and end2 - H <= end2 - 5 < end2 and n > end2
    return imp, n, [first, second, n - end2]


@pytest.mark.parametrize("D,ntp", [(12, 40), (5, 2400), (8, 304), (1, 1280)], ids=["wide_d12_40", "wide_d5_2400", "staged_d8_304", "staged_d1_1280"])
def test_shared_kernels_read_an_impulse_through_the_carry(gpu, D, ntp):
    ntaps = ntp - 1
    imp, n, pushes = _carry_stream(D, ntp)
    x = xr.impulse_stream(n, imp)
    with _shared_handle(D, ntaps, QUARTERS, n // D + 1) as r:
        h = _read_back_shared(r, D, ntaps)
        whole = _shared_once(r, x)
        r.reset()
        parts, o = [], 0
        for b in pushes:
            parts.append(r.debug_xlate_shared(x[o:o + b]))
            o += b
    got = np.concatenate(parts, axis=1)
    assert np.array_equal(got.view(np.uint32), whole.view(np.uint32))
    for c, q in enumerate(QUARTERS):
        _same(got[c], xr.impulse_expected(h, D, n // D, imp, q), "three pushes, centre %d/4 of the rate" % q)


@pytest.mark.parametrize("D,ntp", [(2, 304), (4, 1024)])
def test_per_row_kernel_reads_an_impulse_through_the_carry(gpu, D, ntp):
    ntaps, fs = ntp - 1, _rate(D)
    imp, n, pushes = _carry_stream(D, ntp)
    base, nb = _base(D, ntp)
    rows = np.stack([xr.impulse_stream(n, [(n0, a * 2.0 ** c) for n0, a in imp]) for c in range(2)])
    with capi.Recc(n_channels=2, sps=SPS, max_samples=max(n, nb) // D + 1, max_bursts=4) as r:
        r.set_xlate(rate_hz=fs, center_hz=0.0, decim=D, width_hz=xr.width_for(fs, ntaps))
        xb = xr.impulse_stream(nb, base)
        h, seen = xr.taps_from_impulses(r.debug_xlate(np.stack([xb, xb]))[1], ntp, D, base)
        _check_taps(h, D, ntaps, seen)
        for q in (0, -1):
            r.set_xlate(rate_hz=fs, center_hz=q * fs / 4, decim=D, width_hz=xr.width_for(fs, ntaps))
            whole = r.debug_xlate(rows)
            r.reset()
            parts, o = [], 0
            for b in pushes:
                parts.append(r.debug_xlate(rows[:, o:o + b]))
                o += b
            got = np.concatenate(parts, axis=1)
            assert np.array_equal(got.view(np.uint32), whole.view(np.uint32))
            for c in range(2):
                _same(got[c], xr.impulse_expected(h, D, n // D, [(n0, a * 2.0 ** c) for n0, a in imp], q), "row %d, centre %d/4" % (c, q))


@pytest.mark.parametrize("fmt,top", [(SC16, 15), (SC8, 7)], ids=["sc16", "sc8"])
@pytest.mark.parametrize("D,ntp", [(12, 40), (8, 304)], ids=["wide_d12", "staged_d8"])
def test_integer_impulses_read_the_same_taps(gpu, D, ntp, fmt, top):
    """impulses (+-2^k, 0) and (0, +-2^k) up to the format's most negative value -2^top, as a host block and as a device block: the
    taps the fc32 impulses read on the same handle, scaled exactly.  cu8 has no zero sample and is held bitwise to fc32 elsewhere"""
    import torch
    ntaps = ntp - 1
    imp, n = _base(D, ntp, 2)
    vals = [(1 << (top - 1), 0), (0, -(1 << top)), (-(1 << top), 0), (0, 1 << (top - 2)), (1, 0), (0, -1)]
    imp = [(n0, complex(*vals[m % len(vals)])) for m, (n0, _) in enumerate(imp)]
    block = np.zeros((n, 2), capi.SAMPLE_DTYPES[fmt])
    for n0, a in imp:
        block[n0] = (a.real, a.imag)
    with _shared_handle(D, ntaps, QUARTERS, n // D + 1) as r:
        h = _read_back_shared(r, D, ntaps)
        r.reset()
        host = r.debug_xlate_shared_as(block, fmt)
        r.reset()
        dev = r.debug_xlate_shared_as(torch.from_numpy(block).to(gpu), fmt)
    for c, q in enumerate(QUARTERS):
        want = xr.impulse_expected(h, D, n // D, imp, q)
        _same(host[c], want, "host block, centre %d/4 of the rate" % q)
        _same(dev[c], want, "device block, centre %d/4 of the rate" % q)


# ---- B2
def _noise(seed, n, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) * np.float32(scale)


def _centres(fs):
    """(name, centre in Hz); the tone that goes with a centre lies 3 kHz above it"""
    return [("-0.384375 rate", -0.384375 * fs), ("15 kHz", 15e3), ("rate/2", fs / 2), ("-rate/2", -fs / 2), ("+rate", fs), ("-rate", -fs),
            ("rate 2^-40", fs * 2.0 ** -40), ("0", 0.0)]


@functools.lru_cache(maxsize=4)
def _formula_case(D, ntaps, n):
    """input (noise * 0.5 and a unit tone 3 kHz above each of the four distinct centres), the designed taps, and the float64 formula
    per centre -- the reference's arithmetic only, computed once per shape"""
    fs = _rate(D)
    k = np.arange(n)
    x = _noise(100 + D, n, 0.5).astype(np.complex128)
    for fc in (-0.384375 * fs, 15e3, fs / 2, 0.0):
        x += np.exp(2j * np.pi * ((fc + 3e3) / fs) * k)
    x = x.astype(np.complex64)
    taps = _design(D, ntaps)
    e = [xr.exact_hz(x, taps, fc, fs, D) for _, fc in _centres(fs)]
    for a in (x, taps):
        a.setflags(write=False)
    return x, taps, e


def _check_formula(y, D, ntaps, n):
    x, taps, exact = _formula_case(D, ntaps, n)
    names = [name for name, _ in _centres(_rate(D))]
    bound = xr.bound(taps, np.abs(x).max())
    assert y.shape == (len(names), n // D)
    for c, name in enumerate(names):
        err = np.abs(y[c] - exact[c]).max()
        print("D = %d, %d taps, centre %s: max |y - exact| = %.3g, bound %.3g, max |exact| = %.3g" % (D, ntaps, name, err, bound, np.abs(exact[c]).max()))
        assert err <= bound, (name, err, bound)
        assert np.abs(exact[c]).max() > 100 * bound, name
    bits = y.view(np.uint32)
    at = names.index
    assert np.array_equal(bits[at("+rate")], bits[at("0")]) and np.array_equal(bits[at("-rate")], bits[at("0")])
    assert np.array_equal(bits[at("rate/2")], bits[at("-rate/2")])
    assert not np.array_equal(bits[at("rate/2")], bits[at("0")])


@pytest.mark.parametrize("ntp", [8, 304, 2400])
@pytest.mark.parametrize("D", WIDE_D)
def test_wide_kernel_meets_the_exact_formula(gpu, D, ntp):
    ntaps, fs, n = ntp - 1, _rate(D), D * (2 * 256 + 45) + 1
    with capi.Recc(n_channels=8, sps=SPS, max_samples=n // D + 1, max_bursts=4) as r:
        r.set_xlate_shared(fs, [fc for _, fc in _centres(fs)], D, width_hz=xr.width_for(fs, ntaps))
        y = r.debug_xlate_shared(_formula_case(D, ntaps, n)[0])
    _check_formula(y, D, ntaps, n)


@pytest.mark.parametrize("ntp", [8, 304, 1280])
@pytest.mark.parametrize("D", [1, 2, 4, 8])
def test_staged_kernel_meets_the_exact_formula(gpu, D, ntp):
    ntaps, fs, n = ntp - 1, _rate(D), 2 * 2048 + 301
    with capi.Recc(n_channels=8, sps=SPS, max_samples=n // D + 1, max_bursts=4) as r:
        r.set_xlate_shared(fs, [fc for _, fc in _centres(fs)], D, width_hz=xr.width_for(fs, ntaps))
        y = r.debug_xlate_shared(_formula_case(D, ntaps, n)[0])
    _check_formula(y, D, ntaps, n)


@pytest.mark.parametrize("ntp", [8, 304, 1024])
@pytest.mark.parametrize("D", [1, 2, 4])
def test_per_row_kernel_meets_the_exact_formula(gpu, D, ntp):
    ntaps, fs, n = ntp - 1, _rate(D), 2 * 2048 + 301
    x = _formula_case(D, ntaps, n)[0]
    rows = []
    with capi.Recc(n_channels=1, sps=SPS, max_samples=n // D + 1, max_bursts=4) as r:
        for _, fc in _centres(fs):
            r.set_xlate(rate_hz=fs, center_hz=fc, decim=D, width_hz=xr.width_for(fs, ntaps))
            rows.append(r.debug_xlate(x[None, :])[0])
    _check_formula(np.stack(rows), D, ntaps, n)


# ---- B3
def test_the_phase_is_exact_beyond_2_to_the_32_samples(gpu):
    """2.4 Msps / 12, centre rate * p / 2^20 with p odd.  One device block of 12 * 2^18 samples pushed 1366 times: the stream position
    passes 2^32 in the last push.  Its last 2048 outputs and the first push's first 2048 against the integer-phase formula within the
    bound; and the same periodic stream in pushes of half the size on a second handle: the same final outputs bit for bit."""
    import torch
    D, fs, q, p = 12, 2.4e6, 20, 389711
    period = D << 18
    pushes = (1 << 32) // period + 1
    assert p % 2 == 1 and (pushes - 1) * period < (1 << 32) < pushes * period - 2048 * D - 1800
    fc = fs * p / 2.0 ** q
    k = np.arange(period)
    block = (_noise(77, period, 0.5) + np.exp(2j * np.pi * ((fc + 3e3) / fs) * k)).astype(np.complex64)
    taps = oracle.firdes_low_pass(3, fs, 10e3, 4.5e3)
    assert taps.size == 1793
    bound = xr.bound(taps, np.abs(block).max())
    dev = torch.from_numpy(block).to(gpu)
    torch.cuda.synchronize()
    L = capi.load()

    def stream(r, piece, count):
        """push dev[piece * j ...] round and round, count pushes; -> (first, last) push's outputs"""
        nout = piece // D
        out = np.zeros((1, nout), np.complex64)
        no = C.c_size_t(0)
        first = None
        for j in range(count):
            ptr = C.c_void_p(dev.data_ptr() + 8 * ((j * piece) % period))
            rc = L.amps_recc_debug_xlate_shared(r._h, ptr, piece, capi.MEM_DEVICE, capi._hostptr(out), nout, C.byref(no))
            assert rc == 0 and no.value == nout, (j, rc, no.value)
            if j == 0:
                first = out[0].copy()
        return first, out[0].copy()

    def handle():
        r = capi.Recc(n_channels=1, sps=10, max_samples=period // D, max_bursts=4)
        r.set_xlate_shared(fs, [fc], D)
        return r

    with handle() as r:
        first, last = stream(r, period, pushes)
    with handle() as r:
        _, last_half = stream(r, period // 2, 2 * pushes)

    def formula(index0, count):
        """outputs of the periodic stream from absolute sample index0 (a multiple of 12) on"""
        hist = 1800 if index0 else 0                              # >= ntaps - 1 and a multiple of 12
        at = np.arange(index0 - hist, index0 + D * count) % period
        return xr.exact(block[at], taps, p, q, index0 - hist, D)[hist // D:]

    e0 = formula(0, 2048)
    e1 = formula(pushes * period - 2048 * D, 2048)
    for name, got, e in (("first", first[:2048], e0), ("last", last[-2048:], e1)):
        err = np.abs(got - e).max()
        print("%s 2048 outputs: max |y - exact| = %.3g, bound %.3g, max |exact| = %.3g" % (name, err, bound, np.abs(e).max()))
        assert err <= bound, (name, err, bound)
        assert np.abs(e).max() > 100 * bound
    assert np.array_equal(last_half[-2048:].view(np.uint32), last[-2048:].view(np.uint32))


# ---- B4
def _poisoned(gpu, fmt, total):
    """a device tensor [total][2] of the format, all poison: NaN, or full-scale values of alternating sign"""
    import torch
    if fmt == FC32:
        return torch.full((total, 2), float("nan"), dtype=torch.float32, device=gpu)
    info = np.iinfo(capi.SAMPLE_DTYPES[fmt])
    a = np.empty((total, 2), capi.SAMPLE_DTYPES[fmt])
    a[0::2], a[1::2] = info.max, info.min
    return torch.from_numpy(a).to(gpu)


def _samples(fmt, n, seed):
    """[n][2] of the format's dtype: noise * 0.5, or integers over the format's whole range"""
    rng = np.random.default_rng(seed)
    if fmt == FC32:
        return (rng.standard_normal((n, 2)) * 0.5).astype(np.float32)
    info = np.iinfo(capi.SAMPLE_DTYPES[fmt])
    return rng.integers(info.min, info.max + 1, size=(n, 2)).astype(capi.SAMPLE_DTYPES[fmt])


@pytest.mark.parametrize("fmt", [FC32, SC16, SC8], ids=["fc32", "sc16", "sc8"])
@pytest.mark.parametrize("D,ntp", [(12, 304), (20, 2400), (8, 304), (1, 1280)], ids=["wide_d12_304", "wide_d20_2400", "staged_d8_304", "staged_d1_1280"])
def test_shared_kernels_use_nothing_outside_the_block(gpu, D, ntp, fmt):
    """two pushes, each an interior slice -- from an odd sample, thousands of samples of poison before it and behind it -- of one
    device tensor: the bits of the same two pushes from clean host arrays, and finite"""
    import torch
    ntaps, fs = ntp - 1, _rate(D)
    sizes = (2 * _tile_in(D) + 301, _tile_in(D) + 77)
    blocks = [_samples(fmt, n, 40 + i) for i, n in enumerate(sizes)]
    big = _poisoned(gpu, fmt, 4097 + sizes[0] + 8191 + sizes[1] + 8192)
    offs = (4097, 4097 + sizes[0] + 8191)
    assert all(o % 2 == 1 for o in offs)
    for o, b in zip(offs, blocks):
        big[o:o + len(b)] = torch.from_numpy(b).to(gpu)
    with capi.Recc(n_channels=3, sps=SPS, max_samples=sizes[0] // D + 1, max_bursts=4) as r:
        r.set_xlate_shared(fs, [-0.384375 * fs, 0.0, fs / 4], D, width_hz=xr.width_for(fs, ntaps))
        clean = [r.debug_xlate_shared_as(b, fmt) for b in blocks]
        r.reset()
        got = [r.debug_xlate_shared_as(big[o:o + len(b)], fmt) for o, b in zip(offs, blocks)]
    for i in range(2):
        assert clean[i].shape[1] > 0 and np.isfinite(clean[i].view(np.float32)).all() and np.abs(clean[i]).max() > 0
        assert np.isfinite(got[i].view(np.float32)).all(), "push %d" % (i + 1)
        assert np.array_equal(got[i].view(np.uint32), clean[i].view(np.uint32)), "push %d" % (i + 1)


@pytest.mark.parametrize("fmt", [FC32, SC16, SC8], ids=["fc32", "sc16", "sc8"])
@pytest.mark.parametrize("D,ntp", [(2, 304), (4, 1024)])
def test_per_row_kernel_uses_nothing_outside_the_block(gpu, D, ntp, fmt):
    """the same for a pitched block of three rows: every pad column between the rows is poison too"""
    import torch
    ntaps, fs, rows = ntp - 1, _rate(D), 3
    sizes = (2 * 2048 + 301, 2048 + 77)
    ld = sizes[0] + 1023
    blocks = [np.stack([_samples(fmt, n, 50 + 10 * i + c) for c in range(rows)]) for i, n in enumerate(sizes)]      # [rows][n][2]
    big = _poisoned(gpu, fmt, 4097 + 2 * rows * ld + 8192)
    offs = (4097, 4097 + rows * ld)
    for o, b in zip(offs, blocks):
        for c in range(rows):
            big[o + c * ld:o + c * ld + b.shape[1]] = torch.from_numpy(b[c]).to(gpu)
    torch.cuda.synchronize()
    item = big.element_size() * 2
    with capi.Recc(n_channels=rows, sps=SPS, max_samples=sizes[0] // D + 1, max_bursts=4) as r:
        r.set_xlate(rate_hz=fs, center_hz=-0.384375 * fs, decim=D, width_hz=xr.width_for(fs, ntaps))
        clean = [r.debug_xlate_as(b, fmt) for b in blocks]
        r.reset()
        got = [_rows_raw(r, (big.data_ptr() + item * o, big), ld, b.shape[1], fmt) for o, b in zip(offs, blocks)]
    for i in range(2):
        assert clean[i].shape[1] > 0 and np.isfinite(clean[i].view(np.float32)).all() and np.abs(clean[i]).max() > 0
        assert np.isfinite(got[i].view(np.float32)).all(), "push %d" % (i + 1)
        assert np.array_equal(got[i].view(np.uint32), clean[i].view(np.uint32)), "push %d" % (i + 1)


# ---- C
def test_a_filter_the_design_cannot_make_is_refused(gpu):
    """a width that gives fewer than three taps (one tap: the window is 0 / 0) and a cut-off above rate / 2 (firdes.low_pass refuses
    it): -EINVAL from both entry points, the stage left as it was; the shortest and the widest filter the design does make are taken"""
    L = capi.load()
    x = _noise(5, 4000, 0.5)
    inval = -errno.EINVAL

    fs = 400e3
    with capi.Recc(n_channels=1, sps=10, max_samples=4096, max_bursts=4) as r:
        def rc(width=0.0, cutoff=0.0, rate=fs):
            return L.amps_recc_set_xlate(r._h, C.byref(capi.XlateCfg(C.sizeof(capi.XlateCfg), 2, rate, 160e3, 0.0, cutoff, width)))
        assert rc(width=1.7 * fs) == inval and rc(cutoff=fs / 2 + 1) == inval      # and nothing was configured
        assert L.amps_recc_push_raw(r._h, capi._hostptr(x), 16, 16, capi.MEM_HOST) == -errno.ENOSYS
        assert rc() == 0
        before = r.debug_xlate(x[None, :])
        for bad in (dict(width=74 * fs / 44 * 1.0001), dict(width=1.7 * fs), dict(width=100 * fs), dict(width=float("inf")),
                    dict(cutoff=fs / 2 + 1), dict(cutoff=fs), dict(cutoff=float("inf")), dict(cutoff=float("nan")), dict(cutoff=-1.0)):
            assert rc(**bad) == inval, bad
        r.reset()
        after = r.debug_xlate(x[None, :])
        assert np.array_equal(after.view(np.uint32), before.view(np.uint32)) and before.shape == (1, 2000) and np.abs(before).max() > 0
        for good, ntaps in ((dict(width=74 * fs / 44 * 0.9999), 3), (dict(width=xr.width_for(fs, 3), cutoff=fs / 2), 3), (dict(cutoff=fs / 2), 299)):
            assert rc(**good) == 0, good
            y = r.debug_xlate(x[None, :])
            assert np.isfinite(y.view(np.float32)).all() and np.abs(y).max() > 0
            taps = oracle.firdes_low_pass(3, fs, good.get("cutoff", 10e3), good.get("width", 4.5e3))
            assert taps.size == ntaps
            assert np.abs(y[0] - xr.exact_hz(x, taps, 160e3, fs, 2)).max() <= xr.bound(taps, np.abs(x).max())

    fs = 2.4e6
    cen = (C.c_double * 2)(-60e3, 60e3)
    with capi.Recc(n_channels=2, sps=10, max_samples=4096, max_bursts=4) as r:
        def rcs(width=0.0, cutoff=0.0):
            return L.amps_recc_set_xlate_shared(r._h, C.byref(capi.XlateSharedCfg(C.sizeof(capi.XlateSharedCfg), 12, 2, 0, fs, 0.0, cutoff, width, cen)))
        assert rcs(width=1.7 * fs) == inval and rcs(cutoff=fs / 2 + 1) == inval
        assert L.amps_recc_push_raw_shared(r._h, capi._hostptr(x), 16, capi.MEM_HOST) == -errno.ENOSYS
        assert rcs() == 0
        before = r.debug_xlate_shared(x)
        for bad in (dict(width=74 * fs / 44 * 1.0001), dict(width=1.7 * fs), dict(width=float("inf")), dict(cutoff=fs / 2 + 1), dict(cutoff=fs),
                    dict(cutoff=float("nan"))):
            assert rcs(**bad) == inval, bad
        r.reset()
        after = r.debug_xlate_shared(x)
        assert np.array_equal(after.view(np.uint32), before.view(np.uint32)) and before.shape == (2, 333) and np.abs(before).max() > 0
        for good in (dict(width=74 * fs / 44 * 0.9999), dict(width=xr.width_for(fs, 3), cutoff=fs / 2), dict(cutoff=fs / 2)):
            assert rcs(**good) == 0, good
            y = r.debug_xlate_shared(x)
            assert np.isfinite(y.view(np.float32)).all() and np.abs(y).max() > 0
