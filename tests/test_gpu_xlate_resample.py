"""-m gpu: the shared translate seam behind a rational L / M resampler -- 2.048 Msps x 5/64, 2.5 Msps x 2/25, 768 ksps x 5/16,
1.25 Msps x 4/25 and their like through xlate_shared_rational_kernel (amps_recc_set_xlate_resampled).

No older kernel resamples, so the stage is held to its definition directly: the float64 statement (scipy.signal.upfirdn on the
mixed stream, tests/xlateresampleref.py) within the suite's bound over the longest phase; every tap of the prototype read back
exactly through impulses; bit identity across pushes, tiles, channels and sample formats; the records of a plain IQ-seam handle
fed the stage's own output, and the CPU model behind the float64 helper; the error codes; the command line and the example."""
import errno
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import xlateref as xr
import xlateresampleref as rr
from gr_amps_amd import capi, synth
from gr_amps_amd.host import build_host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS2048 = 2.048e6


def _noise(seed, n, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) * np.float32(scale)


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. the exact formula
@pytest.mark.parametrize("fs,L,M,sps", [(2.048e6, 5, 64, 8), (2.5e6, 2, 25, 10), (768e3, 5, 16, 12), (1.25e6, 4, 25, 10), (1.0e6, 3, 25, 6)],
                         ids=["2048k_5_64", "2500k_2_25", "768k_5_16", "1250k_4_25", "1000k_3_25"])
def test_ratios_meet_the_exact_formula(gpu, fs, L, M, sps):
    """64 L 4 + 37 outputs: four tiles of 64 L and a ragged end (two workgroups and a ragged one at L = 2, whose workgroup holds two
    tiles).  The bound is xlateref.bound over the longest phase: (ntp + 16) 2^-24 max_p sum|h_p| max|x| per output sample -- an fp32
    fma chain of ntp terms; an indexing error (a tap, a phase or a sample off by one) is of the order of the output itself, which
    the second assertion keeps far above the bound."""
    want_out = 64 * L * 4 + 37
    n = (want_out * M) // L                                         # the largest n that delivers exactly want_out
    while rr.nout(n + 1, L, M) == want_out:
        n += 1
    centres = [-0.384375 * fs, 0.4375 * fs]
    x = _noise(12, n, 0.5)
    g = rr.design(3.0 * L, L * fs, 10e3, 4.5e3)
    assert (L, M, sps, -(-len(g) // L)) in capi.resample_plan(fs)
    with capi.Recc(n_channels=2, sps=sps, max_samples=want_out, max_bursts=4) as r:
        r.set_xlate_resampled(fs, centres, L, M)
        y = r.debug_xlate_shared(x)
    assert y.shape == (2, want_out)
    bound = rr.bound(g, L, np.abs(x).max())
    for c, fc in enumerate(centres):
        e = rr.exact(x, g, fc, fs, L, M)
        err = np.abs(y[c] - e).max()
        print("%g Msps x %d/%d, centre %+.1f kHz: max |y - exact| = %.3g, bound %.3g, max |exact| = %.3g" % (fs / 1e6, L, M, fc / 1e3, err, bound, np.abs(e).max()))
        assert err <= bound, (fc, err, bound)
        assert np.abs(e).max() > 100 * bound


# ---- 2. every tap of the prototype, exactly
def _lengths(L):
    """odd prototype lengths N_g from 8 L upwards: the smallest for every pair (N_g mod L, taps per phase ceil(N_g / L) mod 8) with
    the second in (0, 1, 7) that an odd length reaches at all (3 x 24 k is even, for one).  Between them N_g mod L takes every
    residue an odd number can -- all of them at odd L, the odd ones at L = 2 and 4 -- and the taps per phase 0, 1 and 7 mod 8."""
    first = {}
    for n in range(8 * L + 1, 8 * L + 1 + 32 * L, 2):               # two periods of the pair
        key = (n % L, -(-n // L) % 8)
        if key[1] in (0, 1, 7):
            first.setdefault(key, n)
    assert {k[0] for k in first} == {res for res in range(L) if L % 2 or res % 2} and {k[1] for k in first} == {0, 1, 7}
    return sorted(first.values())


@pytest.mark.parametrize("L,M", [(2, 25), (3, 25), (4, 25), (5, 64)])
def test_every_prototype_tap_is_read_back_exactly(gpu, L, M):
    """In the style of tests/test_gpu_xlate_taps.py: centre 0, real impulses of power-of-two amplitudes at every input residue mod M,
    further apart than a phase is long: output k holds a g[k M - L n0] and nothing else, so each g[j] is compared with == and every
    other output is exactly zero.  g is the oracle's firdes.low_pass at the up-sampled rate with the gain times L."""
    fs = 20e3 * 10 * M / L
    for ng in _lengths(L):
        width = xr.width_for(L * fs, ng)
        g = oracle.firdes_low_pass(3.0 * L, L * fs, 10e3, width)
        assert len(g) == ng == rr.prototype_ntaps(fs, width, L)
        ntp = xr.pad8(-(-ng // L))
        gap = ntp + M + 3                                          # coprime spacing is not needed: the residue is planted
        imp = [(m * (gap // M + 2) * M + (7 * m) % M, 2.0 ** (m % 5 - 2) * (-1) ** m) for m in range(M)]
        assert sorted(n0 % M for n0, _ in imp) == list(range(M))
        n = imp[-1][0] + gap
        x = xr.impulse_stream(n, imp)
        want, seen = rr.impulse_expected(g, L, M, rr.nout(n, L, M), imp)
        assert seen.all(), (L, ng)
        with capi.Recc(n_channels=1, sps=10, max_samples=rr.nout(n, L, M), max_bursts=4) as r:
            r.set_xlate_resampled(fs, [0.0], L, M, width_hz=width)
            y = r.debug_xlate_shared(x)
        y = y[0] + np.complex64(0)
        assert y.shape == want.shape
        bad = np.flatnonzero(y.view(np.uint32).reshape(-1, 2) != want.view(np.uint32).reshape(-1, 2))
        assert bad.size == 0, (L, M, ng, bad[:8])
        assert np.count_nonzero(want) >= np.count_nonzero(g)        # every non-zero tap was there to be compared


# ---- 3. streaming
@pytest.mark.parametrize("fs,L,M,sps", [(2.048e6, 5, 64, 8), (2.5e6, 2, 25, 10), (1.25e6, 4, 25, 10)], ids=["5_64", "2_25", "4_25"])
def test_streaming_is_bitwise(gpu, fs, L, M, sps):
    """pushes of one sample, of fewer than M / L samples (several in a row deliver nothing) and ragged larger pieces equal one push;
    a host block equals a device block; reset restarts the stream; each push delivers the ceil(L N / M) difference"""
    import torch
    blocks = [1, 1, 5, 3, 1, 12, 13, 298, 4097, 1, 2047, 6, 7777]
    n = sum(blocks)
    x = _noise(13, n)
    centres = [-0.4 * fs, 0.09375 * fs, 0.4 * fs]
    with capi.Recc(n_channels=3, sps=sps, max_samples=rr.nout(n, L, M), max_bursts=4) as r:
        r.set_xlate_resampled(fs, centres, L, M)
        whole = r.debug_xlate_shared(x)
        r.reset()
        parts, o = [], 0
        for b in blocks:
            parts.append(r.debug_xlate_shared(x[o:o + b]))
            o += b
        ragged = np.concatenate(parts, axis=1)
        r.reset()
        dev = r.debug_xlate_shared(torch.from_numpy(x).to(gpu))
        r.reset()
        again = r.debug_xlate_shared(x)
    assert whole.shape == (3, rr.nout(n, L, M)) and np.abs(whole).max() > 0
    ends = np.cumsum(blocks)
    counts = [int(rr.nout(e, L, M) - rr.nout(e - b, L, M)) for e, b in zip(ends, blocks)]
    assert [p.shape[1] for p in parts] == counts and 0 in counts
    for name, got in (("ragged", ragged), ("device", dev), ("after reset", again)):
        assert _bits_equal(got, whole), name


# ---- 4. independence of the grid
def test_a_row_does_not_depend_on_the_other_channels(gpu):
    """row c of a five-centre handle (one centre twice) == row 0 of a one-channel handle with centre c"""
    fs, L, M, n = FS2048, 5, 64, 9001
    centres = [-0.9e6, 37.5e3, 0.0, 37.5e3, 0.95e6]
    x = _noise(11, n, 0.5)
    nmax = rr.nout(n, L, M)
    with capi.Recc(n_channels=5, sps=8, max_samples=nmax, max_bursts=4) as r:
        r.set_xlate_resampled(fs, centres, L, M)
        y = r.debug_xlate_shared(x)
    assert y.shape == (5, nmax)
    for c, fc in enumerate(centres):
        with capi.Recc(n_channels=1, sps=8, max_samples=nmax, max_bursts=4) as r:
            r.set_xlate_resampled(fs, [fc], L, M)
            one = r.debug_xlate_shared(x)
        assert _bits_equal(one[0], y[c]), c
    assert _bits_equal(y[1], y[3]) and not _bits_equal(y[1], y[2])


# ---- 5. sample formats
FORMATS = {"sc16": capi.SAMPLES_SC16, "sc8": capi.SAMPLES_SC8, "cu8": capi.SAMPLES_CU8}
CONFIGS = {"2048k_5_64": (FS2048, 5, 64, 8, (-0.9e6, 15e3, 615e3)), "2500k_2_25": (2.5e6, 2, 25, 10, (-615e3, 15e3))}


def _ints(fmt, n, seed=31):
    """[n, 2] random samples over the whole range of the format, both extremes planted in I and in Q"""
    info = np.iinfo(capi.SAMPLE_DTYPES[fmt])
    rng = np.random.default_rng(seed + fmt)
    a = rng.integers(info.min, info.max + 1, size=(n, 2)).astype(capi.SAMPLE_DTYPES[fmt])
    for i, pair in zip((0, 1, 2, 3, 300, 2047, 2048, n - 1),
                       ((info.min, info.max), (info.max, info.min), (info.min, info.min), (info.max, info.max)) * 2):
        a[i % n] = pair
    return a


def _resampled(cfg, n):
    fs, L, M, sps, centres = CONFIGS[cfg]
    r = capi.Recc(n_channels=len(centres), sps=sps, max_samples=rr.nout(n, L, M) + 1, max_bursts=4)
    r.set_xlate_resampled(fs, list(centres), L, M)
    return r


@pytest.mark.parametrize("name,cfg", [("cu8", "2048k_5_64"), ("sc16", "2048k_5_64"), ("sc8", "2500k_2_25")])
def test_integer_blocks_equal_the_fc32_path(gpu, name, cfg):
    """three tiles, the last one partial.  As a host array, as a device tensor, and as a device tensor that starts at an odd sample
    (aligned to one sample only): each the bits of the fc32 call on the converted block"""
    import torch
    fmt = FORMATS[name]
    _, L, M, _, centres = CONFIGS[cfg]
    n = 2 * 64 * M + 301 if L == 5 else 2 * 128 * M + 301
    x = _ints(fmt, n)
    xf = capi.convert_samples(x, fmt)
    t = torch.from_numpy(x).to(gpu)
    with _resampled(cfg, n) as r:
        want = r.debug_xlate_shared(xf)
        r.reset()
        want_odd = r.debug_xlate_shared(xf[1:])
        r.reset()
        host = r.debug_xlate_shared_as(x, fmt)
        r.reset()
        dev = r.debug_xlate_shared_as(t, fmt)
        r.reset()
        odd = r.debug_xlate_shared_as(t[1:], fmt)
    assert want.shape == (len(centres), rr.nout(n, L, M)) and np.abs(want).max() > 0
    assert _bits_equal(host, want), "host block"
    assert _bits_equal(dev, want), "device block"
    assert _bits_equal(odd, want_odd), "device block from an odd sample"


def test_formats_mix_on_one_handle(gpu):
    """seven pushes, each in another format over its own full range: the rows of ONE fc32 push of the converted stream"""
    blocks = [1, 2, 3, 298, 299, 300, 4097]
    order = [capi.SAMPLES_CU8, capi.SAMPLES_FC32, capi.SAMPLES_SC16, capi.SAMPLES_SC8, capi.SAMPLES_CU8, capi.SAMPLES_FC32, capi.SAMPLES_SC16]
    rng = np.random.default_rng(59)
    raw = [(rng.standard_normal((b, 2)) * 1000).astype(np.float32) if f == capi.SAMPLES_FC32 else _ints(f, b, seed=59 + i)
           for i, (f, b) in enumerate(zip(order, blocks))]
    whole = np.concatenate([capi.convert_samples(a, f) for a, f in zip(raw, order)])
    with _resampled("2048k_5_64", whole.size) as r:
        want = r.debug_xlate_shared(whole)
        r.reset()
        parts = [r.debug_xlate_shared_as(a, f) for a, f in zip(raw, order)]
    assert want.shape[1] == rr.nout(whole.size, 5, 64) and np.abs(want).max() > 0
    assert _bits_equal(np.concatenate(parts, axis=1), want)


# ---- 6. decode: 2.048 Msps cu8 x 5/64, eight samples per symbol
CENTRES_2048 = [-0.9e6, -615e3, 15e3, 45e3, 0.93e6]    # two of them adjacent
SEED_2048 = 8100


@functools.lru_cache(maxsize=None)
def _stream2048(s):
    """five mobiles' channels in 0.6 s of a 2.048 Msps stream (102.4 samples per symbol), one burst each, overlapping in time, two of
    the channels adjacent; quantised as an RTL-SDR would: offset binary, 16 per unit amplitude"""
    n = 1228800
    k = np.arange(n)
    x = np.zeros(n, np.complex128)
    truth = []
    for c, fc in enumerate(CENTRES_2048):
        iq, t = synth.make_channel_block(n, 1, seed=s + c, sps=102.4, snr_db=30, first=4000 + 46000 * c)
        x += iq * np.exp(2j * np.pi * fc * k / FS2048)
        truth.append(t)
    v = np.stack([x.real, x.imag], -1) * 16.0
    assert np.abs(v).max() < 127.0
    q = np.floor(v + 128.0).astype(np.uint8)
    q.setflags(write=False)
    return q, truth


def _sent(truth):
    return sorted((c, b[2]) for c, t in enumerate(truth) for b in t)


def test_records_are_those_of_the_iq_seam_and_of_the_model(gpu):
    """tests/test_gpu_xlate_rates.py's six-samples-per-symbol test restated at 5/64: the records of set_xlate_resampled +
    push_raw_shared_as are, byte for byte, those of a plain IQ-seam handle (8 samples per symbol) given the rows a second handle's
    debug_xlate_shared_as makes of the same pushes; every planted MIN comes back; and the CPU model on the float64 helper's output
    decodes the same words."""
    q, truth = _stream2048(SEED_2048)
    sent = _sent(truth)
    assert len(sent) == 5
    starts = sorted(t[0][0] for t in truth)
    assert starts[1] - starts[0] < 3400 * 102.4                      # the bursts overlap in time
    parts = np.array_split(q, 5)
    nmax = rr.nout(q.shape[0], 5, 64)
    with capi.Recc(n_channels=5, sps=8, max_samples=nmax, max_bursts=64) as r:
        r.set_xlate_resampled(FS2048, CENTRES_2048, 5, 64)
        for part in parts:
            r.push_raw_shared_as(part, capi.SAMPLES_CU8)
        got = r.drain()
    with capi.Recc(n_channels=5, sps=8, max_samples=nmax, max_bursts=64) as stage, \
         capi.Recc(n_channels=5, sps=8, max_samples=nmax, max_bursts=64) as plain:
        stage.set_xlate_resampled(FS2048, CENTRES_2048, 5, 64)
        for part in parts:
            rows = stage.debug_xlate_shared_as(part, capi.SAMPLES_CU8)
            if rows.shape[1]:
                plain.push_iq(np.ascontiguousarray(rows))
        want = plain.drain()
    assert got.tobytes() == want.tobytes()
    assert sorted((int(g["channel"]), g["min"].decode()) for g in got) == sent
    model = _model_records(SEED_2048)
    assert sorted((int(m["channel"]), m["min"].decode()) for m in model) == sent
    for m in model:
        g = got[(got["channel"] == m["channel"]) & (got["min"] == m["min"])]
        assert len(g) == 1
        assert np.array_equal(m["word_dec"], g[0]["word_dec"]) and np.array_equal(m["valid"], g[0]["valid"])


@functools.lru_cache(maxsize=None)
def _model_records(s):
    """the CPU chain on the float64 statement of the stage"""
    q, _ = _stream2048(s)
    x = capi.convert_samples(np.asarray(q), capi.SAMPLES_CU8)
    g = rr.design(15.0, 5 * FS2048, 10e3, 4.5e3)
    rows = np.stack([rr.exact(x, g, fc, FS2048, 5, 64).astype(np.complex64) for fc in CENTRES_2048])
    return oracle.fused_push_all(rows, sps=8)


# ---- 7. errors
def test_errors(gpu):
    L = capi.load()
    cen = (capi.C.c_double * 2)(-60e3, 60e3)

    def cfg(interp=5, decim=64, rate=FS2048, width=0.0, cutoff=0.0, centers=cen, n=2, size=None):
        return capi.XlateResampleCfg(capi.C.sizeof(capi.XlateResampleCfg) if size is None else size, interp, decim, n, 0, rate, 0.0, cutoff, width, centers)

    def rc(r, x):
        return L.amps_recc_set_xlate_resampled(r._h, capi.C.byref(x) if x is not None else None)

    def shared(r, decim, rate):
        x = capi.XlateSharedCfg(capi.C.sizeof(capi.XlateSharedCfg), decim, 2, 0, rate, 0.0, 0.0, 0.0, cen)
        return L.amps_recc_set_xlate_shared(r._h, capi.C.byref(x))

    x = _noise(17, 6400, 0.5)
    z = np.zeros(64, np.complex64)
    with capi.Recc(n_channels=2, sps=8, max_samples=500, max_bursts=4) as r:
        assert L.amps_recc_set_xlate_resampled(None, capi.C.byref(cfg())) == -errno.EINVAL
        assert rc(r, None) == -errno.EINVAL
        assert rc(r, cfg(size=56)) == -errno.EINVAL
        assert rc(r, cfg(n=3)) == -errno.EINVAL
        assert rc(r, cfg(centers=None)) == -errno.EINVAL
        for interp, decim in ((1, 12), (6, 77), (0, 64), (5, 5), (5, 4), (5, 65), (4, 50), (2, 32)):
            # outside 2 ... 5, decim <= interp, decim > 64, a common factor: each at a rate that would match
            assert rc(r, cfg(interp, decim, 160e3 * decim / max(interp, 1))) == -errno.EINVAL, (interp, decim)
        assert rc(r, cfg(5, 64, 2.0e6)) == -errno.EINVAL             # 156.25 ksps is not 8 samples per symbol
        assert rc(r, cfg(2, 25, 2.5e6)) == -errno.EINVAL             # 200 ksps is 10 samples per symbol, not this handle's 8
        assert rc(r, cfg(centers=(capi.C.c_double * 2)(0.0, FS2048 + 1.0))) == -errno.EINVAL   # a centre beyond the rate
        assert rc(r, cfg(centers=(capi.C.c_double * 2)(0.0, float("nan")))) == -errno.EINVAL
        assert rc(r, cfg(width=74 * 5 * FS2048 / 44 * 1.0001)) == -errno.EINVAL   # one tap: no filter
        assert rc(r, cfg(cutoff=2.5 * FS2048 + 1.0)) == -errno.EINVAL         # beyond half the up-sampled rate
        assert rc(r, cfg(width=2.8e3)) == -errno.E2BIG               # 2461 taps per phase
        assert rc(r, cfg(width=3.6e3)) == -errno.E2BIG               # 1914: five tap sets and the window are beyond the LDS
        assert L.amps_recc_push_raw_shared(r._h, capi._hostptr(z), 16, capi.MEM_HOST) == -errno.ENOSYS   # nothing was configured
        # a refused configuration leaves the stage as it was
        assert rc(r, cfg()) == 0
        before = r.debug_xlate_shared(x)
        for bad in (cfg(6, 77, 160e3 * 77 / 6), cfg(5, 64, 2.0e6), cfg(width=2.8e3), cfg(n=3)):
            assert rc(r, bad) < 0
        r.reset()
        assert _bits_equal(r.debug_xlate_shared(x), before) and before.shape == (2, 500) and np.abs(before).max() > 0
        # the limit of one push: 500 outputs are 6400 inputs from the stream's start; one more input is one more output
        r.reset()
        big = np.zeros(6401, np.complex64)
        assert L.amps_recc_push_raw_shared(r._h, capi._hostptr(big), 6400, capi.MEM_HOST) == 0
        r.reset()
        assert L.amps_recc_push_raw_shared(r._h, capi._hostptr(big), 6401, capi.MEM_HOST) == -errno.E2BIG
        assert L.amps_recc_push_raw_shared(r._h, capi._hostptr(big), 6400, capi.MEM_HOST) == 0            # and refusing consumed nothing
        # the three forms exclude each other
        assert L.amps_recc_push_raw(r._h, capi._hostptr(z), 8, 8, capi.MEM_HOST) == -errno.ENOSYS
        assert shared(r, 0, 0.0) == 0                                 # removes the integer shared form only: not this one
        assert L.amps_recc_push_raw_shared(r._h, capi._hostptr(z), 16, capi.MEM_HOST) == 0
        assert shared(r, 10, 1.6e6) == 0                              # 1.6 Msps / 10: the integer shared form replaces it
        r.reset()
        assert r.debug_xlate_shared(x[:5000]).shape == (2, 500)
        assert rc(r, cfg(decim=0)) == 0                               # removes the rational form only: not that one
        assert L.amps_recc_push_raw_shared(r._h, capi._hostptr(z), 16, capi.MEM_HOST) == 0
        assert rc(r, cfg()) == 0                                      # and back
        r.reset()
        assert _bits_equal(r.debug_xlate_shared(x), before)
        one = capi.XlateCfg(capi.C.sizeof(capi.XlateCfg), 2, 320e3, 15e3, 0.0, 0.0, 0.0)
        assert L.amps_recc_set_xlate(r._h, capi.C.byref(one)) == 0     # the per-row form replaces it
        assert L.amps_recc_push_raw_shared(r._h, capi._hostptr(z), 16, capi.MEM_HOST) == -errno.ENOSYS
        assert rc(r, cfg()) == 0
        assert L.amps_recc_push_raw(r._h, capi._hostptr(z), 8, 8, capi.MEM_HOST) == -errno.ENOSYS
        assert rc(r, cfg(decim=0)) == 0
        assert L.amps_recc_push_raw_shared(r._h, capi._hostptr(z), 16, capi.MEM_HOST) == -errno.ENOSYS
    # -ENOSYS: a handle without the IQ seam, and a channel-group handle
    with capi.Recc(n_channels=2, max_bursts=4) as r:
        assert rc(r, cfg()) == -errno.ENOSYS
    wb = {"channels": 1024, "decim": 512, "taps_per_branch": 8, "first_channel": 96, "groups": 2, "group": 0}
    with capi.Recc(n_channels=832, sps=3, max_samples=64 + 72, max_bursts=4, wideband=wb) as r:
        many = (capi.C.c_double * 832)()
        assert rc(r, cfg(3, 50, 1.0e6, n=832, centers=many)) == -errno.ENOSYS


# ---- 8. recctest sub and the example
def _bits(a):
    return "".join(str(int(b)) for b in a)


def _expected_lines(records):
    """what recc_decode publishes for these records, as recctest prints it (tests/test_gpu_host_blocks.py)"""
    lines = []
    for rec in records:
        r = oracle.reply_words(rec)
        if r.has_focc:
            lines.append(f"MSG focc_words stream={r.focc_stream} n={r.focc_nwords} w1={_bits(r.focc_word1)} w2={_bits(r.focc_word2)}")
        if r.has_fvc:
            lines.append(f"MSG fvc_words n={r.fvc_count} w1={_bits(r.fvc_word1)} repeat={r.fvc_repeat}")
        if r.has_mutes:
            lines.append(f"MSG fvc_mute {r.fvc_mute}")
            lines.append(f"MSG audio_mute {r.audio_mute}")
        if r.has_command:
            lines.append("MSG command_out " + r.command.decode())
    return lines


def test_recctest_sub_at_the_rtl_sdr_default_rate(gpu, tmp_path):
    """gr::amps::recc_subband through `recctest sub capture.cu8 <chunk> 2048000 5/64 <centres>`: the five-channel stream in ragged
    work() calls; per channel the lines of the bursts the binding returns for the same samples, in order"""
    q, truth = _stream2048(SEED_2048)
    with capi.Recc(n_channels=5, sps=8, max_samples=rr.nout(q.shape[0], 5, 64), max_bursts=64) as r:
        r.set_xlate_resampled(FS2048, CENTRES_2048, 5, 64)
        for part in np.array_split(q, 5):
            r.push_raw_shared_as(part, capi.SAMPLES_CU8)
        recs = r.drain()
    assert sorted((int(g["channel"]), g["min"].decode()) for g in recs) == _sent(truth)
    p = tmp_path / "capture.cu8"
    np.asarray(q).tofile(p)
    _, exe = build_host()
    out = subprocess.run([exe, "sub", str(p), "777777", "2048000", "5/64", ",".join("%g" % c for c in CENTRES_2048)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got, ch = {}, None
    for line in out.stdout.splitlines():
        if line.startswith("MSG channel "):
            ch = int(line.split()[2])
            got.setdefault(ch, [])
        elif line.startswith("MSG "):
            got[ch].append(line)
    want = {c: _expected_lines(recs[recs["channel"] == c]) for c in range(5)}
    assert got == want and all(len(v) >= 1 for v in want.values())      # one burst a channel: every channel prints
    assert sum(out.stdout.count("MSG channel %d\n" % c) for c in range(5)) == len(recs) == 5


def test_example_decodes_both_systems_from_one_2048_ksps_stream(gpu):
    """examples/decode_subband.py --rtl2048: the 42 control channels of both systems from one 2.048 Msps cu8 stream at 5/64"""
    script = os.path.join(ROOT, "examples", "decode_subband.py")
    p = subprocess.run([sys.executable, script, "--rtl2048"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert "42 bursts sent, 42 decoded" in p.stdout and "MISMATCH" not in p.stdout
    assert p.stdout.count("  MIN ") == 42
