"""-m gpu: the slicers of include/amps_recc_numerics.h on degenerate sample VALUES (tests/valuecases.py): integer lattices with signed
zeros, axis walks, runs of exact zeros, constant streams, power-of-two scales from subnormal products to |x| just below 2^60, and
non-finite poison.  Everywhere else in the suite the inputs are Gaussian noise plus FM bursts, on which a tie, an exact or negative
zero, an antipodal phase step or a subnormal product never happens -- and it is there that a negation folded into an fma operand, a
packed multiply under another denormal mode, a max / min against the floor or a sign bit taken from -0 would show.

  (a) IQ seam taps (amps_recc_debug_demod): g bit for bit, d and S as uint32, against the CPU model; on the integer-valued classes
      also against tests/valueref.py, a float64 statement that shares nothing with the model's C;
  (b) a block whose rows are the classes, pushed in one piece and raggedly: the bit ring equals the model;
  (c) records: a burst, an exact-zero gap, the burst at 2^-40 and at 2^+40;
  (d) device against device: a power-of-two scale changes no bit and scales the reported power exactly, on the IQ, translate and
      wideband seams;
  (e) an exact-zero gap through the fused filter bank;
  (f) NaN / Inf / FLT_MAX are outside the contract: what is promised is containment (sps samples, no other row)."""
import numpy as np
import pytest

import oracle
import valuecases as vc
import valueref as vr
from gr_amps_amd import capi, synth, synth_wideband as sw
from conftest import wb_cfg

pytestmark = pytest.mark.gpu

SPECS = [("atan", 0), ("product", 1), ("sine", 2), ("exact", 3)]
BCD = SPECS[1:]
ALL_SPS = [3, 4, 5, 6, 8, 10, 12]
N = vc.ROW
RAGGED = [1, 63, 777, 4096, 500, 500, 500, 500, 500, 500, 255]
assert sum(RAGGED) == N

_cache = {}


def _classes(sps):
    if ("cls", sps) not in _cache:
        cls = vc.classes(sps, N)
        for rows in cls.values():
            for row in rows.values():
                row.setflags(write=False)
        _cache[("cls", sps)] = cls
    return _cache[("cls", sps)]


def _model(x, sps, sid):
    f = oracle.Fused(0, sps, slicer=sid)
    f.push(x)
    return f.taps()


def _first(a, b):
    return np.nonzero(a != b)[0][:8].tolist()


@pytest.fixture(scope="module")
def tap_handle(gpu):
    """one single-channel handle per (spec, sps): amps_recc_debug_demod resets it before and after every call"""
    held = {}

    def get(spec, sps):
        if (spec, sps) not in held:
            held[(spec, sps)] = capi.Recc(n_channels=1, sps=sps, max_samples=N, max_bursts=8, slicer=spec)
        return held[(spec, sps)]
    yield get
    for r in held.values():
        r.close()


# ---- (a) the IQ seam's taps
@pytest.mark.parametrize("cls", ["V1", "V2", "V3", "V4", "V5"])
@pytest.mark.parametrize("sps", ALL_SPS)
@pytest.mark.parametrize("spec,sid", SPECS)
def test_iq_seam_taps_equal_the_model_and_the_float64_statement(gpu, tap_handle, spec, sid, sps, cls):
    r = tap_handle(spec, sps)
    for name, x in _classes(sps)[cls].items():
        d, S, g = r.debug_demod(x)
        md, mS, mg = _model(x, sps, sid)
        assert len(g) == len(mg) == N
        nd, nS, ng = int((vr.u32(d) != vr.u32(md)).sum()), int((vr.u32(S) != vr.u32(mS)).sum()), int((g != mg).sum())
        print("\n%s %s sps %d spec %s: %d bits, %d d words, %d S words differ from the model" % (cls, name, sps, spec, ng, nd, nS))
        assert ng == 0, (name, _first(g, mg))
        assert nS == 0, (name, _first(vr.u32(S), vr.u32(mS)))
        assert nd == 0, (name, _first(vr.u32(d), vr.u32(md)))
        if cls in vc.EXACT_CLASSES:
            if sid == 0:
                vr.check_spec_a(x, sps, d, S, g)
            else:
                wd, wS, wg = vr.taps32(x, sps, sid)
                assert np.array_equal(g, wg), (name, _first(g, wg))
                assert np.array_equal(vr.u32(S), wS), (name, _first(vr.u32(S), wS))
                assert np.array_equal(vr.u32(d), wd), (name, _first(vr.u32(d), wd))


# ---- (b) rows and pushes
def _straddled(runs, cuts):
    return sorted({(s, L) for c in cuts for s, L in runs if s < c < s + L})


@pytest.mark.parametrize("sps", [3, 10])
@pytest.mark.parametrize("spec,sid", SPECS)
def test_iq_seam_rows_of_every_class_one_shot_and_ragged(gpu, spec, sid, sps):
    rows = [(cls, name, x) for cls, d in _classes(sps).items() for name, x in d.items()]
    block = np.stack([x for _, _, x in rows])
    cuts = np.cumsum(RAGGED)[:-1]
    for kw in ({}, {"negative": True}, {"leading": True}):            # the schedule cuts zero runs in every V3 row
        assert len(_straddled(vc.zero_runs(sps, N, **kw)[1], cuts)) >= 3
    with capi.Recc(n_channels=len(rows), sps=sps, max_samples=N, max_bursts=16, slicer=spec) as r:
        r.push_iq(block)
        one, produced = r.debug_slicer_bits(0, N)
        assert produced == N and len(r.drain()) == 0
    with capi.Recc(n_channels=len(rows), sps=sps, max_samples=N, max_bursts=16, slicer=spec) as r:
        off = 0
        for m in RAGGED:
            r.push_iq(np.ascontiguousarray(block[:, off:off + m]))
            off += m
        many, produced = r.debug_slicer_bits(0, N)
        assert produced == N and len(r.drain()) == 0
    for i, (cls, name, x) in enumerate(rows):
        mg = _model(x, sps, sid)[2]
        assert np.array_equal(one[i], mg), (cls, name, _first(one[i], mg))
        assert np.array_equal(many[i], one[i]), (cls, name, _first(many[i], one[i]))


# ---- (c) records among garbage
@pytest.mark.parametrize("sps", [10, 3])
@pytest.mark.parametrize("spec,sid", [("default", None), ("atan", 0)])
def test_records_of_a_burst_a_zero_gap_and_the_burst_at_two_scales(gpu, spec, sid, sps):
    n1, C = 3456 * sps + 5000, 2
    rows, mins = [], []
    for c in range(C):
        x, truth = synth.make_channel_block(n1, 1, seed=4100 + 10 * sps + c, sps=sps, snr_db=30.0)
        assert len(truth) == 1
        gap = np.zeros(1000 + sps + 37 * c, np.complex64)
        tail = np.zeros(64 + 37 * (C - 1 - c), np.complex64)          # rows of one length; the stream ends in exact zeros too
        rows.append(np.concatenate([x, gap, vc.scaled(x, -40), vc.scaled(x, 40), tail]))
        mins.append(truth[0][2])
    block = np.stack(rows)
    with capi.Recc(n_channels=C, sps=sps, max_samples=block.shape[1], max_bursts=64, slicer=spec) as r:
        r.push_iq(block)
        got = r.drain()
    want = oracle.fused_push_all(block, sps=sps, slicer=sid)
    assert len(want) == 3 * C
    assert got.tobytes() == want.tobytes()
    for c in range(C):
        mine = got[got["channel"] == c]
        assert len(mine) == 3 and all(g["min"].decode() == mins[c] and g["valid"].all() for g in mine)


# ---- (d) power-of-two invariance: device against device
def _same_mantissa_shifted_exponent(P, P0, k):
    """P == 4^k P0 exactly: the mantissas are equal and the exponents differ by 2 k"""
    m, e = np.frexp(P)
    m0, e0 = np.frexp(P0)
    assert P0.size and (P0 > 0).all() and np.isfinite(P).all()
    assert np.array_equal(m, m0) and np.array_equal(e, e0 + 2 * k), k


@pytest.mark.parametrize("sps", [3, 10])
@pytest.mark.parametrize("spec,sid", BCD)
def test_iq_seam_bits_and_power_do_not_depend_on_a_power_of_two_scale(gpu, spec, sid, sps):
    ks = [0, -50, -20, 20, 50]
    rows = _classes(sps)["V5"]
    block = np.stack([rows["2^%d" % k] for k in ks])
    with capi.Recc(n_channels=len(ks), sps=sps, max_samples=N, max_bursts=16, slicer=spec, stream_power=True) as r:
        r.push_iq(block)
        bits, produced = r.debug_slicer_bits(0, N)
        P, first = r.channel_power()
    assert produced == N and first == 0 and P.shape == (len(ks), N // 256)
    assert 0.2 < bits[0].mean() < 0.8
    for i, k in enumerate(ks[1:], 1):
        assert np.array_equal(bits[i], bits[0]), (k, _first(bits[i], bits[0]))
        _same_mantissa_shifted_exponent(P[i], P[0], k)


@pytest.mark.parametrize("sps", [3, 10])
def test_iq_seam_spec_a_bits_at_two_scales(gpu, sps):
    """spec A floors max(|re|, |im|) at 2^-100, so it is scale-free only where the scaled conj-product stays above the floor: the
    samples whose unscaled max(|re|, |im|), in float64, exceeds 2^-50 (every window of them, for a bit) -- nearly all"""
    ks = [0, -20, 20]
    rows = _classes(sps)["V5"]
    block = np.stack([rows["2^%d" % k] for k in ks])
    x = rows["2^0"].astype(np.complex128)
    t = x * np.conj(np.concatenate([[0], x[:-1]]))
    big = np.maximum(np.abs(t.real), np.abs(t.imag)) > 2.0 ** -50
    keep = np.convolve(~big, np.ones(sps), "full")[:N] == 0          # no small product among the sps samples that end here
    keep[:sps] = False                                               # (the first product has no partner: it is zero)
    assert keep.mean() > 0.99
    with capi.Recc(n_channels=len(ks), sps=sps, max_samples=N, max_bursts=16, slicer="atan") as r:
        r.push_iq(block)
        bits, produced = r.debug_slicer_bits(0, N)
    assert produced == N
    for i, k in enumerate(ks[1:], 1):
        assert np.array_equal(bits[i][keep], bits[0][keep]), (k, _first(bits[i][keep], bits[0][keep]))


@pytest.mark.parametrize("spec,sid", BCD)
def test_translate_seam_bits_and_power_do_not_depend_on_a_power_of_two_scale(gpu, spec, sid):
    """a power-of-two scale of a float block is exact through the mixer and the FIR (no under- or overflow at 2^+-20)"""
    ks, sps, n = [0, -20, 20], 10, 20000
    base = np.repeat(vc.carrier_row(n // 2, sps, seed=6), 2)
    block = np.stack([vc.scaled(base, k) for k in ks])
    with capi.Recc(n_channels=len(ks), sps=sps, max_samples=n // 2, max_bursts=16, slicer=spec, stream_power=True) as r:
        r.set_xlate(rate_hz=400e3, center_hz=37.5e3, decim=2)
        r.push_raw(block)
        produced = r.debug_slicer_bits(0, 0)[1]
        bits, _ = r.debug_slicer_bits(0, produced)
        P, first = r.channel_power()
    assert produced >= 9000 and first == 0 and P.shape == (len(ks), produced // 256)
    assert 0.2 < bits[0].mean() < 0.8
    for i, k in enumerate(ks[1:], 1):
        assert np.array_equal(bits[i], bits[0]), (k, _first(bits[i], bits[0]))
        _same_mantissa_shifted_exponent(P[i], P[0], k)


WB_FIRST, WB_C = 200, 64


def _wb_handle(D, frames, **kw):
    wb, sps = wb_cfg(D, WB_FIRST)
    return capi.Recc(n_channels=WB_C, sps=sps, max_samples=frames + 72, max_bursts=16, wideband=wb, **kw)


def _wb_noise(D, frames, seed):
    if ("wb", D, frames, seed) not in _cache:
        x = sw.make_wideband(frames * D, [], seed=seed)[0]
        x.setflags(write=False)
        _cache[("wb", D, frames, seed)] = x
    return _cache[("wb", D, frames, seed)]


@pytest.mark.parametrize("spec,sid", BCD)
def test_wideband_seam_bits_and_power_do_not_depend_on_a_power_of_two_scale(gpu, decim, spec, sid):
    """... and through the filter bank's fold and FFT"""
    D, frames = decim, 200
    x = _wb_noise(D, frames, 8)                                       # 200 frames: 192 consumed, one power snapshot (frame 0)
    out = {}
    for k in (0, -20, 20):
        with _wb_handle(D, frames, slicer=spec, channel_power=True) as r:
            r.push_wideband(vc.scaled(x, k))
            produced = r.debug_slicer_bits(0, 0)[1]
            out[k] = (r.debug_slicer_bits(0, produced)[0], r.channel_power()[0])
    bits0, P0 = out[0]
    assert bits0.shape == (WB_C, frames // 64 * 64) and 0.2 < bits0.mean() < 0.8 and P0.shape[1] >= 1
    for k in (-20, 20):
        rows, at = np.nonzero(out[k][0] != bits0)
        assert rows.size == 0, (k, rows.size, list(zip(rows[:8].tolist(), at[:8].tolist())))
        _same_mantissa_shifted_exponent(out[k][1], P0, k)


# ---- (e) an exact-zero gap through the filter bank
@pytest.mark.parametrize("spec,sid", SPECS)
def test_wideband_seam_zero_gap(gpu, decim, spec, sid):
    """the gap is longer than the 8192-tap prototype plus 20 frames: at least 20 frames come out exactly zero in every channel; the fused
    bank's bits equal the model run on the IQ form's output (as in tests/test_gpu_wideband_bits.py) -- if the two forms disagreed in
    the SIGN of those zeros, the bits of specs B, C and D would show it"""
    D, frames, sps = decim, 400, 1536 // decim
    if ("gap", D) not in _cache:
        x = _wb_noise(D, frames, 9).copy()
        x[100 * D:100 * D + 12288 + 20 * D] = 0
        with _wb_handle(D, frames) as r:
            chan = r.debug_channelize(x)
        _cache[("gap", D)] = (x, chan)
    x, chan = _cache[("gap", D)]
    v = chan.view(np.float32).reshape(WB_C, -1, 2)
    zero = (v == 0).all(axis=(0, 2))                                  # frames that are +-0 in every channel, both parts
    zf = np.nonzero(zero)[0]
    assert len(zf) >= 20 and zf[-1] - zf[0] + 1 == len(zf), zf        # one contiguous stretch
    assert 100 <= zf[0] and zf[-1] <= 100 + 12288 // D + 20 + 2
    assert np.isfinite(v).all()
    with _wb_handle(D, frames, slicer=spec) as r:
        r.push_wideband(x)
        produced = r.debug_slicer_bits(0, 0)[1]
        bits = r.debug_slicer_bits(0, produced)[0]
    assert produced == frames // 64 * 64 and produced > zf[-1] + 20
    for row in range(WB_C):
        mg = _model(chan[row], sps, sid)[2][:produced]
        assert np.array_equal(bits[row], mg), (row, _first(bits[row], mg))


# ---- (f) containment of out-of-contract values
P_START, P_LEN = 1000, 100


def _poison_block(sps):
    if ("poison", sps) not in _cache:
        n = 3456 * sps + 5000
        rows = [synth.make_channel_block(n, 1, seed=4300 + 10 * sps + c, sps=sps, snr_db=30.0) for c in range(3)]
        assert all(len(t) == 1 and t[0][0] > P_START + P_LEN + 74 * sps for _, t in rows)       # the stretch lies in the quiet part
        block = np.stack([x for x, _ in rows])
        block.setflags(write=False)
        _cache[("poison", sps)] = block
    return _cache[("poison", sps)]


def _bits_and_records(block, sps, spec):
    n = block.shape[1]
    with capi.Recc(n_channels=block.shape[0], sps=sps, max_samples=n, max_bursts=16, slicer=spec) as r:
        r.push_iq(block)
        bits, produced = r.debug_slicer_bits(0, n // 64 * 64)
        return bits, r.drain()


@pytest.mark.parametrize("kind", sorted(vc.POISON))
@pytest.mark.parametrize("sps", [3, 10])
@pytest.mark.parametrize("spec,sid", SPECS)
def test_non_finite_samples_are_contained(gpu, spec, sid, sps, kind):
    """100 samples of NaN, of +-Inf or of +-FLT_MAX (whose products overflow) in the quiet part of row 1 -- shorter than a trigger:
    rows 0 and 2 are untouched, row 1's bits are those of the clean run from sps + 1 samples behind the stretch on, and every record
    is the clean run's.  Nothing is asserted about the bits inside the stretch."""
    clean = _poison_block(sps)
    assert P_LEN < 74 * sps
    if ("clean", sps, spec) not in _cache:
        _cache[("clean", sps, spec)] = _bits_and_records(clean, sps, spec)
    bits0, rec0 = _cache[("clean", sps, spec)]
    assert len(rec0) == 3 and sorted(rec0["channel"]) == [0, 1, 2]
    dirty = clean.copy()
    dirty[1] = vc.poison(clean[1], kind, P_START, P_LEN)
    bits, rec = _bits_and_records(dirty, sps, spec)
    for row in (0, 2):
        assert np.array_equal(bits[row], bits0[row]), (row, _first(bits[row], bits0[row]))
    assert np.array_equal(bits[1, :P_START], bits0[1, :P_START])
    end = P_START + P_LEN
    assert np.array_equal(bits[1, end + sps + 1:], bits0[1, end + sps + 1:]), _first(bits[1, end + sps + 1:], bits0[1, end + sps + 1:])
    assert rec.tobytes() == rec0.tobytes()
