"""-m gpu: the fused filter bank's slicer bits, read frame by frame through amps_recc_debug_slicer_bits (the bit ring), for every
channel of a wrapped 832-channel band -- instead of only through the records decoded from a few thousand of them.

  (a) bit for bit against the CPU model (oracle.Fused) run on the IQ form's output of the same block, one-shot and ragged;
  (b) against the float64 statement of each slicer spec (tests/slicerbound.py) on the float64 filter-bank model, within an explicit
      perturbation bound built from the row's own channelizer error;
  (c) the same bits from the two-kernel form, from channel-group handles, after set_origin and after reset.
Every test runs at both decimations (conftest.py: `decim`) and, where it has the parameter, for all four slicer specs."""
import errno

import numpy as np
import pytest

import oracle
import slicerbound as sb
from oracle import channelizer as cz
from gr_amps_amd import capi, synth, synth_wideband as sw
from conftest import wb_cfg

pytestmark = pytest.mark.gpu

FIRST, C, M = 700, 832, 1024        # bins 700 .. 1023, 0 .. 507: the band wraps past bin 1023
NFR = 4500                          # frames in the block: a one-shot push consumes 4480 (70 workgroups of 64 frames on 256 CUs)
SPECS = [("atan", 0), ("product", 1), ("sine", 2), ("exact", 3)]
# rows with a burst: the band's first and last, the two around the wrap (bins 1023 and 0), two interior ones
BURST_ROWS = (0, C - 1, (1023 - FIRST) % M, (0 - FIRST) % M, 100, 600)
BURST_FRAMES = (80, 600, 1200, 2000, 2800, 3500)
# the ragged schedule: pushes of whole frames plus odd samples.  Produced frames after each push: 0, 64 (1 frame left in the carry),
# 128 (33 left), 192 (63 left), 256 (a push of less than one frame completes 64), 320 (exactly 64 frames pushed), 4416 (one launch of
# 4096 frames = 64 workgroups: carry written in-kernel), 4480 (one workgroup: carry written by the copy kernel)
RAGGED = lambda D: [10 * D + 100, 55 * D - 93, 96 * D, 94 * D + 500, D - 504, 64 * D, 4100 * D, None]
L_TAPS = 8 * M
EXPLAINED_FRAC = 1e-3   # differences from the float64 statement that the bound explains: at most this fraction of all bits

_cache = {}


def _handle(D, max_frames=NFR + 72, **kw):
    wb, sps = wb_cfg(D, FIRST, groups=kw.pop("groups", 0), group=kw.pop("group", 0))
    return capi.Recc(n_channels=C, sps=sps, max_samples=max_frames, max_bursts=64, wideband=wb, **kw)


def _block(D):
    """the stream: noise in every channel, bursts at 30 dB in six of them (cut by the block's end), its IQ-form and float64 frames"""
    if ("block", D) not in _cache:
        n = NFR * D + 333
        bursts = [((FIRST + r) % M, f * D + 17 * i) for i, (r, f) in enumerate(zip(BURST_ROWS, BURST_FRAMES))]
        x, truth = sw.make_wideband(n, bursts, seed=77)
        assert len(truth) == len(bursts)
        with _handle(D) as r:
            chan = r.debug_channelize(x)
        y64 = cz.channelize(x, P=8, D=D)                                   # float64, all 1024 bins
        norm = np.sqrt((np.abs(y64) ** 2).sum(0))                          # ||Y64(frame)||_2
        rows = (FIRST + np.arange(C)) % M
        _cache[("block", D)] = (x, bursts, chan, y64[rows], norm)
    return _cache[("block", D)]


def _bits(r, first=0, n=None):
    """all bits the handle has produced from `first` on, and `produced`"""
    if n is None:
        n = r.debug_slicer_bits(0, 0)[1] - first
    return r.debug_slicer_bits(first, n)


def _oneshot(D, spec):
    if ("one", D, spec) not in _cache:
        x = _block(D)[0]
        with _handle(D, slicer=spec) as r:
            r.push_wideband(x)
            _cache[("one", D, spec)] = _bits(r)
    return _cache[("one", D, spec)]


def _model(D, sid):
    if ("model", D, sid) not in _cache:
        chan = _block(D)[2]
        out = []
        for row in range(C):
            f = oracle.Fused(row, 1536 // D, slicer=sid)
            f.push(chan[row])
            out.append(f.taps()[2])
        _cache[("model", D, sid)] = np.stack(out)
    return _cache[("model", D, sid)]


def _first_mismatches(a, b, k=8):
    r, f = np.nonzero(a != b)
    return list(zip(r[:k].tolist(), f[:k].tolist())), r.size


@pytest.mark.parametrize("spec,sid", SPECS)
def test_fused_bits_equal_the_cpu_model_every_channel_and_frame(gpu, decim, spec, sid):
    D = decim
    x = _block(D)[0]
    bits, produced = _oneshot(D, spec)
    assert produced == (len(x) // D) & ~63 and produced // 64 >= 65          # one launch of >= 64 workgroups: carry in-kernel
    assert bits.shape == (C, produced)
    model = _model(D, sid)
    assert model.shape[1] >= produced
    where, count = _first_mismatches(bits, model[:, :produced])
    assert count == 0, (count, where)
    # the stream start is covered: specs B and D slice ones while no partner exists
    if sid in (1, 3):
        assert bits[:, :1536 // D].all()


@pytest.mark.parametrize("spec,sid", SPECS)
def test_fused_bits_ragged_pushes_equal_one_shot(gpu, decim, spec, sid):
    D = decim
    x = _block(D)[0]
    one, produced_one = _oneshot(D, spec)
    parts, off, prev, lefts, deltas = [], 0, 0, [], []
    with _handle(D, slicer=spec) as r:
        for m in RAGGED(D):
            m = len(x) - off if m is None else m
            r.push_wideband(x[off:off + m])
            off += m
            frames = off // D
            bits, produced = r.debug_slicer_bits(prev, 0)
            assert produced == frames & ~63, (off, produced)           # the fused form produces whole 64-frame words only
            bits, produced = r.debug_slicer_bits(prev, produced - prev)
            assert bits.shape == (C, produced - prev)
            parts.append(bits)
            lefts.append(frames - produced)
            deltas.append((m, produced - prev))
            with pytest.raises(capi.AmpsError) as e:                    # the next sample is not produced yet
                r.debug_slicer_bits(produced, 1)
            assert e.value.code == -errno.ERANGE
            prev = produced
    assert off == len(x)
    # the schedule has what it claims: a push that produces nothing, carries of 1, 33 and 63 frames, a push of exactly 64 frames,
    # a 64-workgroup launch (4096 frames) beside one-workgroup launches
    assert deltas[0][1] == 0 and {1, 33, 63} <= set(lefts) and (64 * D, 64) in deltas
    assert max(d for _, d in deltas) >= 4096 and min(d for _, d in deltas[1:]) == 64
    many = np.concatenate(parts, axis=1)
    assert prev == produced_one and many.shape == one.shape
    where, count = _first_mismatches(many, one)
    assert count == 0, (count, where)


@pytest.mark.parametrize("spec,sid", SPECS)
def test_fused_bits_against_the_float64_statement(gpu, decim, spec, sid):
    D = decim
    sps = 1536 // D
    x, bursts, chan, y64, norm = _block(D)
    bits, produced = _oneshot(D, spec)
    y32 = chan[:, :produced].astype(np.complex128)
    y64 = y64[:, :produced]
    err = np.abs(y32 - y64)
    # the filter bank's own error stays inside the fixed per-frame bound: a broken bank cannot widen its own tolerance
    lim = sb.FFT_C * sb.U32 * np.log2(M) * norm[:produced]
    assert (err <= lim).all(), (err / lim).max()
    explained = 0
    for row in range(C):
        eps = err[row].max()
        bad, ex = sb.unexplained(bits[row], y64[row], eps, sps, sid)
        assert bad.size == 0, (row, bad[:8].tolist(), sb.statistic(y64[row], sps, sid)[bad[:8]].tolist())
        explained += ex
    assert explained <= EXPLAINED_FRAC * bits.size, explained
    # inside every burst (30 dB, carrier on from the filter's full overlap on) no bit differs at all
    for k, off in bursts:
        row = (k - FIRST) % M
        assert len(x) - off < 3374 * 1536                     # a burst is longer than the block: it runs to the block's end
        lo = (off + L_TAPS) // D + 1 + sps
        want = sb.float64_bits(y64[row], sps, sid)
        d = np.nonzero(bits[row, lo:] != want[lo:])[0]
        assert d.size == 0, (row, (d[:8] + lo).tolist())
    print(f"\nD={D} spec {spec}: eps/bound max {(err / lim).max():.3f}, explained differences {explained} of {bits.size}")


@pytest.mark.parametrize("spec,sid", SPECS)
def test_two_kernel_form_gives_the_fused_bits(gpu, decim, spec, sid):
    """AMPS_RECC_FLAG_UNFUSED_WIDEBAND: the IQ-form bank, then the streaming kernel at 2 (3) samples per symbol.  It holds back other
    frames than the fused form (a multiple of 4 / 2 in the bank's carry, the rest in the streaming kernel's); both sides agree on
    every sample both have produced, after every push"""
    D = decim
    x = _block(D)[0]
    one, produced_one = _oneshot(D, spec)
    off, prev = 0, 0
    with _handle(D, slicer=spec, unfused_wideband=True) as r:
        for m in RAGGED(D):
            m = len(x) - off if m is None else m
            r.push_wideband(x[off:off + m])
            off += m
            produced = r.debug_slicer_bits(0, 0)[1]
            assert produced == (off // D) & ~63, (off, produced)       # whole 64-sample words of what the bank has delivered
            if produced > prev:
                bits, _ = r.debug_slicer_bits(prev, min(produced, produced_one) - prev)
                where, count = _first_mismatches(bits, one[:, prev:min(produced, produced_one)])
                assert count == 0, (off, count, where)
                prev = min(produced, produced_one)
    assert prev == produced_one


@pytest.mark.parametrize("G", [2, 4, 8])
@pytest.mark.parametrize("spec,sid", SPECS)
def test_channel_group_rows_are_the_whole_band_rows(gpu, decim, spec, sid, G):
    D = decim
    x = _block(D)[0]
    whole, produced = _oneshot(D, spec)
    seen = np.zeros(C, int)
    for g in range(G):
        rows = [c for c in range(C) if (((FIRST + c) % M) & 63) // (64 // G) == g]      # chz_rows: row i = the i-th channel of the group
        with _handle(D, slicer=spec, groups=G, group=g) as r:
            r.push_wideband(x)
            bits, p = _bits(r)
        assert p == produced and bits.shape == (len(rows), produced), (g, bits.shape)
        where, count = _first_mismatches(bits, whole[rows])
        assert count == 0, (g, count, where)
        seen[rows] += 1
    assert (seen == 1).all()


@pytest.mark.parametrize("spec,sid", SPECS)
def test_origin_shifts_the_bits_and_reset_starts_afresh(gpu, decim, spec, sid):
    D = decim
    x = _block(D)[0]
    whole, produced = _oneshot(D, spec)
    origin = (1 << 42) + 64 * 999
    with _handle(D, slicer=spec) as r:
        r.set_origin(origin)
        assert r.debug_slicer_bits(0, 0)[1] == origin
        r.push_wideband(x[: len(x) // 3])
        r.push_wideband(x[len(x) // 3:])
        bits, p = r.debug_slicer_bits(origin, produced)
        assert p == origin + produced
        assert np.array_equal(bits, whole)
        with pytest.raises(capi.AmpsError) as e:                        # nothing before the origin is held
            r.debug_slicer_bits(origin - 64, 64)
        assert e.value.code == -errno.ERANGE
        # reset: the next push behaves like the first push of a fresh handle
        r.reset()
        assert r.debug_slicer_bits(0, 0)[1] == 0
        r.push_wideband(x)
        bits, p = _bits(r)
    assert p == produced and np.array_equal(bits, whole)


def test_tap_holds_exactly_its_window_on_the_iq_and_translate_seams(gpu):
    """IQ seam: the ring keeps exactly [produced - R, produced), R = the smallest power of two >= max_samples_per_push + sps x 3586 +
    1024 (include/amps_recc.h), and its bits are the CPU model's; the translate seam slices into the same ring"""
    sps, cap, Cn = 10, 8192, 2
    x = np.stack([synth.make_channel_block(120000, 2, seed=500 + c, snr_db=20.0)[0] for c in range(Cn)])
    R = 1 << int(np.ceil(np.log2(cap + sps * 3586 + 1024)))
    with capi.Recc(n_channels=Cn, sps=sps, max_samples=cap, max_bursts=16) as r:
        for off in range(0, x.shape[1], 8000):
            r.push_iq(np.ascontiguousarray(x[:, off:off + 8000]))
        produced = r.debug_slicer_bits(0, 0)[1]
        assert produced == (x.shape[1] // 64) * 64 and produced > R
        bits, _ = r.debug_slicer_bits(produced - R, R)
        for first, n in ((produced - R - 64, 64), (produced - R - 1, 1), (produced, 1), (produced - 64, 65)):
            with pytest.raises(capi.AmpsError) as e:
                r.debug_slicer_bits(first, n)
            assert e.value.code == -errno.ERANGE
    for c in range(Cn):
        f = oracle.Fused(c, sps)
        f.push(x[c])
        assert np.array_equal(bits[c], f.taps()[2][produced - R:produced]), c
    # translate seam: push_raw slices what debug_xlate delivers
    raw = np.stack([np.repeat(x[c, :20000], 2) for c in range(Cn)]).astype(np.complex64)
    with capi.Recc(n_channels=Cn, sps=sps, max_samples=cap, max_bursts=16) as r:
        r.set_xlate(rate_hz=400e3, center_hz=37.5e3, decim=2)
        y = np.concatenate([r.debug_xlate(np.ascontiguousarray(raw[:, o:o + 16000])) for o in range(0, raw.shape[1], 16000)], axis=1)
    with capi.Recc(n_channels=Cn, sps=sps, max_samples=cap, max_bursts=16) as r:
        r.set_xlate(rate_hz=400e3, center_hz=37.5e3, decim=2)
        for off in range(0, raw.shape[1], 16000):
            r.push_raw(np.ascontiguousarray(raw[:, off:off + 16000]))
        got, produced = _bits(r)
    assert produced == (y.shape[1] // 64) * 64
    for c in range(Cn):
        f = oracle.Fused(c, sps)
        f.push(y[c])
        assert np.array_equal(got[c], f.taps()[2][:produced]), c
