"""-m gpu: the wideband seam at 25, 20, 10 and 5 Msps -- the filter banks of 2500, 2000, 1000 and 500 branches of 10 kHz at D = M / 4
(chz_grid10_kernel), an AMPS channel on every third bin -- against the float64 filter-bank model, against itself under other cuts of the
stream and in other sample formats, against the CPU model of the IQ seam on the bank's own output, against the transmitted words, and,
for received power and carrier offset, against float64 statistics.  Every parametrised test runs over the four sizes
(tests/grid10block.py holds them, the prototype and the blocks)."""
import errno
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import slicerbound as sb
import streamoffsetunitref as sur
import streampowerref as spr
from gr_amps_amd import capi

import formatblock as fb
import grid10block as gb

pytestmark = pytest.mark.gpu
GRID = pytest.mark.parametrize("M", gb.SIZES, ids=gb.IDS)
FC32, SC16, SC8, CU8 = capi.SAMPLES_FC32, capi.SAMPLES_SC16, capi.SAMPLES_SC8, capi.SAMPLES_CU8
FMT_IDS = {SC16: "sc16", SC8: "sc8", CU8: "cu8"}
GRID_FMT = pytest.mark.parametrize("M,fmt", [(M, f) for M in gb.SIZES for f in FMT_IDS], ids=["M%d-%s" % (M, FMT_IDS[f]) for M in gb.SIZES for f in FMT_IDS])


def _handle(M, C, first, max_frames, max_bursts=64, **kw):
    return capi.Recc(n_channels=C, max_samples=max_frames, max_bursts=max_bursts, wideband={"channels": M, "decim": gb.decim(M), "first_channel": first}, **kw)


def _flush(M):
    return np.zeros(64 * gb.decim(M), np.complex64)


def _bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _pieces_of(r, block, pieces, fmt=None):
    parts, off = [], 0
    for m in pieces:
        piece = block[off:off + m]
        parts.append(r.debug_channelize(piece) if fmt is None else r.debug_channelize_as(piece, fmt))
        off += m
    assert off == block.shape[0]
    return parts


def _tone_pieces(M, n):
    D = gb.decim(M)
    pieces = [D - 5, 3 * D + 11, 150 * D + 11, 2 * D + 1]
    pieces.append(n - sum(pieces))
    assert pieces[-1] > 0
    return pieces


# ---- 1. against float64, bin by bin and frame by frame
@GRID
def test_bank_per_bin_error_on_a_wrapped_band(gpu, M):
    """|y32 - y64| <= c 2^-24 log2(M) ||Y64(frame)||_2 with c = slicerbound.FFT_C, the constant of the 1024 bank, for every row and frame:
    the band's first bin is M - 8, so the rows wrap past bin M - 1; tones sit 3 kHz above the centres of the bins of rows 0, 1, C / 2 - 1,
    C / 2 and C - 1 over noise at 0.02; about 300 frames in ragged pieces, one shorter than a frame, one long enough for several
    workgroups.  Measured worst ratios (against FFT_C = 0.54): M = 2500: 0.090, 2000: 0.061, 1000: 0.079, 500: 0.092."""
    D, C, first = gb.decim(M), gb.max_channels(M), M - 8
    x = gb.tone_block(M)
    n = x.shape[0]
    with _handle(M, C, first, 320) as r:
        parts = _pieces_of(r, x, _tone_pieces(M, n))
        got = np.concatenate(parts, axis=1)
    assert parts[0].shape == (C, 0) and parts[2].shape[1] >= 148 and got.shape == (C, (n // D) & ~3)
    want = gb.tone_model(M)[:, :got.shape[1]]                             # all M bins, float64
    norm = np.sqrt((np.abs(want) ** 2).sum(0))
    bins = gb.row_bins(M, first, C)
    assert bins.max() == M - 2 and bins[3] < bins[2]                       # the rows do wrap
    ratio = np.abs(got - want[bins]) / (sb.U32 * np.log2(M) * norm)
    print(f"\nM={M}: worst |y32 - y64| / (2^-24 log2(M) ||Y64(frame)||) = {ratio.max():.3f}")
    assert ratio.max() <= sb.FFT_C, (ratio.max(), np.unravel_index(np.argmax(ratio), ratio.shape))
    # the tones come out at full scale (unit DC gain, 3 kHz inside the pass band) on their rows, and nowhere else
    quiet = np.ones(C, bool)
    for row, a in zip(gb.tone_rows(M), gb.TONE_AMPS):
        level = np.abs(got[row, 100:]).mean()
        assert 0.9 * a < level < 1.1 * a, (row, level)
        quiet[[(row + d) % C for d in (-1, 0, 1)]] = False
    assert np.abs(got[quiet, 100:]).mean() < 0.02


@GRID
def test_prototype_read_back_by_impulses(gpu, M):
    """the library's prototype is oracle.channelizer.design_taps(3, M, 15e3, chan_hz=10e3) to fp32 rounding: D unit impulses, one of
    every residue mod D and 3 M + D + 1 samples apart, each read in bin 0 by the twelve frames that cover it -- frame m reads tap
    n0 - (m + 1) D + 3 M.  A frame holds one non-zero sample, so its FFT only multiplies it by twiddles, at most once per pass and
    once inside a radix-8 or radix-16 butterfly: 7 complex multiplications by fp32 factors, each within 3 u of exact (u = 2^-24: the
    factor's own rounding and the product's), on a tap that is within u of the float64 design: 22 u |h| in all.  The float64 designs
    (a Bessel series here, numpy's there) agree to 1e-12 of the largest tap."""
    D, L = gb.decim(M), gb.P * M
    h = gb.taps(M)
    n0 = np.arange(D) * (L + D + 1)
    n = int(n0[-1]) + L + 4 * D
    x = np.zeros(n, np.complex64)
    x[n0] = 1.0
    with _handle(M, 1, 0, n // D + 8) as r:
        got = r.debug_channelize(x)[0]
    m = np.arange(got.shape[0])
    want = np.zeros(got.shape[0], np.float64)
    seen = np.zeros(L, bool)
    for p in n0:
        i = p - (m + 1) * D + L
        ok = (i >= 0) & (i < L)
        want[ok] += h[i[ok]]
        seen[i[ok]] = True
    assert seen.all() and got.shape[0] >= (n0[-1] + L) // D
    err = np.abs(got - want)
    tol = 22 * sb.U32 * np.abs(want) + 1e-12 * np.abs(h).max()
    assert np.all(err <= tol), (err / tol).max()


# ---- 2. streaming equals one-shot
@GRID
def test_bank_streaming_equals_one_shot(gpu, M):
    D = gb.decim(M)
    rng = np.random.default_rng(2 + M)
    n = 20000 + 96 * D + 77
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    first, C = 5, gb.max_channels(M) - 3
    with _handle(M, C, first, n // D + 8) as r:
        one = r.debug_channelize(x)
    with _handle(M, C, first, n // D + 8) as r:
        parts, off = [], 0
        for m in (1, D - 1, D, D + 1, 5000, 12345, n):
            m = min(m, n - off)
            assert m > 0
            parts.append(r.debug_channelize(x[off:off + m]))
            off += m
        many = np.concatenate(parts, axis=1)
    assert off == n and one.shape == (C, (n // D) & ~3) and many.shape == one.shape
    assert np.array_equal(_bits32(one), _bits32(many))                   # a frame's arithmetic does not depend on the cut
    assert np.abs(one).min() > 0                                          # every row and frame was written


# ---- 3. bursts
def _halves(n, D):
    return (n // 2) // D * D + 100


@GRID
def test_grid10_bursts_decode_to_the_transmitted_words(gpu, M):
    D, C = gb.decim(M), gb.max_channels(M)
    x, truth = gb.burst_block(M)
    n = x.shape[0]
    cap = (n + 64 * D) // D + 72
    with _handle(M, C, gb.FIRST, cap) as r:
        assert r.sps == 2 and r.decim == D
        chan = r.debug_channelize(np.concatenate([x, _flush(M)]))
    with _handle(M, C, gb.FIRST, cap) as r:
        r.push_wideband(x[:_halves(n, D)])
        r.push_wideband(x[_halves(n, D):])
        r.push_wideband(_flush(M))
        got = r.drain()
    assert len(got) == 6
    by_chan = {int(g["channel"]): g for g in got}
    for (row, off), (kind, min10, esn, dialed, words) in truth.items():
        g = by_chan[row]
        assert g["min"].decode() == min10 and capi.MSG_CLASSES[g["msg_class"]] == kind and g["valid"].all()
        for w, bits in enumerate(words):
            assert list(g["word_dec"][w]) == list(bits)
    # the kernels behind the bank are bit-exact against the CPU model when both see the bank's own output
    active = sorted(by_chan)
    want = oracle.fused_push_all(chan[active], sps=2)
    want["channel"] = np.array(active, np.uint32)[want["channel"]]
    assert got.tobytes() == want.tobytes()
    # and the float64 bank leads to the same words
    ref = oracle.fused_push_all(gb.model_rows(M).astype(np.complex64), sps=2)
    assert len(ref) == 6
    for a in ref:
        g = by_chan[gb.planted(M)[int(a["channel"])][0]]
        assert a["min"] == g["min"] and np.array_equal(a["word_raw"], g["word_raw"])


# ---- 4. integer formats
def _quantise(x, fmt):
    if fmt == SC16:
        peak = max(np.abs(x.real).max(), np.abs(x.imag).max())
        return np.rint(np.stack([x.real, x.imag], axis=1).astype(np.float64) * (30000.0 / peak)).astype(np.int16)
    return fb.quantise(x, fmt)


def _silence(n, fmt):
    return np.zeros((n, 2), np.int16) if fmt == SC16 else fb.silence(n, fmt)


def _extremes(q, fmt):
    """plant the format's extreme codes, both components, a few samples apart"""
    lo, hi = {SC16: (-32768, 32767), SC8: (-128, 127), CU8: (0, 255)}[fmt]
    n = q.shape[0]
    for i, pair in ((5, (lo, hi)), (6, (hi, lo)), (n // 2, (lo, lo)), (n // 2 + 1, (hi, hi)), (n - 3, (hi, lo))):
        q[i] = pair
    assert q.min() == lo and q.max() == hi
    return q


@functools.lru_cache(maxsize=None)
def _burst_block_as(M, fmt):
    """(q [n, 2] in fmt, xf = capi.convert_samples(q, fmt), the fc32 handle's records on xf and the converted silence)"""
    x, _ = gb.burst_block(M)
    D, n = gb.decim(M), x.shape[0]
    q = _quantise(x, fmt)
    xf = capi.convert_samples(q, fmt)
    with _handle(M, gb.max_channels(M), gb.FIRST, (n + 64 * D) // D + 72) as r:
        r.push_wideband(xf[:_halves(n, D)])
        r.push_wideband(xf[_halves(n, D):])
        r.push_wideband(capi.convert_samples(_silence(64 * D, fmt), fmt))
        want = r.drain()
    return q, xf, want


@GRID_FMT
def test_integer_formats_equal_the_converted_block(gpu, M, fmt):
    """debug_channelize_as and push_wideband_as are the fc32 calls on capi.convert_samples of the block, bit for bit and record for
    record: the tone block with the format's extreme codes planted, in ragged pieces, from the host and from a device slice that is
    aligned to one sample and not to two; the burst block in the format alone, and with the format and fc32 taking turns push by push."""
    import torch
    D, C = gb.decim(M), gb.max_channels(M)
    q = _extremes(_quantise(gb.tone_block(M), fmt), fmt)
    xf = capi.convert_samples(q, fmt)
    n = q.shape[0]
    pieces = _tone_pieces(M, n)
    with _handle(M, C, M - 8, 320) as r:
        want = _pieces_of(r, xf, pieces)
    with _handle(M, C, M - 8, 320) as r:
        got = _pieces_of(r, q, pieces, fmt)
    assert want[0].shape == (C, 0) and sum(p.shape[1] for p in want) == (n // D) & ~3
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(_bits32(g), _bits32(w)), (i, pieces[i])
    assert np.abs(np.concatenate(want, axis=1)).min() > 0                  # every row and frame was written
    big = np.full((n + 3, 2), 77, q.dtype)                                 # the block at sample 1 of a larger tensor of other values
    big[1:n + 1] = q
    dev = torch.from_numpy(big).to(gpu)[1:n + 1]
    size = 2 * q.dtype.itemsize
    assert dev.data_ptr() % (2 * size) == size and dev.is_contiguous()
    with _handle(M, C, M - 8, 320) as r:
        got = _pieces_of(r, dev, pieces, fmt)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(_bits32(g), _bits32(w)), ("device", i, pieces[i])
    # records
    qb, xb, want = _burst_block_as(M, fmt)
    nb_ = qb.shape[0]
    cap = (nb_ + 64 * D) // D + 72
    assert len(want) == 6 and sorted(int(c) for c in want["channel"]) == sorted(row for row, _ in gb.planted(M))
    with _handle(M, C, gb.FIRST, cap) as r:
        r.push_wideband_as(qb[:_halves(nb_, D)], fmt)
        r.push_wideband_as(qb[_halves(nb_, D):], fmt)
        r.push_wideband_as(_silence(64 * D, fmt), fmt)
        assert r.drain().tobytes() == want.tobytes()
    cuts = [0, nb_ // 5 + 3, nb_ // 2 + D // 3, 3 * nb_ // 4 + 1, nb_ - D - 1, nb_]
    with _handle(M, C, gb.FIRST, cap) as r:
        for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            if i % 2 == 0:
                r.push_wideband_as(qb[a:b], fmt)
            else:
                r.push_wideband(xb[a:b])
        r.push_wideband_as(_silence(64 * D, fmt), fmt)
        assert r.drain().tobytes() == want.tobytes()


# ---- 5. ragged pushes through the handle
@pytest.mark.parametrize("M", [500, 2500], ids=["M500", "M2500"])
def test_ragged_pushes_leave_the_one_shot_handles_bits(gpu, M):
    """a push shorter than a frame, pushes that leave 1, 2, 3 and 0 frames waiting in the carry, exactly four frames, exactly one
    workgroup's frames, several workgroups' and odd ends: after every push the slicer-bit ring reads as the one-shot handle's"""
    D, FR, C = gb.decim(M), (8 if M == 500 else 4), 40
    x, _ = gb.burst_block(M)
    sched = [D - 5, 5, D, D, D, 4 * D, FR * D, 2 * D + 7, 2 * D - 7, 37 * FR * D + 3 * D + 11, D - 11, 64 * D, 3 * D, 200 * D + 1, 131 * D - 1]
    n = sum(sched)
    x = x[20000:20000 + n]
    cap = n // D + 72
    with _handle(M, C, gb.FIRST, cap) as r:
        r.push_wideband(x)
        produced = r.debug_slicer_bits(0, 0)[1]
        one = r.debug_slicer_bits(0, produced)[0]
    assert produced == ((n // D) & ~3) // 64 * 64 and produced >= 384 and one.shape == (C, produced)
    frames = []
    with _handle(M, C, gb.FIRST, cap) as r:
        off = prev = 0
        for m in sched:
            r.push_wideband(x[off:off + m])
            off += m
            now = r.debug_slicer_bits(0, 0)[1]
            assert now == ((off // D) & ~3) // 64 * 64, (off, now)
            if now > prev:
                assert np.array_equal(r.debug_slicer_bits(prev, now - prev)[0], one[:, prev:now]), (off, prev, now)
            frames.append((off // D) & ~3)
            prev = now
    assert prev == produced and frames[:7] == [0, 0, 0, 0, 4, 8, 8 + FR]
    assert 0 < one.mean() < 1


# ---- 6. received power and carrier offset
@GRID
def test_grid10_power_and_offset_rings(gpu, M):
    """40 ksps per channel, which the plain IQ seam does not take: the rings are the same under another cut of the stream, the power
    blocks are within 2e-5 relative (the bound tests/test_gpu_stream_power.py derives: 257 u) of the float64 mean of |y|^2 over blocks
    of 256 of the bank's own output, and a burst planted 1500 Hz above its centre reads, through amps_recc_burst_offset, what the
    float64 bank with the float64 unit-amplitude statistic reads, within 0.5 Hz: a sample of the fp32 bank is within
    FFT_C 2^-24 log2(M) ||Y|| < 2e-6 of the float64 one at a burst's amplitude of 1, a phase error that is 0.01 Hz at 40 ksps, and
    the ring's fp32 sums add 2e-5 rad, 0.13 Hz.  A conversion at another rate than 40 ksps -- 30 kHz M / D is 120 ksps here -- would
    read a multiple of the offset.  Every burst reads within 150 Hz of what was planted, as on the narrow banks."""
    D, C = gb.decim(M), gb.max_channels(M)
    x, truth = gb.burst_block(M, 1500.0)
    n = x.shape[0]
    xz = np.concatenate([x, _flush(M)])
    cap = xz.shape[0] // D + 72
    rows = [row for row, _ in gb.planted(M)]
    with _handle(M, C, gb.FIRST, cap) as r:
        chan = r.debug_channelize(xz)
    outs = []
    for cuts in ([0, _halves(n, D), xz.shape[0]], [0, 7 * D + 5, n // 3, n // 3 + D - 1, 2 * n // 3 + 17, xz.shape[0]]):
        with _handle(M, C, gb.FIRST, cap, stream_power=True, stream_offset="unit") as r:
            for a, b in zip(cuts[:-1], cuts[1:]):
                r.push_wideband(xz[a:b])
            recs = r.drain()
            power, pfirst = r.channel_power()
            ac, afirst = r.channel_autocorr()
            off_hz, off_n = r.burst_offset(recs)
            outs.append((recs, power, ac, off_hz, off_n))
            assert pfirst == 0 and afirst == 0
    assert len(outs[0][0]) == 6 and outs[0][0].tobytes() == outs[1][0].tobytes()
    assert np.array_equal(_bits32(outs[0][1]), _bits32(outs[1][1])) and np.array_equal(_bits32(outs[0][2]), _bits32(outs[1][2]))
    assert np.array_equal(_bits32(outs[0][3]), _bits32(outs[1][3])) and np.array_equal(outs[0][4], outs[1][4])
    recs, power, ac, off_hz, off_n = outs[0]
    assert sorted(g["min"].decode() for g in recs) == sorted(v[1] for v in truth.values())
    want = spr.blocks(chan[:, :chan.shape[1] // 64 * 64])
    assert power.shape == want.shape and want.min() > 0
    err = np.abs(power.astype(np.float64) - want) / want
    print(f"\nM={M}: worst |P_gpu - P_ref| / P_ref = {err.max():.3g} (bound 2e-5) over {want.size} blocks")
    assert np.all(err <= 2e-5)
    model = gb.model_rows(M, 1500.0)
    assert [int(c) for c in recs["channel"]] == sorted(rows) and off_n.min() >= 25      # 3374 symbols x 2 samples / 256: 25 or 26 whole blocks
    ref = []
    for g, n_blocks in zip(recs, off_n):
        hz, cnt = sur.burst_offset_hz(sur.blocks(model[rows.index(int(g["channel"]))])[0], int(g["position"]), 2)
        assert cnt == n_blocks
        ref.append(hz)
    print(f"M={M}: burst offsets {np.round(off_hz, 2)} Hz, float64 bank and statistic {np.round(ref, 2)} Hz (planted +1500)")
    assert np.all(np.abs(off_hz - np.array(ref)) <= 0.5), (off_hz, ref)
    assert np.all(np.abs(off_hz - 1500.0) <= 150.0), off_hz


# ---- 7. refusals
def test_grid10_refusals(gpu):
    def refused(wb, n_channels=4, **kw):
        with pytest.raises(capi.AmpsError) as e:
            capi.Recc(n_channels=n_channels, max_samples=1024, max_bursts=16, wideband=wb, **kw)
        return e.value.code

    for M in gb.SIZES:
        D = M // 4
        assert refused({"channels": M}) == -errno.EINVAL                                   # no decimation stated
        for bad in (M // 2, 3 * M // 4, D + 1):
            assert refused({"channels": M, "decim": bad}) == -errno.EINVAL
            assert refused({"channels": M, "decim": bad, "taps_per_branch": 3}, sps=2) == -errno.EINVAL
        assert refused({"channels": M, "decim": D, "taps_per_branch": 8}) == -errno.EINVAL
        assert refused({"channels": M, "decim": D}, n_channels=M // 3 + 1) == -errno.EINVAL
        assert refused({"channels": M, "decim": D, "first_channel": M}) == -errno.EINVAL
        assert refused({"channels": M, "decim": D, "groups": 2}) == -errno.EINVAL
        assert refused({"channels": M, "decim": D}, channel_power=True) == -errno.EINVAL
        assert refused({"channels": M, "decim": D}, sps=3) == -errno.EINVAL
        with _handle(M, M // 3, M - 1, 1024, unfused_wideband=(M == 1000)) as r:          # the flag is accepted and changes nothing
            with pytest.raises(capi.AmpsError) as e:
                r.rccl_init(bytes(128), 1, 0)
            assert e.value.code == -errno.ENOSYS
    # cfg.wideband_decim = 0 itself, which the binding never hands over
    cfg = capi.Cfg()
    cfg.struct_size, cfg.n_channels, cfg.max_samples_per_push, cfg.max_bursts, cfg.device = capi.C.sizeof(capi.Cfg), 4, 1024, 16, -1
    cfg.wideband_channels = 1000
    h = capi.C.c_void_p()
    assert capi.load().amps_recc_create(capi.C.byref(h), capi.C.byref(cfg)) == -errno.EINVAL and not h.value
    cfg.wideband_decim = 250                                                               # ... and with it stated: taps 0 -> 3, sps 0 -> 2
    assert capi.load().amps_recc_create(capi.C.byref(h), capi.C.byref(cfg)) == 0
    capi.load().amps_recc_destroy(h)


def test_oversized_push_consumes_nothing(gpu):
    """-E2BIG: the handle's bits and records afterwards are those of a handle that was never offered the block"""
    M = 500
    D, C = gb.decim(M), gb.max_channels(M)
    x, _ = gb.burst_block(M)
    n = x.shape[0]
    cap = (n + 64 * D) // D + 72
    outs = []
    for offer in (False, True):
        with _handle(M, C, gb.FIRST, cap) as r:
            r.push_wideband(x[:_halves(n, D)])
            if offer:
                with pytest.raises(capi.AmpsError) as e:
                    r.push_wideband(np.ones((cap + 8) * D, np.complex64))
                assert e.value.code == -errno.E2BIG
                with pytest.raises(capi.AmpsError) as e:
                    r.debug_channelize_as(np.full(((cap + 8) * D, 2), 50, np.int8), SC8)
                assert e.value.code == -errno.E2BIG
            r.push_wideband(x[_halves(n, D):])
            r.push_wideband(_flush(M))
            recs = r.drain()
            produced = r.debug_slicer_bits(0, 0)[1]
            outs.append((recs, produced, r.debug_slicer_bits(produced - 4096, 4096)[0]))
    assert len(outs[0][0]) == 6 and outs[1][0].tobytes() == outs[0][0].tobytes()
    assert outs[1][1] == outs[0][1] and np.array_equal(outs[1][2], outs[0][2])


# ---- 8. tools
@pytest.mark.parametrize("ext", ["fc32", "sc8"])
def test_recctest_wide_with_channels_500(gpu, tmp_path, ext):
    """gr::amps::recc_wideband::make(..., decim = 125, ..., channels = 500, input_format) through recctest, which sets the decimation of
    these sizes itself: a 5 Msps capture file in, the lines of the six bursts out, as the C ABI's own records give them"""
    from gr_amps_amd.host import build_host
    from test_gpu_host_blocks import _expected_lines
    M = 500
    D, C = gb.decim(M), gb.max_channels(M)
    x, truth = gb.burst_block(M, first=0)                        # recctest's band starts at bin 0
    p = tmp_path / ("block." + ext)
    if ext == "sc8":
        q = fb.quantise(x, SC8)
        q.tofile(p)
        x = capi.convert_samples(q, SC8)
    else:
        x.tofile(p)
    with _handle(M, C, 0, (x.shape[0] + 64 * 768) // D + 72) as r:
        r.push_wideband(x)
        r.push_wideband(np.zeros(64 * 768, np.complex64))        # recctest's own tail of silence
        recs = r.drain()
    assert len(recs) == 6
    want = []
    for g in recs:
        want.append("MSG channel %d" % int(g["channel"]))
        want += _expected_lines(recs[recs["channel"] == g["channel"]])
    _, exe = build_host()
    out = subprocess.run([exe, "wide", str(p), "777777", "channels=500"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = [l for l in out.stdout.splitlines() if l.startswith("MSG ")]
    assert sorted(got) == sorted(want) and len([l for l in got if l.startswith("MSG channel")]) == 6


def test_example_decodes_a_5_msps_stream(gpu):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "decode_wideband.py"), "--channels", "500"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "MISMATCH" not in out.stdout and " decoded" in out.stdout
