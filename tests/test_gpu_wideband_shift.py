"""-m gpu: amps_recc_set_wideband_shift -- a tuner's frequency error corrected inside the filter banks below 1024 branches
(chz_narrow_mix_kernel, chz_grid10_mix_kernel): exact at the quarter-rate shifts against a plain handle on the pre-mixed block, against
the float64 bank on the float64-mixed block within the bound tests/test_cpu_wideband_shift.py states, against itself under other cuts
and in other sample formats, against a twin handle across a retune, against the transmitted words on blocks that decode nothing
uncorrected, and against the IQ seam on the shifted bank's own rows."""
import errno
import functools
import subprocess

import numpy as np
import pytest

import oracle
from oracle import channelizer as cz
from gr_amps_amd import capi
from gr_amps_amd import synth_wideband as sw

import formatblock as fb
import grid10block as gb
import narrowblock as nb
import shiftblock as shb
import slicerbound as sb
import streamoffsetunitref as sur

pytestmark = pytest.mark.gpu
FC32, SC16, SC8, CU8 = capi.SAMPLES_FC32, capi.SAMPLES_SC16, capi.SAMPLES_SC8, capi.SAMPLES_CU8
FMT_IDS = {FC32: "fc32", SC16: "sc16", SC8: "sc8", CU8: "cu8"}
GEOMETRIES = nb.GEOMETRIES + [(M, gb.decim(M)) for M in gb.SIZES]       # six narrow, four on the 10 kHz grid
GEOM_IDS = nb.IDS + gb.IDS


def _grid(M):
    return M in gb.SIZES


def _fs(M):
    return M * (gb.BIN_HZ if _grid(M) else 30e3)


def _taps(M, D):
    return gb.taps(M) if _grid(M) else nb.taps(M, D)


def _whole_band(M, first=0):
    """(n_channels, the bins of the rows) of a handle that decodes every channel from bin `first` on"""
    C = gb.max_channels(M) if _grid(M) else M
    return C, (gb.row_bins(M, first, C) if _grid(M) else (first + np.arange(M)) % M)


def _burst_first(M):
    """the first bin of the band the burst blocks are built for"""
    return gb.FIRST if _grid(M) else 0


def _handle(M, D, max_frames, C=None, first=0, shift=None, max_bursts=64, **kw):
    r = capi.Recc(n_channels=_whole_band(M)[0] if C is None else C, max_samples=max_frames, max_bursts=max_bursts,
                  wideband={"channels": M, "decim": D, "first_channel": first}, **kw)
    if shift is not None:
        r.set_wideband_shift(shift)
    return r


def _bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _tap(r, piece, fmt):
    return r.debug_channelize(piece) if fmt == FC32 else r.debug_channelize_as(piece, fmt)


def _pieces(r, block, cuts, fmt=FC32):
    """the debug tap over block[cuts[i]:cuts[i + 1]]; fmt may be a list, one format per piece, block then a dict by format"""
    out = []
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        f = fmt[i % len(fmt)] if isinstance(fmt, (list, tuple)) else fmt
        out.append(_tap(r, (block[f] if isinstance(block, dict) else block)[a:b], f))
    return out


def _ragged(n, D):
    """pushes of 1, D - 1, D + 1, 3 D + 11 samples and the rest"""
    cuts = np.cumsum([0, 1, D - 1, D + 1, 3 * D + 11]).tolist() + [n]
    assert cuts[-1] > cuts[-2]
    return cuts


def _tone(M, D):
    return gb.tone_block(M) if _grid(M) else shb.narrow_tone_block(M, D)


# ---- 1. quarter-rate shifts are exact
def _integer_block(M, D, fmt):
    """about 44 frames of random samples in the block's own type, negatable: sc8 inside +-127, sc16 inside +-32767"""
    rng = np.random.default_rng(1000 * M + D + fmt)
    n = 44 * D + 7
    if fmt == FC32:
        return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    lo, hi, dt = {SC16: (-32767, 32767, np.int16), SC8: (-127, 127, np.int8), CU8: (0, 255, np.uint8)}[fmt]
    q = rng.integers(lo, hi + 1, (n, 2)).astype(dt)
    q[3], q[4] = (lo, hi), (hi, lo)
    return q


def _times_unit_power(q, fmt, turn):
    """q[n] times turn^n, turn one of -1j, 1j, -1, in q's own type: swaps and negations only"""
    if fmt == FC32:
        z = q.copy()
        k = np.arange(q.shape[0]) % 4
        for p in (1, 2, 3):
            u = turn ** p
            sel = k == p
            # multiply by +-1 or +-i without arithmetic
            z[sel] = {(1, 0): q[sel], (-1, 0): -q[sel], (0, 1): (-q[sel].imag + 1j * q[sel].real), (0, -1): (q[sel].imag - 1j * q[sel].real)}[(int(round(u.real)), int(round(u.imag)))]
        return z.astype(np.complex64)
    neg = (lambda v: (255 - v.astype(np.int16)).astype(np.uint8)) if fmt == CU8 else (lambda v: (-v.astype(np.int32)).astype(v.dtype))
    z = q.copy()
    k = np.arange(q.shape[0]) % 4
    for p in (1, 2, 3):
        u = turn ** p
        re, im = int(round(u.real)), int(round(u.imag))
        sel = k == p
        i, qq = q[sel, 0], q[sel, 1]
        if (re, im) == (-1, 0):
            z[sel, 0], z[sel, 1] = neg(i), neg(qq)
        elif (re, im) == (0, -1):                                            # (I + jQ)(-j) = Q - jI
            z[sel, 0], z[sel, 1] = qq, neg(i)
        elif (re, im) == (0, 1):                                             # (I + jQ)(+j) = -Q + jI
            z[sel, 0], z[sel, 1] = neg(qq), i
    return z


@pytest.mark.parametrize("fmt", list(FMT_IDS), ids=list(FMT_IDS.values()))
@pytest.mark.parametrize("M,D", GEOMETRIES, ids=GEOM_IDS)
def test_quarter_rate_shifts_are_exact(gpu, M, D, fmt):
    """shift = +fs / 4, -fs / 4 and fs / 2: the phasor is exactly +-1 or +-i and the product exact, so the shifted handle on x gives the
    float values a plain handle gives on x (-i)^n, x (+i)^n and x (-1)^n, the pre-mixed block built on the host in the block's own
    integer type.  Ragged pushes: the absolute index holds across carry, leftover samples and formats."""
    fs = _fs(M)
    q = _integer_block(M, D, fmt)
    n = q.shape[0]
    cuts = _ragged(n, D)
    assert np.array_equal(capi.convert_samples(_times_unit_power(q, fmt, -1j), fmt) if fmt != FC32 else _times_unit_power(q, fmt, -1j),
                          (capi.convert_samples(q, fmt) if fmt != FC32 else q) * (-1j) ** (np.arange(n) % 4))
    with _handle(M, D, 64) as plain, _handle(M, D, 64) as shifted:
        for shift, turn in ((0.25 * fs, -1j), (-0.25 * fs, 1j), (0.5 * fs, -1 + 0j)):
            shifted.reset()
            plain.reset()
            shifted.set_wideband_shift(shift)
            assert shifted.wideband_shift == shift and plain.wideband_shift == 0.0
            got = np.concatenate(_pieces(shifted, q, cuts, fmt), axis=1)
            want = np.concatenate(_pieces(plain, _times_unit_power(q, fmt, turn), cuts, fmt), axis=1)
            assert got.shape == want.shape == (_whole_band(M)[0], (n // D) & (~1 if 2 * D == M else ~3)) and got.shape[1] >= 40
            assert np.array_equal(got, want), (shift, np.argwhere(got != want)[:4])
            assert np.abs(got).min() > 0


# ---- 2. against float64
@pytest.mark.parametrize("M,D", [(128, 64), (128, 96), (512, 384), (500, 125), (2500, 625)], ids=["M128-D64", "M128-D96", "M512-D384", "M500", "M2500"])
def test_shifted_bank_against_float64(gpu, M, D):
    """device against cz.channelize(x e^{-2 pi j n step / 2^64}) in float64, every row and frame of a tone block in ragged pieces, at
    +6543.21 Hz and -11 kHz: |y32 - y64| <= FFT_C 2^-24 log2(M) ||Y64(frame)||_2 + DELTA sum_i |h[i]| |x[n0 + i]|, the banks' own
    constant plus what the mixer may add (tests/shiftblock.py; tests/test_cpu_wideband_shift.py holds the numpy statement of the mixer
    to the second term alone).  Measured worst fractions of the bound: M = 128 / 64: 0.154, 128 / 96: 0.151, 512 / 384: 0.131,
    500: 0.124, 2500: 0.102 (in the banks' unit alone: 0.38, 0.39, 0.28, 0.20, 0.15 against FFT_C = 0.54)."""
    fs, h = _fs(M), _taps(M, D)
    x = _tone(M, D)
    n = x.shape[0]
    C, bins = _whole_band(M)
    cuts = [0, D - 5, 4 * D + 6, 154 * D + 17, 156 * D + 18, n]
    weights = shb.frame_weights(x, h, D)
    for shift in shb.SHIFTS:
        step = shb.step_of(shift, fs)
        with _handle(M, D, 320, shift=shift) as r:
            assert abs(r.wideband_shift - shift) <= fs * 2.0 ** -52
            got = np.concatenate(_pieces(r, x, cuts), axis=1)
        want = cz.channelize(shb.mix64(x, step), P=h.size // M, M=M, D=D, taps=h)[:, :got.shape[1]]
        assert got.shape == (C, (n // D) & (~1 if 2 * D == M else ~3))
        unit = sb.U32 * np.log2(M) * np.sqrt((np.abs(want) ** 2).sum(0))
        bound = sb.FFT_C * unit + shb.DELTA * weights[:got.shape[1]]
        frac = np.abs(got - want[bins]) / bound
        print(f"\nM={M} D={D} shift {shift:+.2f}: worst |y32 - y64| / bound = {frac.max():.3f}; in units alone {(np.abs(got - want[bins]) / unit).max():.3f}")
        assert frac.max() <= 1.0, (shift, frac.max(), np.unravel_index(np.argmax(frac), frac.shape))


# ---- 3. one stream, any cut, any format
@pytest.mark.parametrize("M,D", [(128, 96), (500, 125)], ids=["M128-D96", "M500"])
def test_shifted_stream_is_one_stream_at_any_cut_in_any_format(gpu, M, D):
    """with a shift set: a cut stream equals the one-shot bit for bit; sc16, sc8 and cu8 equal fc32 on the converted block; formats
    alternate push by push; a device slice of an 8-bit block is aligned to one sample and not to two"""
    import torch
    x = _tone(M, D)
    n = x.shape[0]
    cuts = [0, 1, D, 2 * D + 1, 5 * D + 12, 150 * D + 5, 151 * D + 4, n]
    with _handle(M, D, 320, shift=6543.21) as r:
        one = r.debug_channelize(x)
        r.reset()
        many = np.concatenate(_pieces(r, x, cuts), axis=1)
        assert one.shape[1] >= 296 and np.array_equal(_bits32(one), _bits32(many))
        with _handle(M, D, 320) as plain:
            assert not np.array_equal(_bits32(one), _bits32(plain.debug_channelize(x)))   # the shift does something
        for fmt in (SC16, SC8, CU8):
            q = np.rint(np.stack([x.real, x.imag], axis=1).astype(np.float64) * (30000.0 / np.abs(x).max())).astype(np.int16) if fmt == SC16 else fb.quantise(x, fmt)
            xf = capi.convert_samples(q, fmt)
            r.reset()
            want = r.debug_channelize(xf)
            r.reset()
            got = np.concatenate(_pieces(r, q, cuts, fmt), axis=1)
            assert np.array_equal(_bits32(got), _bits32(want)), FMT_IDS[fmt]
            r.reset()
            got = np.concatenate(_pieces(r, {fmt: q, FC32: xf}, cuts, [fmt, FC32]), axis=1)
            assert np.array_equal(_bits32(got), _bits32(want)), ("alternating", FMT_IDS[fmt])
            if fmt != SC16:
                big = np.full((n + 3, 2), 77, q.dtype)                       # the block at sample 1 of a larger tensor of other values
                big[1:n + 1] = q
                dev = torch.from_numpy(big).to(gpu)[1:n + 1]
                assert dev.data_ptr() % 4 == 2 and dev.is_contiguous()
                r.reset()
                got = np.concatenate(_pieces(r, dev, cuts, fmt), axis=1)
                assert np.array_equal(_bits32(got), _bits32(want)), ("device", FMT_IDS[fmt])


# ---- 4. retune
def _burst_block(M, D, cfo):
    return gb.burst_block(M, cfo_hz=cfo) if _grid(M) else nb.burst_block(M, D, cfo_hz=cfo)


@pytest.mark.parametrize("M,D", [(128, 96), (500, 125)], ids=["M128-D96", "M500"])
def test_retune_equals_the_twin_from_the_next_push(gpu, M, D):
    """A runs three pushes at f1, then set_wideband_shift(f2); twin B has f2 from creation; the same pushes through the debug tap.
    From the fourth push on A equals B bit for bit; before it they differ.  A refused call (NaN, fs) changes nothing.  Then shift 0
    on A against a plain handle C: bit-equal from the next push.  Records: a burst planted more than 2048 channel-rate samples behind
    the retune push's first frame gives a record byte-identical to the twin's."""
    f1, f2 = 5000.0, -7321.5
    x = _tone(M, D)
    n = x.shape[0]
    cuts = [0, 30 * D + 7, 61 * D - 3, 95 * D + 50, 130 * D + 1, 170 * D + D // 2, 211 * D + 9, 250 * D - 1, n]
    with _handle(M, D, 320, shift=f1) as A, _handle(M, D, 320, shift=f2) as B, _handle(M, D, 320) as C:
        equal_ab, equal_ac = [], []
        for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            if i == 3:
                A.set_wideband_shift(f2)
                assert A.wideband_shift == B.wideband_shift
            if i == 4:                                                       # refused: the handle is as it was
                for bad in (float("nan"), _fs(M), -0.5 * _fs(M) - 1.0):
                    with pytest.raises(capi.AmpsError) as e:
                        A.set_wideband_shift(bad)
                    assert e.value.code == -errno.EINVAL
                assert A.wideband_shift == B.wideband_shift
            if i == 6:
                A.set_wideband_shift(0.0)
                assert A.wideband_shift == 0.0
            ya, yb, yc = (h.debug_channelize(x[a:b]) for h in (A, B, C))
            assert ya.shape == yb.shape == yc.shape and ya.shape[1] >= 28
            equal_ab.append(bool(np.array_equal(_bits32(ya), _bits32(yb))))
            equal_ac.append(bool(np.array_equal(_bits32(ya), _bits32(yc))))
        assert equal_ab == [False] * 3 + [True] * 3 + [False] * 2, equal_ab
        assert equal_ac == [False] * 6 + [True] * 2, equal_ac
    # records
    cfo = 9e3
    xb, truth = _burst_block(M, D, cfo)
    rng = np.random.default_rng(5 + M)
    noise = lambda m: (0.3 * (rng.standard_normal(m) + 1j * rng.standard_normal(m))).astype(np.complex64)
    first, second = noise(40 * D + 17), np.concatenate([noise(2100 * D), xb])
    flush = np.zeros(64 * D, np.complex64)
    cap = (second.shape[0] + 64 * D) // D + 72
    recs = []
    for start in (f1, cfo):
        with _handle(M, D, cap, first=_burst_first(M), shift=start) as r:
            r.push_wideband(first)
            r.set_wideband_shift(cfo)
            r.push_wideband(second)
            r.push_wideband(flush)
            recs.append(r.drain())
    assert len(recs[1]) == 6 and sorted(g["min"].decode() for g in recs[1]) == sorted(v[1] for v in truth.values())
    assert 2100 * D // D >= 2048 + 40                                        # every dotting begins that far behind the retune push's first frame
    assert recs[0].tobytes() == recs[1].tobytes()


# ---- 5. end to end
@functools.lru_cache(maxsize=None)
def _e2e_block(M, D, fmt):
    """(block in fmt, its fc32 conversion, truth) of the +9 kHz burst block"""
    x, truth = _burst_block(M, D, 9e3)
    if fmt == FC32:
        return x, x, truth
    q = fb.quantise(x, fmt)
    return q, capi.convert_samples(q, fmt), truth


@functools.lru_cache(maxsize=None)
def _e2e_model(M, D, fmt, shift):
    """float64: the planted channels' rows of the float64 bank on the float64-mixed converted block, complex128 [6][frames]"""
    _, xf, truth = _e2e_block(M, D, fmt)
    y = cz.channelize(shb.mix64(xf, shb.step_of(shift, _fs(M))), P=_taps(M, D).size // M, M=M, D=D, taps=_taps(M, D))
    _, bins = _whole_band(M, _burst_first(M))
    return y[[int(bins[c]) for c in _planted_channels(M)]]


def _planted_channels(M):
    return [r for r, _ in gb.planted(M)] if _grid(M) else [k for k, _ in nb.planted(M)]


E2E = pytest.mark.parametrize("M,D,fmt", [(128, 96, FC32), (128, 96, SC8), (500, 125, FC32), (500, 125, SC8)], ids=["M128-fc32", "M128-sc8", "M500-fc32", "M500-sc8"])


def _run(M, D, fmt, shift, **kw):
    q, xf, _ = _e2e_block(M, D, fmt)
    n = q.shape[0]
    half = (n // 2) // D * D + 100
    silence = np.zeros(64 * D, np.complex64) if fmt == FC32 else fb.silence(64 * D, fmt)
    with _handle(M, D, (n + 64 * D) // D + 72, first=_burst_first(M), shift=shift, **kw) as r:
        for piece in (q[:half], q[half:], silence):
            r.push_wideband(piece) if fmt == FC32 else r.push_wideband_as(piece, fmt)
        recs = r.drain()
        off = r.burst_offset(recs) if kw else None
    return recs, off


@E2E
def test_a_9_khz_tuner_error_end_to_end(gpu, M, D, fmt):
    """the +9 kHz blocks of tests/test_cpu_wideband_shift.py: the plain handle returns fewer than six planted MINs (the models say
    none), the handle with shift = 9000 all six, on the right channels, valid, MIN and words as transmitted, word_raw as the float64
    bank on the mixed block gives it"""
    _, _, truth = _e2e_block(M, D, fmt)
    mins = sorted(v[1] for v in truth.values())
    plain, _ = _run(M, D, fmt, None)
    assert len([g for g in plain if g["min"].decode() in mins]) < 6
    got, _ = _run(M, D, fmt, 9e3)
    assert len(got) == 6 and sorted(int(g["channel"]) for g in got) == sorted(_planted_channels(M))
    by_chan = {int(g["channel"]): g for g in got}
    for (chan, off), (kind, min10, esn, dialed, words) in truth.items():
        g = by_chan[chan]
        assert g["min"].decode() == min10 and capi.MSG_CLASSES[g["msg_class"]] == kind and g["valid"].all()
        for w, bits in enumerate(words):
            assert list(g["word_dec"][w]) == list(bits)
    ref = oracle.fused_push_all(_e2e_model(M, D, fmt, 9e3).astype(np.complex64), sps=2)
    assert len(ref) == 6
    for a in ref:
        g = by_chan[_planted_channels(M)[int(a["channel"])]]
        assert a["min"] == g["min"] and np.array_equal(a["word_raw"], g["word_raw"])


OFFSET_MARGIN_HZ = 0.5


@E2E
def test_burst_offset_reads_the_residual(gpu, M, D, fmt):
    """stream_offset="unit" on a handle shifted by 7.5 kHz: amps_recc_burst_offset reads the 1.5 kHz that are left, within 0.5 Hz of
    the float64 bank on the float64-mixed block with the float64 unit-amplitude statistic.  The margin is that of
    test_grid10_power_and_offset_rings, and so is its reasoning: the bank's samples are within 2e-6 of the float64 ones at a burst's
    amplitude of 1 (0.01 Hz at 40 ksps), the ring's fp32 sums add 2e-5 rad (0.13 Hz); the mixer adds DELTA sum |h| |x| / |y| < 1e-5
    rad with six mobiles and the noise in the stream, 0.06 Hz.  Measured: 0.0002 Hz at the worst of all four cases."""
    recs, (off_hz, off_n) = _run(M, D, fmt, 7.5e3, stream_offset="unit")
    chans = _planted_channels(M)
    assert len(recs) == 6 and [int(c) for c in recs["channel"]] == sorted(chans) and off_n.min() >= 25
    model = _e2e_model(M, D, fmt, 7.5e3)
    ref = []
    for g, n_blocks in zip(recs, off_n):
        hz, cnt = sur.burst_offset_hz(sur.blocks(model[chans.index(int(g["channel"]))])[0], int(g["position"]), 2)
        assert cnt == n_blocks
        ref.append(hz)
    worst = np.abs(off_hz - np.array(ref)).max()
    print(f"\nM={M} {FMT_IDS[fmt]}: burst offsets {np.round(off_hz, 2)} Hz, float64 {np.round(ref, 2)} Hz, worst difference {worst:.4f} Hz (planted residual +1500)")
    assert worst <= OFFSET_MARGIN_HZ, (off_hz, ref)
    assert np.all(np.abs(off_hz - 1500.0) <= 150.0), off_hz


# ---- 6. rings and reset
def test_shifted_rings_equal_the_iq_seam_on_the_shifted_rows(gpu):
    """M = 128 at D = 64, 60 ksps per channel, which the plain IQ seam takes: the records, power and autocorrelation rings of a handle
    shifted by 7.5 kHz on the +9 kHz block are those of an IQ-seam handle fed the shifted handle's own debug_channelize rows"""
    M, D = 128, 64
    x, truth = nb.burst_block(M, D, 9e3)
    n = x.shape[0]
    xz = np.concatenate([x, np.zeros(64 * D, np.complex64)])
    cap = xz.shape[0] // D + 72
    kw = dict(stream_power=True, stream_offset="unit")
    with _handle(M, D, cap, shift=7.5e3) as r:
        chan = r.debug_channelize(xz)
    with _handle(M, D, cap, shift=7.5e3, **kw) as r:
        half = (n // 2) // D * D + 100
        r.push_wideband(xz[:half])
        r.push_wideband(xz[half:])
        recs = r.drain()
        power, ac = r.channel_power()[0], r.channel_autocorr()[0]
        off_hz, off_n = r.burst_offset(recs)
    with capi.Recc(n_channels=M, sps=3, max_samples=chan.shape[1], max_bursts=64, **kw) as q:
        q.push_iq(chan)
        qrecs = q.drain()
        qpower, qac = q.channel_power()[0], q.channel_autocorr()[0]
        qoff_hz, qoff_n = q.burst_offset(qrecs)
    assert len(recs) == 6 and recs.tobytes() == qrecs.tobytes()
    assert sorted(g["min"].decode() for g in recs) == sorted(v[1] for v in truth.values())
    assert power.shape == qpower.shape and power.shape[1] >= 40 and np.array_equal(_bits32(power), _bits32(qpower))
    assert np.array_equal(_bits32(ac), _bits32(qac))
    assert np.array_equal(_bits32(off_hz), _bits32(qoff_hz)) and np.array_equal(off_n, qoff_n)
    assert np.all(np.abs(off_hz - 1500.0) <= 150.0), off_hz


@pytest.mark.parametrize("M,D", [(128, 96), (500, 125)], ids=["M128-D96", "M500"])
def test_reset_keeps_the_shift_and_restarts_the_index(gpu, M, D):
    """the stream pushed again after a reset gives the first run's bits: the shift is kept, and a sample's phase is again that of
    its index in the new stream (the first run ends off a frame, so the index does not restart at a multiple of anything)"""
    x = _tone(M, D)
    n = x.shape[0]
    cuts = [0, 33 * D + 5, 200 * D + 77, n - 3]                              # leaves samples in the carry: a stream that ends off a frame
    with _handle(M, D, 320, shift=-11000.0) as r:
        was = r.wideband_shift
        first = _pieces(r, x, cuts)
        r.reset()
        assert r.wideband_shift == was and abs(was + 11000.0) < 1e-6
        again = _pieces(r, x, cuts)
        for a, b in zip(first, again):
            assert a.shape[1] > 0 and np.array_equal(_bits32(a), _bits32(b))


def test_the_1024_bank_refuses_and_is_unchanged(gpu):
    """-ENOSYS from both calls on a 1024-channel handle and on a handle without the wideband seam; the records of the 1024 handle
    afterwards are those of a handle that was never asked"""
    D = int(capi.load().amps_recc_default_wideband_decim())
    first, C = 700, 64
    n = int(0.18 * sw.FS_WIDE) // D * D
    x, truth = sw.make_wideband(n, [((first + 20) % 1024, 30000)], seed=77)
    outs = []
    for ask in (False, True):
        with capi.Recc(n_channels=C, sps=1536 // D, max_samples=n // D + 64 + 72, max_bursts=16, wideband={"channels": 1024, "decim": D, "first_channel": first}) as r:
            r.push_wideband(x[:n // 3 + 5])
            if ask:
                for hz in (1e3, 0.0):
                    with pytest.raises(capi.AmpsError) as e:
                        r.set_wideband_shift(hz)
                    assert e.value.code == -errno.ENOSYS
                with pytest.raises(capi.AmpsError) as e:
                    r.wideband_shift
                assert e.value.code == -errno.ENOSYS
                with pytest.raises(capi.AmpsError) as e:
                    r.set_wideband_shift(float("nan"))
                assert e.value.code == -errno.EINVAL
            r.push_wideband(x[n // 3 + 5:])
            r.push_wideband(np.zeros(64 * D, np.complex64))
            outs.append(r.drain())
    assert len(outs[0]) == 1 and outs[0]["min"][0].decode() == list(truth.values())[0][1] and int(outs[0]["channel"][0]) == 20
    assert outs[1].tobytes() == outs[0].tobytes()
    with capi.Recc(n_channels=1, sps=10, max_samples=4096, max_bursts=16) as r:   # no wideband seam
        with pytest.raises(capi.AmpsError) as e:
            r.set_wideband_shift(1e3)
        assert e.value.code == -errno.ENOSYS
        with pytest.raises(capi.AmpsError) as e:
            r.wideband_shift
        assert e.value.code == -errno.ENOSYS


# ---- 7. recctest
def test_recctest_wide_with_a_shift(gpu, tmp_path):
    """`recctest wide block.sc8 ... channels=128 shift=9000` prints the six records of the +9 kHz block, as the C ABI's own records
    give them; without the shift it prints fewer"""
    from gr_amps_amd.host import build_host
    from test_gpu_host_blocks import _expected_lines
    M, D = 128, 96
    x, truth = nb.burst_block(M, D, 9e3)
    q = fb.quantise(x, SC8)
    p = tmp_path / "block.sc8"
    q.tofile(p)
    with capi.Recc(n_channels=M, max_samples=(q.shape[0] + 64 * 768) // D + 72, max_bursts=64, wideband={"channels": M}) as r:
        r.set_wideband_shift(9000.0)
        r.push_wideband_as(q, SC8)
        r.push_wideband_as(fb.silence(64 * 768, SC8), SC8)                   # recctest's own tail of silence
        recs = r.drain()
    assert sorted(int(g["channel"]) for g in recs) == sorted(k for k, _ in nb.planted(M))
    want = []
    for g in recs:
        want.append("MSG channel %d" % int(g["channel"]))
        want += _expected_lines(recs[recs["channel"] == g["channel"]])
    _, exe = build_host()
    out = subprocess.run([exe, "wide", str(p), "777777", "channels=128", "shift=9000"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = [l for l in out.stdout.splitlines() if l.startswith("MSG ")]
    assert sorted(got) == sorted(want) and len([l for l in got if l.startswith("MSG channel")]) == 6
    out = subprocess.run([exe, "wide", str(p), "777777", "channels=128"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and len([l for l in out.stdout.splitlines() if l.startswith("MSG channel")]) < 6
