"""-m gpu: the carrier-offset measurement of the IQ and translate seams (AMPS_RECC_FLAG_STREAM_OFFSET: amps_recc_channel_autocorr,
amps_recc_burst_autocorr, amps_recc_burst_offset) against the float64 model tests/streamoffsetref.py.

Tolerance of a block, derived and not measured.  Each component of A[c][j] is a sum of 256 fp32 terms fma(p, q, r * s) with
|p q| + |r s| <= |y[s]| |y[s - 1]|: a term carries at most 2 u |y[s]| |y[s - 1]| (the product's rounding and the fma's), u = 2^-24, and
adding 256 of them carries at most 255 u times the sum of their magnitudes whatever the order.  The terms cancel, so the bound is
relative to W = 2^-8 sum |y[s]| |y[s - 1]| (streamoffsetref.weights), not to |A|: |A_gpu - A_ref| <= 257 u W = 1.54e-5 W per component.
The checks use REL = 2e-5 (the power tests' figure), against float64 on the very fp32 samples the seam sliced.

Tolerance of an angle.  With both components within E of the model's A, the argument is within asin(sqrt(2) E / |A|) of the model's
(a disc of radius sqrt(2) E around A, seen from the origin).  A burst sum adds the blocks' E and the gather's own additions: fewer than
`count` per lane chain and butterfly together, each within u of the magnitudes added so far, so count * u * sum(|re A_j| + |im A_j|) at
most.  The host formula (double, rounded to float once) adds half a float ulp of the result.

Bounds against what was SENT come from the CPU measurement alone (scripts/offset_estimator_cpu.py): twice the IQ-seam
table's figure; behind the channel filter the table's error at the tested point times 1.5.

The origin cases use 960 and 1024: amps_recc_set_origin takes multiples of 64 only."""
import functools
import math

import numpy as np
import pytest

import streamoffsetref as sor
import streampowerref as spr
from gr_amps_amd import capi, synth
from test_gpu_stream_power import PIECES, XL, _configure, _cuts, _ints

pytestmark = pytest.mark.gpu

REL = 2e-5
U = 2.0 ** -24


def _noise(seed, shape, scale=1.0):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * scale).astype(np.complex64)


def _noise_plus_tone(seed, C, n):
    """noise of unit variance per component over a tone of amplitude 1.5 at a frequency of the row's own, scaled per row"""
    k = np.arange(n)
    f = np.linspace(-0.21, 0.17, C)[:, None]
    y = _noise(seed, (C, n)) + 1.5 * np.exp(2j * np.pi * f * k[None, :])
    return (y * np.linspace(0.25, 2.0, C)[:, None]).astype(np.complex64)


def _bits(a):
    return np.ascontiguousarray(a, np.complex64).view(np.uint32)


def _check(got, y, origin=0, cols=slice(None)):
    """every component of every block within REL * W of the model on the same samples"""
    want, w = sor.blocks(y, origin=origin)[:, cols], sor.weights(y, origin=origin)[:, cols]
    assert got.shape == want.shape and got.dtype == np.complex64, (got.shape, want.shape)
    assert want.size and w.min() > 0
    err = np.maximum(np.abs(got.real.astype(np.float64) - want.real), np.abs(got.imag.astype(np.float64) - want.imag)) / w
    print("\nworst component error / W = %.3g (bound %.3g) over %d blocks" % (err.max(), REL, want.size))
    assert np.all(err <= REL), np.unravel_index(np.argmax(err), err.shape)
    return want, w


def _iq(C, n, **kw):
    return capi.Recc(n_channels=C, sps=kw.pop("sps", 10), max_samples=kw.pop("max_samples", n), max_bursts=kw.pop("max_bursts", 16),
                     stream_offset=kw.pop("stream_offset", True), **kw)


# ---- 1. the IQ seam, ragged pushes
@pytest.mark.parametrize("C", [5, 66])
def test_iq_seam_blocks_equal_the_model_however_the_stream_is_cut(gpu, C):
    import torch
    n = sum(PIECES)
    assert n == 6000
    y = _noise_plus_tone(200 + C, C, n)
    # what the pushes process: n_done after each, by the seam's rule (whole 64-sample words of what has arrived).  Launch boundaries at
    # all four residues mod 256: blocks that begin at the launch's first sample, inside the carry, and that straddle carry and block
    done = [int(e) // 64 * 64 for _, e in _cuts(PIECES)]
    assert done[0] == 0 and done[6] == done[5] and {d % 256 for d in done} == {0, 64, 128, 192}
    # a sample whose predecessor is the carry's last sample: a push that begins on a word boundary leaves nothing unprocessed before it
    with _iq(C, n) as r:
        assert r.autocorr_ring_blocks * 256 >= n
        r.push_iq(y)
        one, first = r.channel_autocorr()
    assert first == 0 and one.shape == (C, n // 64 * 64 // 256) == (C, 23)
    _check(one, y[:, :n // 64 * 64])

    def ragged(device):
        with _iq(C, n) as r:
            seen = []
            for a, b in _cuts(PIECES):
                if device:                                           # device memory, row pitch 13 samples more than the push
                    t = torch.zeros((C, b - a + 13), dtype=torch.complex64, device=gpu)
                    t[:, :b - a] = torch.from_numpy(y[:, a:b]).to(gpu)
                    r.push_iq(t, nsamp=int(b - a))
                else:
                    r.push_iq(np.ascontiguousarray(y[:, a:b]))
                seen.append(r.channel_autocorr()[0].shape[1])
            A, f = r.channel_autocorr()
        assert f == 0 and seen == [d // 256 for d in done]           # block j exists once 256 (j + 1) <= produced
        return A

    assert np.array_equal(_bits(ragged(False)), _bits(one))
    assert np.array_equal(_bits(ragged(True)), _bits(one))


def test_word_aligned_pushes_take_the_predecessor_from_the_carry(gpu):
    """pushes of 64 k samples leave no remainder: every launch's first sample has the carry's LAST sample as its predecessor, and
    launches that begin at s = 256 j read it through lane 0's extra load"""
    C, pieces = 3, [256, 64, 192, 512, 320, 704]
    n = sum(pieces)
    y = _noise_plus_tone(77, C, n)
    with _iq(C, n) as r:
        r.push_iq(y)
        one, _ = r.channel_autocorr()
    with _iq(C, n) as r:
        for a, b in _cuts(pieces):
            r.push_iq(np.ascontiguousarray(y[:, a:b]))
        cut, _ = r.channel_autocorr()
    _check(one, y)
    assert one.shape == (C, n // 256) and np.array_equal(_bits(cut), _bits(one))


# ---- 2. the origin
def test_origin_moves_the_block_edges(gpu):
    C, n, origin = 5, 3000, 960
    y = _noise_plus_tone(7, C, n)
    with _iq(C, n) as r:
        r.set_origin(origin)
        r.push_iq(y[:, :777])
        r.push_iq(y[:, 777:])
        got, first = r.channel_autocorr()
        _, produced = r.debug_slicer_bits(origin, 0)
        out = np.zeros((C, 1), np.complex64)
        L = capi.load()
        assert L.amps_recc_channel_autocorr(r._h, 3, 1, out.ctypes.data, 1, None, None) == -34     # block 3 begins before the origin
        assert L.amps_recc_channel_autocorr(r._h, 4, 1, out.ctypes.data, 1, None, None) == 0
    assert produced == origin + n // 64 * 64
    assert first == sor.first_block(origin) == 4 and first + got.shape[1] == produced // 256
    _check(got, y[:, :n // 64 * 64], origin=origin)                  # s = origin + m
    assert np.array_equal(_bits(out[:, 0]), _bits(got[:, 0]))


def test_the_sample_in_front_of_the_stream_is_zero(gpu):
    """origin 1024: block 4 begins at the stream's first sample, so its first product is y[0] * conj(0).  That is the model, which puts
    a zero in front -- and not the model of a stream that had one more sample before it."""
    C, n, origin = 3, 2048, 1024
    y = _noise_plus_tone(8, C, n + 1)                                # y[:, 0] is the sample that does NOT exist
    y[:, :2] = (2 + 1j) * np.linspace(0.25, 2.0, C, dtype=np.float32)[:, None]     # the product in question is no accident of the noise
    with _iq(C, n) as r:
        r.set_origin(origin)
        r.push_iq(np.ascontiguousarray(y[:, 1:]))
        got, first = r.channel_autocorr()
    assert first == 4 and got.shape == (C, 8)
    want, w = _check(got, y[:, 1:], origin=origin)
    longer = sor.blocks(y, origin=origin - 1)                        # fed one earlier sample: the blocks of samples 1 ... with y[0] in front
    # (origin - 1 = 1023 puts block 4 at the second sample of the longer stream)
    assert longer.shape == want.shape and np.allclose(longer[:, 1:], want[:, 1:], rtol=0, atol=1e-12)
    gap = np.abs(longer[:, 0] - want[:, 0])
    assert np.all(gap > 100 * REL * w[:, 0])                         # |y[1]| |y[0]| / 256: far beyond the tolerance
    assert np.all(np.abs(got[:, 0] - longer[:, 0]) > 0.5 * gap)


# ---- 3. the ring
def test_ring_holds_exactly_the_window(gpu):
    C, sps, push, n = 2, 3, 1000, 50000
    y = _noise_plus_tone(11, C, n)
    L = capi.load()
    with _iq(C, n, sps=sps, max_samples=1024) as r:
        slots = r.autocorr_ring_blocks
        assert slots == 64                                           # R = 16384: the smallest power of two >= 1024 + 3 * 3586 + 1024
        for a in range(0, n, push):
            r.push_iq(np.ascontiguousarray(y[:, a:a + push]))
        got, first = r.channel_autocorr()
        _, produced = r.debug_slicer_bits(0, 0)
        prod = first + got.shape[1]
        rows, ps = capi.C.c_uint32(0), capi.C.c_uint64(0)
        assert L.amps_recc_channel_autocorr(r._h, 0, 0, None, 0, capi.C.byref(rows), capi.C.byref(ps)) == 0    # n = 0 only reports
        assert rows.value == C and ps.value == prod
        out = np.zeros((C, slots + 1), np.complex64)
        p = out.ctypes.data
        assert L.amps_recc_channel_autocorr(r._h, first - 1, 1, p, slots + 1, None, None) == -34          # -ERANGE: no longer held
        assert L.amps_recc_channel_autocorr(r._h, first - 1, slots + 1, p, slots + 1, None, None) == -34
        assert L.amps_recc_channel_autocorr(r._h, first, slots + 1, p, slots + 1, None, None) == -34      # not yet produced
        assert L.amps_recc_channel_autocorr(r._h, prod + 1, 0, None, 0, None, None) == 0
        assert L.amps_recc_channel_autocorr(r._h, prod + 1, 1, p, slots + 1, None, None) == -34
        assert L.amps_recc_channel_autocorr(r._h, prod - 1, 2, p, slots + 1, None, None) == -34
        assert L.amps_recc_channel_autocorr(r._h, prod, 0, None, 0, None, None) == 0
        assert L.amps_recc_channel_autocorr(r._h, prod - 1, 1, p, slots + 1, None, None) == 0
        assert np.array_equal(_bits(out[:, 0]), _bits(got[:, -1]))
        assert L.amps_recc_channel_autocorr(r._h, first, slots, p, slots + 1, None, None) == 0            # the whole window, wrapped
        assert np.array_equal(_bits(out[:, :slots]), _bits(got))
        assert L.amps_recc_channel_autocorr(r._h, first, 1, None, 0, None, None) == -22                   # argument errors as for power
        assert L.amps_recc_channel_autocorr(r._h, first, 2, p, 1, None, None) == -22
        assert L.amps_recc_channel_autocorr(None, 0, 0, None, 0, None, None) == -22
        r.reset()                                                    # reset empties the window
        empty, f0 = r.channel_autocorr()
        assert empty.shape == (C, 0) and f0 == 0
    assert produced == n // 64 * 64 and produced > 3 * 64 * 256      # three turns of the ring
    assert prod == produced // 256 and first == prod - slots
    _check(got, y[:, :produced], cols=slice(first, prod))


# ---- 4. the translate seams: the sums of what the stage delivers
@pytest.mark.parametrize("name", sorted(XL))
def test_translate_seams_report_the_sums_of_the_stage_output(gpu, name):
    cfg, C, sps, n, fmt, nmax = XL[name]
    rows = cfg[0] == "rows"
    if fmt == capi.SAMPLES_FC32:
        x = _noise(21, (C, n) if rows else n, 0.5)
    else:
        x = _ints(fmt, n, 22)
    cuts = _cuts([n // 3 + 17, 5, n - n // 3 - 22])                  # ragged, one piece shorter than any decimation
    with capi.Recc(n_channels=C, sps=sps, max_samples=nmax, max_bursts=16) as twin, \
         capi.Recc(n_channels=C, sps=sps, max_samples=nmax, max_bursts=16, stream_offset=True) as r:
        _configure(twin, cfg)
        _configure(r, cfg)
        ys = []
        for a, b in cuts:
            if rows:
                ys.append(twin.debug_xlate(np.ascontiguousarray(x[:, a:b])))
                r.push_raw(np.ascontiguousarray(x[:, a:b]))
            elif fmt == capi.SAMPLES_FC32:
                ys.append(twin.debug_xlate_shared(x[a:b]))
                r.push_raw_shared(x[a:b])
            else:
                ys.append(twin.debug_xlate_shared_as(x[a:b], fmt))
                r.push_raw_shared_as(x[a:b], fmt)
        got, first = r.channel_autocorr()
        _, produced = r.debug_slicer_bits(0, 0)
        if not rows:                                                 # the tap leaves the window alone
            (r.debug_xlate_shared if fmt == capi.SAMPLES_FC32 else functools.partial(r.debug_xlate_shared_as, format=fmt))(x[:999])
            again, f2 = r.channel_autocorr()
            assert f2 == first and np.array_equal(_bits(again), _bits(got))
    y = np.concatenate(ys, axis=1)
    assert y.shape[0] == C and produced == y.shape[1] // 64 * 64 and produced > 7000
    assert first == 0 and got.shape == (C, produced // 256)
    _check(got, y[:, :produced])


def test_an_sc16_stream_and_its_fc32_conversion_give_the_same_bits(gpu):
    cfg, C, sps, n, _, nmax = XL["2400k_d12_cu8"]
    q = _ints(capi.SAMPLES_SC16, n, 23)
    xf = capi.convert_samples(q, capi.SAMPLES_SC16)
    A = []
    for fmt, data in ((capi.SAMPLES_SC16, q), (capi.SAMPLES_FC32, xf)):
        with capi.Recc(n_channels=C, sps=sps, max_samples=nmax, max_bursts=16, stream_offset=True) as r:
            _configure(r, cfg)
            for a, b in _cuts([50001, n - 50001]):
                if fmt == capi.SAMPLES_FC32:
                    r.push_raw_shared(data[a:b])
                else:
                    r.push_raw_shared_as(data[a:b], fmt)
            A.append(r.channel_autocorr()[0])
    assert A[0].shape == (C, n // 12 // 64 * 64 // 256) and A[0].any()
    assert np.array_equal(_bits(A[0]), _bits(A[1]))


# ---- 5. what the numbers mean
def _angle_bound_hz(err, mag, fs, f):
    """the frequency bound of a sum whose components are each within `err` of a model value of magnitude `mag`, plus the float rounding
    of the host formula's result near f"""
    return math.asin(min(1.0, math.sqrt(2.0) * err / mag)) * fs / (2.0 * math.pi) + abs(f) * U


@pytest.mark.parametrize("f", [1234.0, -2500.0])
def test_an_unmodulated_carrier_reads_its_offset_in_every_block(gpu, f):
    """Bound, derived: the device's block is within REL W per component of the model's (above), so its argument is within
    asin(sqrt(2) REL W / |A|) of the model's; and the model, fed the carrier ROUNDED to fp32, is within 2 u rad of 2 pi f / fs -- a
    sample's rounding moves its phase by at most u (|dx| <= u |x|), a product of two by at most 2 u, and a sum of vectors that each
    point within 2 u of one direction points within 2 u of it.  Times fs / 2 pi: about 0.9 Hz at 200 ksps."""
    fs, a, n = 200e3, 0.37, 256 * 12
    y = (a * np.exp(2j * np.pi * f * np.arange(n) / fs + 0.4j)).astype(np.complex64)[None, :]
    with _iq(1, n) as r:
        r.push_iq(y[:, :1000])
        r.push_iq(y[:, 1000:])
        got, first = r.channel_autocorr()
    want, w = _check(got, y)
    assert first == 0 and got.shape == (1, 12)
    worst = 0.0
    for j in range(12):
        bound = _angle_bound_hz(REL * w[0, j], abs(want[0, j]), fs, f) + 2.0 * U * fs / (2.0 * math.pi)
        assert 0.5 < bound < 1.0
        hz = sor.offset_hz(got[0, j], 10)
        worst = max(worst, abs(hz - f))
        assert abs(hz - f) <= bound, (j, hz, bound)
    assert abs(abs(got[0, 5]) / (a * a) - 1.0) < 1e-4                # a^2 e^(j 2 pi f / fs)
    print("\ncarrier at %+g Hz: worst |block estimate - f| = %.4f Hz" % (f, worst))


def _burst_bounds(model_row, w_row, pos, sps, f):
    """(model offset, count, Hz bound of the device's offset against the model's) for one record"""
    j0, cnt = sor.burst_window(pos, sps)
    total = complex(np.sum(model_row[j0:j0 + cnt]))
    err = REL * float(np.sum(w_row[j0:j0 + cnt])) + cnt * U * float(np.sum(np.abs(model_row[j0:j0 + cnt].real) + np.abs(model_row[j0:j0 + cnt].imag)))
    return sor.offset_hz(total, sps), cnt, _angle_bound_hz(err, abs(total), 20000.0 * sps, f)


def _host_formula(total, sps):
    return np.float32(math.atan2(float(total.imag), float(total.real)) * (20000.0 * sps) / (2.0 * math.pi))


def _offset_checks(r, recs, y, sps, sent):
    """burst_autocorr / burst_offset of one record against the model on the samples y the seam sliced"""
    total, cnt = r.burst_autocorr(recs)
    hz, cnt2 = r.burst_offset(recs)
    assert total.dtype == np.complex64 and hz.dtype == np.float32 and cnt.dtype == np.uint32 and len(recs) == 1
    g = recs[0]
    ch, pos = int(g["channel"]), int(g["position"])
    model, w = sor.blocks(y)[ch], sor.weights(y)[ch]
    want, wcnt, bound = _burst_bounds(model, w, pos, sps, sent)
    assert wcnt in (3374 * sps // 256, 3374 * sps // 256 - 1) and int(cnt[0]) == int(cnt2[0]) == wcnt
    print("\nchannel %d at %d: sent %+g Hz, device %+.3f Hz, model %+.3f Hz (bound %.3f), n = %d" % (ch, pos, sent, hz[0], want, bound, wcnt))
    assert abs(float(hz[0]) - want) <= bound
    # the host formula on the device's own sums, to its float rounding
    mine = _host_formula(total[0], sps)
    assert abs(float(hz[0]) - float(mine)) <= float(np.spacing(np.abs(mine)))
    return float(hz[0])


CFO = 1500.0


@functools.lru_cache(maxsize=None)
def _burst200():
    """one burst 1500 Hz above the centre over noise 30 dB down, 200 ksps"""
    n = 44000
    iq, truth = synth.make_channel_block(n, 1, seed=9100, sps=10, snr_db=30.0, first=2000, cfo_hz=CFO)
    assert len(truth) == 1
    y = (iq * np.float32(0.5)).astype(np.complex64)
    y.setflags(write=False)
    return y, truth


def test_burst_offset_on_the_iq_seam(gpu):
    y, truth = _burst200()
    n = y.size
    rows = np.stack([_noise(42, n, 0.01), y])                        # the mobile is on channel 1
    with _iq(2, n) as r:
        r.push_iq(np.ascontiguousarray(rows[:, :17001]))
        r.push_iq(np.ascontiguousarray(rows[:, 17001:]))
        recs = r.drain()
        assert [(int(g["channel"]), g["min"].decode()) for g in recs] == [(1, truth[0][2])]
        hz = _offset_checks(r, recs, rows[:, :n // 64 * 64], 10, CFO)
        assert abs(hz - CFO) <= 14.0                                 # twice the CPU table's 7 Hz at 10 samples per symbol and 30 dB
        bad = recs.copy()
        bad["channel"][0] = 2                                        # channel = n_channels
        for call in (r.burst_autocorr, r.burst_offset):
            with pytest.raises(capi.AmpsError) as e:
                call(bad)
            assert e.value.code == -22
        assert r.burst_autocorr(recs[:0])[0].shape == (0,) and r.burst_offset(recs[:0])[0].shape == (0,)


FILTER_SEED = 9200                                                   # scripts/offset_estimator_cpu.py measured these very bursts
# cut-off of the channel filter -> |estimate - sent| of the CPU measurement at +1500 Hz, 30 dB, 2.4 Msps / 12.  Behind the
# default filter the estimate is not merely low: the filter cuts the side of the signal the offset moved outwards, the amplitude-weighted
# sum leans to the other side, and the figure comes out at -475 Hz.  The bound says how wrong it may be, as measured; the 16 kHz case is
# the one a retune loop can steer by.
FILTER_ERR_HZ = {10e3: 1975.0, 16e3: 64.0}


@pytest.mark.parametrize("cutoff", sorted(FILTER_ERR_HZ))
def test_burst_offset_behind_the_channel_filter(gpu, cutoff):
    fs, decim, fc = 2.4e6, 12, 615e3
    centres = [-1.05e6, fc, 15e3]
    n = 4000 * decim + (3374 + 300) * 10 * decim
    iq, truth = synth.make_channel_block(n, 1, seed=FILTER_SEED, sps=10 * decim, snr_db=30.0 - 10.0 * np.log10(decim), first=2000 * decim, cfo_hz=CFO)
    assert len(truth) == 1
    x = (iq * np.exp(2j * np.pi * fc * np.arange(n) / fs)).astype(np.complex64)
    cuts = _cuts([200003, n - 200003])
    with capi.Recc(n_channels=3, sps=10, max_samples=n // decim, max_bursts=16) as twin, \
         capi.Recc(n_channels=3, sps=10, max_samples=n // decim, max_bursts=16, stream_offset=True) as r:
        twin.set_xlate_shared(fs, centres, decim, cutoff_hz=cutoff)
        r.set_xlate_shared(fs, centres, decim, cutoff_hz=cutoff)
        ys = []
        for a, b in cuts:
            ys.append(twin.debug_xlate_shared(x[a:b]))
            r.push_raw_shared(x[a:b])
        recs = r.drain()
        assert [(int(g["channel"]), g["min"].decode()) for g in recs] == [(1, truth[0][2])]
        y = np.concatenate(ys, axis=1)
        hz = _offset_checks(r, recs, y[:, :y.shape[1] // 64 * 64], 10, CFO)
    assert abs(hz - CFO) <= 1.5 * FILTER_ERR_HZ[cutoff]


# ---- 6. the burst sum is the stated reduction of the ring, bit for bit, across the ring's wrap
def test_burst_sums_are_the_stated_reduction_of_the_ring_bit_for_bit(gpu):
    """amps_recc_burst_autocorr against streamoffsetref.gather_sum on the very values amps_recc_channel_autocorr returns: no tolerance.
    The records are fabricated (the entry point takes any channel and position); held and unheld ones alternate in one call."""
    C, sps, push, pushes = 3, 12, 4096, 27
    y = _noise_plus_tone(48, C, push * pushes)
    with _iq(C, push, sps=sps) as r:
        assert r.autocorr_ring_blocks == 256                         # R = 65536: the smallest power of two >= 4096 + 12 * 3586 + 1024
        for a in range(0, y.shape[1], push):
            r.push_iq(np.ascontiguousarray(y[:, a:a + push]))
        ring, lo = r.channel_autocorr()
        # position -> (first block, blocks): 158 blocks from 200 cross slot 255 -> 0 and give three values to the first lanes; 157 is
        # the other count class; block 172 has left the window; block 469 is not produced yet
        cases = {51200: (200, 158), 44000: (172, 0), 51201: (201, 157), 80000: (313, 0)}
        recs = np.zeros(len(cases) * C, capi.BURST_DTYPE)
        recs["position"] = np.repeat(list(cases), C)
        recs["channel"] = np.tile(np.arange(C), len(cases))
        total, cnt = r.burst_autocorr(recs)
        hz, cnt2 = r.burst_offset(recs)
    assert lo == 176 and ring.shape == (C, 256)                      # 110 592 samples: blocks [176, 432) are held
    assert np.array_equal(cnt, cnt2)
    held = 0
    for g, t, c, f in zip(recs, total, cnt, hz):
        j0, count = cases[int(g["position"])]
        assert j0 == (int(g["position"]) + 255) // 256 and int(c) == count, (g["position"], int(c))
        if count == 0:                                               # {0, 0}, 0 and an offset of 0.0: not held is not an error
            assert not _bits(t).any() and np.float32(f).view(np.uint32) == 0
            continue
        assert count == spr.burst_window(int(g["position"]), sps)[1] and j0 < 256 < j0 + count
        re, im = sor.gather_sum(ring[int(g["channel"]), j0 - lo:j0 - lo + count])
        print("\nchannel %d at %d: %d blocks, sum %.9g %+.9gj, stated reduction %.9g %+.9gj" % (g["channel"], g["position"], count, t.real, t.imag, re, im))
        assert np.float32(t.real).view(np.uint32) == re.view(np.uint32) and np.float32(t.imag).view(np.uint32) == im.view(np.uint32)
        mine = _host_formula(t, sps)
        assert abs(float(f) - float(mine)) <= float(np.spacing(np.abs(mine)))
        held += 1
    assert held == 2 * C


def test_a_capture_that_has_left_a_small_ring_reads_nothing(gpu):
    y, truth = _burst200()
    n = y.size
    rows = np.stack([_noise(42, n, 0.01), y])
    with _iq(2, n, max_samples=4096) as r:
        R = r.autocorr_ring_blocks * 256
        assert R == 65536
        for a in range(0, n, 4096):
            r.push_iq(np.ascontiguousarray(rows[:, a:a + 4096]))
        recs = r.drain()
        assert [(int(g["channel"]), g["min"].decode()) for g in recs] == [(1, truth[0][2])]
        total, cnt = r.burst_autocorr(recs)
        assert int(cnt[0]) in (130, 131) and total[0] != 0           # still held
        zeros = np.zeros((2, 4096), np.complex64)
        for _ in range(R // 4096):
            r.push_iq(zeros)
        total, cnt = r.burst_autocorr(recs)
        hz, cnt2 = r.burst_offset(recs)
        assert not cnt.any() and not cnt2.any() and not _bits(total).any() and not hz.view(np.uint32).any()


def test_a_record_drained_behind_later_pushes_still_has_its_sums(gpu):
    y, truth = _burst200()
    lead = 70000                                                     # the burst lies beyond one span of the ring (65536)
    x = np.concatenate([_noise(46, lead, 0.01), y, _noise(47, 8192, 0.01)])[None, :]
    n = x.shape[1]
    with _iq(1, n, max_samples=8192) as r:
        slots = r.autocorr_ring_blocks
        assert slots * 256 == 65536
        edge = lead + y.size
        for a in range(0, edge, 8192):
            r.push_iq(np.ascontiguousarray(x[:, a:min(a + 8192, edge)]))
        r.drain_begin()
        r.push_iq(np.ascontiguousarray(x[:, edge:]))                 # streaming use: the next push is enqueued before the drain ends
        recs = r.drain_end()
        assert [g["min"].decode() for g in recs] == [truth[0][2]] and int(recs[0]["position"]) > 65536
        _, first = r.channel_autocorr()
        assert first == n // 64 * 64 // 256 - slots > 0
        hz = _offset_checks(r, recs, x[:, :n // 64 * 64], 10, CFO)
    assert abs(hz - CFO) <= 14.0


# ---- 7. off means off, and on changes nothing else
def test_off_means_off_and_on_changes_nothing_else(gpu):
    L = capi.load()
    with _iq(4, 4096, stream_offset=False) as r:
        out, cnt = np.zeros((4, 1), np.complex64), np.zeros(1, np.uint32)
        recs = np.zeros(1, capi.BURST_DTYPE)
        r.push_iq(_noise(1, (4, 4096)))
        assert L.amps_recc_channel_autocorr(r._h, 0, 0, None, 0, None, None) == -38                    # -ENOSYS
        assert L.amps_recc_channel_autocorr(r._h, 0, 1, out.ctypes.data, 1, None, None) == -38
        assert L.amps_recc_burst_autocorr(r._h, recs.ctypes.data, 1, out.ctypes.data, cnt.ctypes.data) == -38
        assert L.amps_recc_burst_offset(r._h, recs.ctypes.data, 1, out.ctypes.data, cnt.ctypes.data) == -38
    with _iq(4, 4096, stream_offset=False, stream_power=True) as r:                                    # the power flag does not bring it
        assert L.amps_recc_channel_autocorr(r._h, 0, 0, None, 0, None, None) == -38
    wb = {"channels": 1024, "decim": 512, "taps_per_branch": 8, "first_channel": 96}
    for kw in (dict(n_channels=832, sps=3, max_samples=256, wideband=wb),
               dict(n_channels=832, sps=3, max_samples=256, unfused_wideband=True, wideband=wb),
               dict(n_channels=832, sps=3, max_samples=256, channel_power=True, wideband=wb),
               dict(n_channels=4, sps=10, max_samples=0),                                              # the symbol seam only
               dict(n_channels=4, sps=10, max_samples=4096, channel_power=True)):
        with pytest.raises(capi.AmpsError) as e:
            capi.Recc(max_bursts=16, stream_offset=True, **kw)
        assert e.value.code == -22, kw
    # the records of a two-burst stream with the flag off and on, and the power values with and without it
    n = 90000
    iq, truth = synth.make_channel_block(n, 2, seed=44, sps=10, snr_db=30.0, first=2000)
    assert len(truth) == 2
    rows = np.stack([iq, _noise(45, n, 0.03)])
    got, power = [], []
    for kw in (dict(stream_offset=False), dict(stream_offset=True), dict(stream_offset=False, stream_power=True), dict(stream_offset=True, stream_power=True)):
        with _iq(2, n, **kw) as r:
            r.push_iq(np.ascontiguousarray(rows[:, :33333]))
            r.push_iq(np.ascontiguousarray(rows[:, 33333:]))
            got.append(r.drain())
            if kw.get("stream_power"):
                power.append((r.channel_power()[0], r.burst_power(got[-1])[0]))
            if kw["stream_offset"]:
                hz, cnt = r.burst_offset(got[-1])
                assert cnt.all() and np.all(np.abs(hz) <= 14.0)      # both mobiles on their centre
    assert len(got[0]) == 2 and all(g.tobytes() == got[0].tobytes() for g in got[1:])
    assert power[0][0].size and np.array_equal(power[0][0].view(np.uint32), power[1][0].view(np.uint32))
    assert np.array_equal(power[0][1].view(np.uint32), power[1][1].view(np.uint32))
