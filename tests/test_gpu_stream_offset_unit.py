"""-m gpu: the unit-amplitude carrier-offset statistic of the IQ and translate seams (AMPS_RECC_FLAG_STREAM_OFFSET_UNIT, behind
amps_recc_channel_autocorr, amps_recc_burst_autocorr, amps_recc_burst_offset) against the float64 model tests/streamoffsetunitref.py.

Tolerance of a block, derived and not measured (include/amps_recc.h states the same).  A term u(s) = p / |p|: p carries at most 2 u |p|
(u = 2^-24: the product's rounding and the fma's), the normalisation about 4 u more (m's two roundings halved by the root, the root's
1 ulp, one multiply), so a term is within about 6 u of the exact unit vector; adding 256 terms of magnitude <= 1 carries at most 255 u
times the sum of their magnitudes <= 256; times 2^-8: each component of U within 261 u = 1.56e-5 of the model's, ABSOLUTE.  The checks
use ABS = 2e-5, the figure of the shipped statistic's tests, against float64 on the very fp32 samples the seam sliced.  The device's
reciprocal square root is not correctly rounded, so against the model this is a bound and not bit equality; between two runs of the
device on the same stream it is bit equality.

Tolerance of an angle: both components within E of a model value of magnitude |S| put the argument within asin(sqrt(2) E / |S|) of
the model's (test_gpu_stream_offset._angle_bound_hz).  For a burst sum E = count * ABS plus the gather's own additions.

Bounds against what was SENT come from the CPU measurement alone (scripts/offset_unit_estimator_cpu.py,
profiles/stream_offset_unit/estimator_cpu.txt): the model's error at the tested point times 1.5."""
import math

import numpy as np
import pytest

import streamoffsetunitref as sur
from gr_amps_amd import capi, synth
from test_gpu_stream_offset import CFO, FILTER_SEED, U, _angle_bound_hz, _bits, _burst200, _host_formula, _noise, _noise_plus_tone
from test_gpu_stream_power import PIECES, XL, _configure, _cuts, _ints

pytestmark = pytest.mark.gpu

ABS = 2e-5
# |model - sent| at 2.4 Msps / 12 behind the default 10 kHz filter, +1500 Hz, 30 dB: 4.8 Hz in estimator_cpu.txt (3), rounded up;
# tests/test_cpu_stream_offset_unit.py holds the model to it
FILTER_UNIT_ERR_HZ = 5.0
IQ_UNIT_ERR_HZ = 2.0                                                 # the IQ-seam table at 10 samples per symbol and 30 dB


def _check(got, y, origin=0, cols=slice(None)):
    """every component of every block within ABS of the model on the same samples"""
    want = sur.blocks(y, origin=origin)[:, cols]
    assert got.shape == want.shape and got.dtype == np.complex64, (got.shape, want.shape)
    assert want.size
    err = np.maximum(np.abs(got.real.astype(np.float64) - want.real), np.abs(got.imag.astype(np.float64) - want.imag))
    print("\nworst component error = %.3g (bound %.3g) over %d blocks" % (err.max(), ABS, want.size))
    assert np.all(err <= ABS), np.unravel_index(np.argmax(err), err.shape)
    return want


def _iq(C, n, **kw):
    return capi.Recc(n_channels=C, sps=kw.pop("sps", 10), max_samples=kw.pop("max_samples", n), max_bursts=kw.pop("max_bursts", 16),
                     stream_offset=kw.pop("stream_offset", "unit"), **kw)


# ---- 1. the IQ seam, ragged pushes
@pytest.mark.parametrize("C", [5, 66])
def test_iq_seam_blocks_equal_the_model_however_the_stream_is_cut(gpu, C):
    import torch
    n = sum(PIECES)
    y = _noise_plus_tone(300 + C, C, n)
    with _iq(C, n) as r:
        r.push_iq(y)
        one, first = r.channel_autocorr()
    assert first == 0 and one.shape == (C, 23)
    _check(one, y[:, :n // 64 * 64])
    assert np.all(np.abs(one) <= 1.0 + ABS)

    done = [int(e) // 64 * 64 for _, e in _cuts(PIECES)]            # n_done after each push: whole 64-sample words of what has arrived

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
                seen.append(r.channel_autocorr()[0].shape[1])        # waits for the push: the device block is the caller's until then
            assert seen == [d // 256 for d in done]                  # block j exists once 256 (j + 1) <= produced
            return r.channel_autocorr()[0]

    assert np.array_equal(_bits(ragged(False)), _bits(one))
    assert np.array_equal(_bits(ragged(True)), _bits(one))


def test_pushes_that_begin_on_a_block_edge_take_the_predecessor_from_the_carry(gpu):
    """launches that begin at s = 256 j read sample 256 j - 1 through lane 0's extra load, from the carry"""
    C, pieces = 3, [256, 64, 192, 512, 320, 704]
    n = sum(pieces)
    y = _noise_plus_tone(78, C, n)
    with _iq(C, n) as r:
        r.push_iq(y)
        one, _ = r.channel_autocorr()
    with _iq(C, n) as r:
        for a, b in _cuts(pieces):
            r.push_iq(np.ascontiguousarray(y[:, a:b]))
        cut, _ = r.channel_autocorr()
    _check(one, y)
    assert one.shape == (C, n // 256) and np.array_equal(_bits(cut), _bits(one))


# ---- 2. the origin: the product with y[origin - 1] = 0 is a zero TERM, and the divisor stays 2^8
@pytest.mark.parametrize("origin,first_block", [(960, 4), (1024, 4)])
def test_origin_and_the_zero_term_in_front_of_the_stream(gpu, origin, first_block):
    C, n = 3, 2048 + 64
    f, fs = 3000.0, 200e3
    y = np.tile((0.8 * np.exp(2j * np.pi * f * np.arange(n) / fs)).astype(np.complex64), (C, 1)) * np.float32([0.5, 1.0, 2.0])[:, None]
    with _iq(C, n) as r:
        r.set_origin(origin)
        r.push_iq(y[:, :777])
        r.push_iq(y[:, 777:])
        got, first = r.channel_autocorr()
    assert first == first_block and got.shape[1] == (origin + n) // 256 - first_block
    want = _check(got, y, origin=origin)
    # a clean carrier: every block is e^(j 2 pi f / fs) whatever the amplitude -- but for the block that begins AT the origin, whose first
    # term is (0, 0) and which is still divided by 256
    full = np.exp(2j * np.pi * f / fs)
    head = 255.0 / 256.0 if origin % 256 == 0 else 1.0
    assert np.all(np.abs(want[:, 0] - head * full) < 1e-6) and np.all(np.abs(want[:, 1:] - full) < 1e-6)
    assert np.all(np.abs(got[:, 0] - head * full) < 1e-6 + 2 * ABS)


# ---- 3. the ring
def test_three_turns_of_a_64_slot_ring(gpu):
    C, sps, push, n = 2, 3, 1000, 50000
    y = _noise_plus_tone(12, C, n)
    with _iq(C, n, sps=sps, max_samples=1024) as r:
        slots = r.autocorr_ring_blocks
        assert slots == 64
        for a in range(0, n, push):
            r.push_iq(np.ascontiguousarray(y[:, a:a + push]))
        got, first = r.channel_autocorr()
        out = np.zeros((C, 1), np.complex64)
        assert capi.load().amps_recc_channel_autocorr(r._h, first - 1, 1, out.ctypes.data, 1, None, None) == -34     # -ERANGE
    produced = n // 64 * 64
    assert produced > 3 * 64 * 256 and first == produced // 256 - slots and got.shape == (C, slots)
    _check(got, y[:, :produced], cols=slice(first, first + slots))


def test_all_zero_rows_and_non_finite_samples(gpu):
    """a silent row reads exactly (0, 0); a sample that is not finite takes the two products it is part of out of the sum, and nothing else"""
    C, n = 3, 1024
    y = _noise_plus_tone(13, C, n)
    y[1] = 0
    y[2, 300] = np.complex64(complex(np.inf, 1.0))
    y[2, 700] = np.complex64(complex(np.nan, 0.0))
    y[2, 900] = np.complex64(complex(3e38, 3e38))                    # finite, its products are not
    y[2, 901] = np.complex64(complex(3e38, -3e38))
    with _iq(C, n) as r:
        r.push_iq(y[:, :300])
        r.push_iq(y[:, 300:])
        got, _ = r.channel_autocorr()
    assert got.shape == (C, 4) and not _bits(got[1]).any()
    assert np.isfinite(got.view(np.float32)).all()
    _check(got, y)
    u = sur.units(y[2])[0]
    assert not u[300] and not u[301] and not u[700] and not u[701] and not u[901] and u[299] and u[302]


# ---- 4. the translate seams: the sums of what the stage delivers
@pytest.mark.parametrize("name", ["400k_d2_fc32", "2400k_d12_cu8", "2048k_5_64_cu8"])
def test_translate_seams_report_the_sums_of_the_stage_output(gpu, name):
    cfg, C, sps, n, fmt, nmax = XL[name]
    x = _noise(21, n, 0.5) if fmt == capi.SAMPLES_FC32 else _ints(fmt, n, 22)
    cuts = _cuts([n // 3 + 17, 5, n - n // 3 - 22])                  # ragged, one piece shorter than any decimation
    with capi.Recc(n_channels=C, sps=sps, max_samples=nmax, max_bursts=16) as twin, \
         capi.Recc(n_channels=C, sps=sps, max_samples=nmax, max_bursts=16, stream_offset="unit") as r:
        _configure(twin, cfg)
        _configure(r, cfg)
        ys = []
        for a, b in cuts:
            if fmt == capi.SAMPLES_FC32:
                ys.append(twin.debug_xlate_shared(x[a:b]))
                r.push_raw_shared(x[a:b])
            else:
                ys.append(twin.debug_xlate_shared_as(x[a:b], fmt))
                r.push_raw_shared_as(x[a:b], fmt)
        got, first = r.channel_autocorr()
    y = np.concatenate(ys, axis=1)
    produced = y.shape[1] // 64 * 64
    assert first == 0 and produced > 7000 and got.shape == (C, produced // 256)
    _check(got, y[:, :produced])


def test_an_sc16_stream_and_its_fc32_conversion_give_the_same_bits(gpu):
    cfg, C, sps, n, _, nmax = XL["2400k_d12_cu8"]
    q = _ints(capi.SAMPLES_SC16, n, 23)
    xf = capi.convert_samples(q, capi.SAMPLES_SC16)
    A = []
    for fmt, data in ((capi.SAMPLES_SC16, q), (capi.SAMPLES_FC32, xf)):
        with capi.Recc(n_channels=C, sps=sps, max_samples=nmax, max_bursts=16, stream_offset="unit") as r:
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
@pytest.mark.parametrize("f", [1234.0, -2500.0])
def test_an_unmodulated_carrier_reads_its_offset_in_every_block(gpu, f):
    """Bound, derived: each component of the device's block is within ABS of the model's, whose magnitude is 1 (255 / 256 in the first
    block), so its argument is within asin(sqrt(2) ABS / |U|) of the model's; the model, fed the carrier ROUNDED to fp32, is within
    2 u rad of 2 pi f / fs (test_gpu_stream_offset).  Times fs / 2 pi: 0.9 Hz at 200 ksps."""
    fs, a, n = 200e3, 0.37, 256 * 12
    y = (a * np.exp(2j * np.pi * f * np.arange(n) / fs + 0.4j)).astype(np.complex64)[None, :]
    with _iq(1, n) as r:
        r.push_iq(y[:, :1000])
        r.push_iq(y[:, 1000:])
        got, first = r.channel_autocorr()
    want = _check(got, y)
    assert first == 0 and got.shape == (1, 12)
    worst = 0.0
    for j in range(12):
        bound = _angle_bound_hz(ABS, abs(want[0, j]), fs, f) + 2.0 * U * fs / (2.0 * math.pi)
        assert 0.5 < bound < 1.0
        hz = sur.offset_hz(got[0, j], 10)
        worst = max(worst, abs(hz - f))
        assert abs(hz - f) <= bound, (j, hz, bound)
    assert abs(abs(got[0, 5]) - 1.0) < 2 * ABS                       # e^(j 2 pi f / fs): the amplitude is gone
    print("\ncarrier at %+g Hz: worst |block estimate - f| = %.4f Hz" % (f, worst))


def test_the_normalisation_does_not_need_the_squares_to_fit_fp32(gpu):
    """carriers of amplitude 1e-15 and 3e15: the products (1e-30, 9e30) are normal fp32 numbers, re^2 + im^2 of them (1e-60, 8e61)
    is not.  Both rows read the same unit phasor"""
    fs, f, n = 200e3, 1234.0, 1024
    amps = np.array([1e-15, 3e15], np.float64)
    y = (amps[:, None] * np.exp(2j * np.pi * f * np.arange(n) / fs)[None, :]).astype(np.complex64)
    with _iq(2, n) as r:
        r.push_iq(y)
        got, _ = r.channel_autocorr()
    want = _check(got, y)
    full = np.exp(2j * np.pi * f / fs)
    assert np.all(np.abs(want[:, 1:] - full) < 1e-6)                # the model itself: the rounding of y to fp32 is relative
    assert np.all(np.abs(got[:, 1:] - full) < 1e-6 + 2 * ABS)


def _offset_checks(r, recs, y, sps, sent):
    """burst_autocorr / burst_offset of one record against the model on the samples y the seam sliced.  Bound from ABS: each of the
    `count` blocks is within ABS per component, the gather's additions within count * u * sum(|re U_j| + |im U_j|); the angle by the
    disc of that radius around the model's sum"""
    total, cnt = r.burst_autocorr(recs)
    hz, cnt2 = r.burst_offset(recs)
    assert total.dtype == np.complex64 and hz.dtype == np.float32 and len(recs) == 1
    ch, pos = int(recs[0]["channel"]), int(recs[0]["position"])
    model = sur.blocks(y)[ch]
    j0, count = sur.burst_window(pos, sps)
    want_sum = complex(np.sum(model[j0:j0 + count]))
    err = count * ABS + count * U * float(np.sum(np.abs(model[j0:j0 + count].real) + np.abs(model[j0:j0 + count].imag)))
    want, bound = sur.offset_hz(want_sum, sps), _angle_bound_hz(err, abs(want_sum), 20000.0 * sps, sent)
    assert int(cnt[0]) == int(cnt2[0]) == count
    coh = sur.coherence(total[0], count)
    print("\nchannel %d at %d: sent %+g Hz, device %+.3f Hz, model %+.3f Hz (bound %.3f), n = %d, coherence %.3f" % (ch, pos, sent, hz[0], want, bound, count, coh))
    assert bound < 5.0                                               # "a few Hz"
    assert abs(float(hz[0]) - want) <= bound
    assert 0.0 < coh <= 1.0 + ABS
    mine = _host_formula(total[0], sps)
    assert abs(float(hz[0]) - float(mine)) <= float(np.spacing(np.abs(mine)))
    return float(hz[0])


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
    assert abs(hz - CFO) <= 1.5 * IQ_UNIT_ERR_HZ


def test_burst_offset_behind_the_default_channel_filter(gpu):
    """the case the shipped statistic reads as -475 Hz: 2.4 Msps / 12, the default 10 kHz cut-off, a burst +1500 Hz off at 30 dB"""
    fs, decim, fc = 2.4e6, 12, 615e3
    centres = [-1.05e6, fc, 15e3]
    n = 4000 * decim + (3374 + 300) * 10 * decim
    iq, truth = synth.make_channel_block(n, 1, seed=FILTER_SEED, sps=10 * decim, snr_db=30.0 - 10.0 * np.log10(decim), first=2000 * decim, cfo_hz=CFO)
    assert len(truth) == 1
    x = (iq * np.exp(2j * np.pi * fc * np.arange(n) / fs)).astype(np.complex64)
    with capi.Recc(n_channels=3, sps=10, max_samples=n // decim, max_bursts=16) as twin, \
         capi.Recc(n_channels=3, sps=10, max_samples=n // decim, max_bursts=16, stream_offset="unit") as r:
        twin.set_xlate_shared(fs, centres, decim)
        r.set_xlate_shared(fs, centres, decim)
        ys = []
        for a, b in _cuts([200003, n - 200003]):
            ys.append(twin.debug_xlate_shared(x[a:b]))
            r.push_raw_shared(x[a:b])
        recs = r.drain()
        assert [(int(g["channel"]), g["min"].decode()) for g in recs] == [(1, truth[0][2])]
        y = np.concatenate(ys, axis=1)
        hz = _offset_checks(r, recs, y[:, :y.shape[1] // 64 * 64], 10, CFO)
    assert abs(hz - CFO) <= 1.5 * FILTER_UNIT_ERR_HZ


# ---- 6. the burst sum is the stated reduction of the ring, bit for bit, across the ring's wrap
def test_burst_sums_are_the_stated_reduction_of_the_ring_bit_for_bit(gpu):
    C, sps, push, pushes = 3, 12, 4096, 27
    y = _noise_plus_tone(49, C, push * pushes)
    with _iq(C, push, sps=sps) as r:
        assert r.autocorr_ring_blocks == 256
        for a in range(0, y.shape[1], push):
            r.push_iq(np.ascontiguousarray(y[:, a:a + push]))
        ring, lo = r.channel_autocorr()
        cases = {51200: (200, 158), 44000: (172, 0), 51201: (201, 157), 80000: (313, 0)}     # as the shipped statistic's test
        recs = np.zeros(len(cases) * C, capi.BURST_DTYPE)
        recs["position"] = np.repeat(list(cases), C)
        recs["channel"] = np.tile(np.arange(C), len(cases))
        total, cnt = r.burst_autocorr(recs)
    assert lo == 176 and ring.shape == (C, 256)
    held = 0
    for g, t, c in zip(recs, total, cnt):
        j0, count = cases[int(g["position"])]
        assert int(c) == count
        if count == 0:
            assert not _bits(t).any()
            continue
        assert j0 < 256 < j0 + count                                 # across slot 255 -> 0
        re, im = sur.gather_sum(ring[int(g["channel"]), j0 - lo:j0 - lo + count])
        assert np.float32(t.real).view(np.uint32) == re.view(np.uint32) and np.float32(t.imag).view(np.uint32) == im.view(np.uint32)
        held += 1
    assert held == 2 * C


# ---- 7. off means off, one statistic per handle, and on changes nothing else
def test_off_means_off_and_on_changes_nothing_else(gpu, monkeypatch):
    L = capi.load()
    with _iq(4, 4096, stream_offset=False) as r:
        out, cnt = np.zeros((4, 1), np.complex64), np.zeros(1, np.uint32)
        recs = np.zeros(1, capi.BURST_DTYPE)
        r.push_iq(_noise(1, (4, 4096)))
        assert L.amps_recc_channel_autocorr(r._h, 0, 0, None, 0, None, None) == -38                    # -ENOSYS
        assert L.amps_recc_burst_autocorr(r._h, recs.ctypes.data, 1, out.ctypes.data, cnt.ctypes.data) == -38
        assert L.amps_recc_burst_offset(r._h, recs.ctypes.data, 1, out.ctypes.data, cnt.ctypes.data) == -38
    wb = {"channels": 1024, "decim": 512, "taps_per_branch": 8, "first_channel": 96}
    for kw in (dict(n_channels=832, sps=3, max_samples=256, wideband=wb),
               dict(n_channels=4, sps=10, max_samples=0),                                              # the symbol seam only
               dict(n_channels=4, sps=10, max_samples=4096, channel_power=True)):
        with pytest.raises(capi.AmpsError) as e:
            capi.Recc(max_bursts=16, stream_offset="unit", **kw)
        assert e.value.code == -22, kw
    with pytest.raises(ValueError):
        capi.Recc(n_channels=4, sps=10, max_samples=4096, stream_offset="units")
    # both offset flags in one cfg: a handle keeps one ring with one statistic
    with monkeypatch.context() as m:
        m.setattr(capi, "FLAG_STREAM_OFFSET_UNIT", capi.FLAG_STREAM_OFFSET_UNIT | capi.FLAG_STREAM_OFFSET)
        with pytest.raises(capi.AmpsError) as e:
            capi.Recc(n_channels=4, sps=10, max_samples=4096, stream_offset="unit")
        assert e.value.code == -22
    # the records of a two-burst stream with the flag off and on, and the power values with and without it
    n = 90000
    iq, truth = synth.make_channel_block(n, 2, seed=44, sps=10, snr_db=30.0, first=2000)
    assert len(truth) == 2
    rows = np.stack([iq, _noise(45, n, 0.03)])
    got, power = [], []
    for kw in (dict(stream_offset=False), dict(stream_offset="unit"), dict(stream_offset=False, stream_power=True), dict(stream_offset="unit", stream_power=True)):
        with _iq(2, n, **kw) as r:
            r.push_iq(np.ascontiguousarray(rows[:, :33333]))
            r.push_iq(np.ascontiguousarray(rows[:, 33333:]))
            got.append(r.drain())
            if kw.get("stream_power"):
                power.append((r.channel_power()[0], r.burst_power(got[-1])[0]))
            if kw["stream_offset"]:
                hz, cnt = r.burst_offset(got[-1])
                assert cnt.all() and np.all(np.abs(hz) <= 1.5 * IQ_UNIT_ERR_HZ)      # both mobiles on their centre
    assert len(got[0]) == 2 and all(g.tobytes() == got[0].tobytes() for g in got[1:])
    assert power[0][0].size and np.array_equal(power[0][0].view(np.uint32), power[1][0].view(np.uint32))
    assert np.array_equal(power[0][1].view(np.uint32), power[1][1].view(np.uint32))


def test_the_two_statistics_differ_and_share_the_ring_rules(gpu):
    """the same stream through a handle of each flag: same shape, same numbering, different values (so the flag reaches the kernel)"""
    C, n = 2, 2048
    y = _noise_plus_tone(50, C, n)
    got = []
    for mode in (True, "unit"):
        with _iq(C, n, stream_offset=mode) as r:
            r.push_iq(y)
            got.append(r.channel_autocorr())
    assert got[0][1] == got[1][1] == 0 and got[0][0].shape == got[1][0].shape == (C, 8)
    assert np.all(np.abs(got[1][0]) <= 1.0 + ABS) and np.abs(got[0][0] - got[1][0]).min() > 100 * ABS
