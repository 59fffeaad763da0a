"""-m gpu: per-channel received power of the IQ and translate seams (AMPS_RECC_FLAG_STREAM_POWER: amps_recc_channel_power,
amps_recc_burst_power on a handle without a filter bank) against the float64 model tests/streampowerref.py.

Tolerance, derived and not measured.  A block is a sum of 256 non-negative fp32 terms fma(im, im, re * re): each term carries at most
2 u (the product's rounding and the fma's), u = 2^-24, and adding 256 of them carries at most 255 u more whatever the order, since
nothing cancels: |P_gpu - P_ref| <= 257 u P_ref = 1.54e-5 P_ref.  The checks use REL = 2e-5 per block, against float64 on the very fp32
samples the seam sliced.  A burst's mean adds 3 + 6 additions and one division to at most that: 267 u, under the same bound.

The origin case uses 960, not 1000: amps_recc_set_origin takes multiples of 64 only, and 960 is the one whose window also starts at
block 4 with a block edge (1024) that is not the origin."""
import functools

import numpy as np
import pytest

import gatherref
import oracle
import streampowerref as spr
from gr_amps_amd import capi, synth

pytestmark = pytest.mark.gpu

REL = 2e-5
PIECES = [1, 63, 200, 1000, 37, 2500, 5, 700, 130, 1364]              # 6000 samples; the 1 and the 5 process no word (P == 0)


def _noise(seed, shape, scale=1.0):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * scale).astype(np.complex64)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(got, want):
    """every block within REL of the model, relative"""
    assert got.shape == want.shape and got.dtype == np.float32, (got.shape, want.shape)
    assert want.size and want.min() > 0
    err = np.abs(got.astype(np.float64) - want) / want
    print("\nworst |P_gpu - P_ref| / P_ref = %.3g (bound %.3g) over %d blocks" % (err.max(), REL, want.size))
    assert np.all(err <= REL), np.unravel_index(np.argmax(err), err.shape)


def _iq(C, n, **kw):
    return capi.Recc(n_channels=C, sps=kw.pop("sps", 10), max_samples=kw.pop("max_samples", n), max_bursts=kw.pop("max_bursts", 16),
                     stream_power=kw.pop("stream_power", True), **kw)


def _cuts(pieces):
    ends = np.cumsum(pieces)
    return list(zip(ends - pieces, ends))


# ---- 1. the IQ seam, ragged pushes
@pytest.mark.parametrize("C", [5, 66])
def test_iq_seam_blocks_equal_the_model_however_the_stream_is_cut(gpu, C):
    import torch
    n = sum(PIECES)
    y = _noise(100 + C, (C, n)) * np.linspace(0.25, 2.0, C, dtype=np.float32)[:, None]
    want = spr.blocks(y[:, :n // 64 * 64])
    # what the pushes process: n_done after each, by the seam's rule (whole 64-sample words of what has arrived)
    done = [int(e) // 64 * 64 for _, e in _cuts(PIECES)]
    assert done[0] == 0 and done[6] == done[5] and {d % 256 for d in done} == {0, 64, 128, 192}
    with _iq(C, n) as r:
        assert r.power_ring_snaps * 256 >= n
        r.push_iq(y)
        one, first = r.channel_power()
        rows = one.shape[0]
    assert first == 0 and rows == C and one.shape == (C, n // 64 * 64 // 256) == (C, 23)
    _check(one, want)

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
                seen.append(r.channel_power()[0].shape[1])
            P, f = r.channel_power()
        assert f == 0 and seen == [d // 256 for d in done]           # block j exists once 256 (j + 1) <= produced
        return P

    assert np.array_equal(_bits(ragged(False)), _bits(one))
    assert np.array_equal(_bits(ragged(True)), _bits(one))


# ---- 2. the origin
def test_origin_moves_the_block_edges(gpu):
    C, n, origin = 5, 3000, 960
    y = _noise(7, (C, n))
    with _iq(C, n) as r:
        r.set_origin(origin)
        r.push_iq(y[:, :777])
        r.push_iq(y[:, 777:])
        got, first = r.channel_power()
        _, produced = r.debug_slicer_bits(origin, 0)
        out = np.zeros((C, 1), np.float32)
        L = capi.load()
        assert L.amps_recc_channel_power(r._h, 3, 1, out.ctypes.data, 1, None, None) == -34     # block 3 begins before the origin
        assert L.amps_recc_channel_power(r._h, 4, 1, out.ctypes.data, 1, None, None) == 0
    assert produced == origin + n // 64 * 64
    assert first == spr.first_block(origin) == 4 and first + got.shape[1] == produced // 256
    want = spr.blocks(y[:, :n // 64 * 64], origin=origin)            # s = origin + m
    _check(got, want)
    assert np.array_equal(out[:, 0], got[:, 0])


# ---- 3. the ring
def test_ring_holds_exactly_the_window(gpu):
    C, sps, push, n = 2, 3, 1000, 50000
    y = _noise(11, (C, n))
    L = capi.load()
    with _iq(C, n, sps=sps, max_samples=1024) as r:
        snaps = r.power_ring_snaps
        assert snaps == 64                                           # R = 16384: the smallest power of two >= 1024 + 3 * 3586 + 1024
        for a in range(0, n, push):
            r.push_iq(np.ascontiguousarray(y[:, a:a + push]))
        got, first = r.channel_power()
        _, produced = r.debug_slicer_bits(0, 0)
        prod = first + got.shape[1]
        rows, ps = capi.C.c_uint32(0), capi.C.c_uint64(0)
        assert L.amps_recc_channel_power(r._h, 0, 0, None, 0, capi.C.byref(rows), capi.C.byref(ps)) == 0    # n = 0 only reports
        assert rows.value == C and ps.value == prod
        out = np.zeros((C, snaps + 1), np.float32)
        p = out.ctypes.data
        assert L.amps_recc_channel_power(r._h, first - 1, 1, p, snaps + 1, None, None) == -34          # -ERANGE: no longer held
        assert L.amps_recc_channel_power(r._h, first - 1, snaps + 1, p, snaps + 1, None, None) == -34
        assert L.amps_recc_channel_power(r._h, first, snaps + 1, p, snaps + 1, None, None) == -34      # not yet produced
        assert L.amps_recc_channel_power(r._h, prod + 1, 0, None, 0, None, None) == 0
        assert L.amps_recc_channel_power(r._h, prod + 1, 1, p, snaps + 1, None, None) == -34
        assert L.amps_recc_channel_power(r._h, prod - 1, 2, p, snaps + 1, None, None) == -34
        assert L.amps_recc_channel_power(r._h, prod, 0, None, 0, None, None) == 0
        assert L.amps_recc_channel_power(r._h, prod - 1, 1, p, snaps + 1, None, None) == 0
        assert np.array_equal(out[:, 0], got[:, -1])
        assert L.amps_recc_channel_power(r._h, first, snaps, p, snaps + 1, None, None) == 0            # the whole window, wrapped
        assert np.array_equal(out[:, :snaps], got)
        assert L.amps_recc_channel_power(r._h, first, 1, None, 0, None, None) == -22                   # argument errors as on the wideband seam
        assert L.amps_recc_channel_power(r._h, first, 2, p, 1, None, None) == -22
        assert L.amps_recc_channel_power(None, 0, 0, None, 0, None, None) == -22
        r.reset()                                                    # reset empties the window
        empty, f0 = r.channel_power()
        assert empty.shape == (C, 0) and f0 == 0
    assert produced == n // 64 * 64 and produced > 3 * 64 * 256      # three turns of the ring
    assert prod == produced // 256 and first == prod - snaps
    _check(got, spr.blocks(y)[:, first:prod])


# ---- 4. the translate seams: the power of what the stage delivers
def _ints(fmt, n, seed):
    info = np.iinfo(capi.SAMPLE_DTYPES[fmt])
    return np.random.default_rng(seed).integers(info.min, info.max + 1, size=(n, 2)).astype(capi.SAMPLE_DTYPES[fmt])


def _configure(r, cfg):
    kind = cfg[0]
    if kind == "shared":
        r.set_xlate_shared(cfg[1], cfg[2], cfg[3])
    elif kind == "resampled":
        r.set_xlate_resampled(cfg[1], cfg[2], cfg[3], cfg[4])
    else:
        r.set_xlate(rate_hz=cfg[1], center_hz=cfg[2], decim=cfg[3])


XL = {
    # name: (configuration, rows, sps, input samples (about 0.05 s), format, channel-rate samples at most)
    "400k_d2_fc32": (("shared", 400e3, [-160e3, 44e3, 130e3], 2), 3, 10, 20000, capi.SAMPLES_FC32, 10000),
    "2400k_d12_cu8": (("shared", 2.4e6, [-1.05e6, -615e3, 15e3, 1.11e6], 12), 4, 10, 120000, capi.SAMPLES_CU8, 10000),
    "2048k_5_64_cu8": (("resampled", 2.048e6, [-800e3, 15e3, 615e3], 5, 64), 3, 8, 102400, capi.SAMPLES_CU8, 8000),
    "per_row_400k_d2": (("rows", 400e3, 160e3, 2), 2, 10, 20000, capi.SAMPLES_FC32, 10000),
}


@pytest.mark.parametrize("name", sorted(XL))
def test_translate_seams_report_the_power_of_the_stage_output(gpu, name):
    cfg, C, sps, n, fmt, nmax = XL[name]
    rows = cfg[0] == "rows"
    if fmt == capi.SAMPLES_FC32:
        x = _noise(21, (C, n) if rows else n, 0.5)
    else:
        x = _ints(fmt, n, 22)
    cuts = _cuts([n // 3 + 17, 5, n - n // 3 - 22])                  # ragged, one piece shorter than any decimation
    with capi.Recc(n_channels=C, sps=sps, max_samples=nmax, max_bursts=16) as twin, \
         capi.Recc(n_channels=C, sps=sps, max_samples=nmax, max_bursts=16, stream_power=True) as r:
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
        got, first = r.channel_power()
        _, produced = r.debug_slicer_bits(0, 0)
        # the tap leaves the window alone
        if not rows:
            (r.debug_xlate_shared if fmt == capi.SAMPLES_FC32 else functools.partial(r.debug_xlate_shared_as, format=fmt))(x[:999])
            again, f2 = r.channel_power()
            assert f2 == first and np.array_equal(_bits(again), _bits(got))
    y = np.concatenate(ys, axis=1)
    assert y.shape[0] == C and produced == y.shape[1] // 64 * 64 and produced > 7000
    assert first == 0 and got.shape == (C, produced // 256)
    _check(got, spr.blocks(y[:, :produced]))


def test_an_sc16_stream_and_its_fc32_conversion_give_the_same_bits(gpu):
    cfg, C, sps, n, _, nmax = XL["2400k_d12_cu8"]
    q = _ints(capi.SAMPLES_SC16, n, 23)
    xf = capi.convert_samples(q, capi.SAMPLES_SC16)
    P = []
    for fmt, data in ((capi.SAMPLES_SC16, q), (capi.SAMPLES_FC32, xf)):
        with capi.Recc(n_channels=C, sps=sps, max_samples=nmax, max_bursts=16, stream_power=True) as r:
            _configure(r, cfg)
            for a, b in _cuts([50001, n - 50001]):
                if fmt == capi.SAMPLES_FC32:
                    r.push_raw_shared(data[a:b])
                else:
                    r.push_raw_shared_as(data[a:b], fmt)
            P.append(r.channel_power()[0])
    assert P[0].shape == (C, n // 12 // 64 * 64 // 256) and P[0].any()
    assert np.array_equal(_bits(P[0]), _bits(P[1]))


@pytest.mark.parametrize("fs,decim,n", [(400e3, 2, 20000), (2.4e6, 12, 120000)], ids=["400k_d2", "2400k_d12"])
def test_a_carrier_on_a_centre_reads_gain_times_amplitude_squared(gpu, fs, decim, n):
    """Tolerance: the translate tests hold the stage to |y - exact| <= (ntaps + 16) 2^-24 sum|h| max|x| per output sample
    (tests/test_gpu_xlate_shared.py, tests/test_gpu_xlate_rates.py); for a carrier of amplitude a on a centre exact = a sum(h) =
    gain a, so the relative bound on the amplitude is (ntaps + 16) 2^-24 sum|h| / gain, and twice that on the power."""
    a, gain, c = 0.37, 3.0, 1
    centres = [-0.4 * fs, 0.1375 * fs, 0.35 * fs]
    taps = np.asarray(oracle.firdes_low_pass(gain, fs, 10e3, 4.5e3), np.float64)
    tol = 2.0 * (len(taps) + 16) * 2.0 ** -24 * np.abs(taps).sum() / gain
    x = (a * np.exp(2j * np.pi * centres[c] * np.arange(n) / fs)).astype(np.complex64)
    with capi.Recc(n_channels=3, sps=10, max_samples=n // decim, max_bursts=16, stream_power=True) as r:
        r.set_xlate_shared(fs, centres, decim)
        r.push_raw_shared(x[:n // 2 + 3])
        r.push_raw_shared(x[n // 2 + 3:])
        P, first = r.channel_power()
    filled = -(-len(taps) // decim // 256)                           # the first block wholly behind the filter's rise
    assert first == 0 and P.shape[1] > filled + 20
    want = (gain * a) ** 2
    err = np.abs(P[c, filled:] / want - 1.0).max()
    print("\n%g ksps / %d: %d taps, worst |P / (gain a)^2 - 1| = %.3g, bound %.3g" % (fs / 1e3, decim, len(taps), err, tol))
    assert err <= tol
    assert P[[0, 2]][:, filled:].max() < 1e-4 * want                 # the other centres see the stop band (a Hamming design: 53 dB)


# ---- 5. burst power
A_BURST = 0.5


@functools.lru_cache(maxsize=None)
def _burst200():
    """one burst of amplitude A_BURST over noise 30 dB down, 200 ksps"""
    n = 44000
    iq, truth = synth.make_channel_block(n, 1, seed=41, sps=10, snr_db=30.0, first=2000)
    assert len(truth) == 1
    y = (iq * np.float32(A_BURST)).astype(np.complex64)
    y.setflags(write=False)
    return y, truth


def _burst_checks(r, recs, model, first=0):
    mean, cnt = r.burst_power(recs)
    assert mean.dtype == np.float32 and cnt.dtype == np.uint32 and len(recs) == 1
    g = recs[0]
    want, wcnt = spr.burst_mean(model[int(g["channel"])], int(g["position"]), 10, first=first)
    assert wcnt in (130, 131) and int(cnt[0]) == wcnt
    print("\nchannel %d at %d: mean %.8g, model %.8g, n = %d" % (g["channel"], g["position"], mean[0], want, wcnt))
    assert abs(float(mean[0]) - want) <= REL * want
    return float(mean[0])


def test_burst_power_on_the_iq_seam(gpu):
    y, truth = _burst200()
    n = y.size
    rows = np.stack([_noise(42, n, 0.01), y])                        # the mobile is on channel 1
    model = spr.blocks(rows[:, :n // 64 * 64])
    with _iq(2, n) as r:
        r.push_iq(np.ascontiguousarray(rows[:, :17001]))
        r.push_iq(np.ascontiguousarray(rows[:, 17001:]))
        recs = r.drain()
        assert [(int(g["channel"]), g["min"].decode()) for g in recs] == [(1, truth[0][2])]
        m = _burst_checks(r, recs, model)
        assert abs(m / A_BURST ** 2 - 1.0) < 0.01                    # a^2 and the noise 30 dB below it
        bad = recs.copy()
        bad["channel"][0] = 2                                        # channel = n_channels
        with pytest.raises(capi.AmpsError) as e:
            r.burst_power(bad)
        assert e.value.code == -22
        assert r.burst_power(recs[:0])[0].shape == (0,)
    # a ring so small that the capture has left the window by the time it is asked for: no count, no power, no error
    with _iq(2, n, max_samples=4096, max_bursts=16) as r:
        R = r.power_ring_snaps * 256
        assert R == 65536
        for a in range(0, n, 4096):
            r.push_iq(np.ascontiguousarray(rows[:, a:a + 4096]))
        small = r.drain()
        assert [(int(g["channel"]), int(g["position"]), g["min"]) for g in small] == [(int(g["channel"]), int(g["position"]), g["min"]) for g in recs]
        mean, cnt = r.burst_power(small)
        assert int(cnt[0]) in (130, 131) and mean[0] == m            # still held; the same bits from 4096-sample pushes
        zeros = np.zeros((2, 4096), np.complex64)
        for _ in range(R // 4096):
            r.push_iq(zeros)
        mean, cnt = r.burst_power(small)
        assert not cnt.any() and not mean.view(np.uint32).any()


def test_burst_power_on_the_shared_translate_seam(gpu):
    fs, decim, fc = 2.4e6, 12, 615e3
    centres = [-1.05e6, fc, 15e3]
    n = 444000
    iq, truth = synth.make_channel_block(n, 1, seed=43, sps=120, snr_db=30.0, first=4000)
    x = (A_BURST * iq * np.exp(2j * np.pi * fc * np.arange(n) / fs)).astype(np.complex64)
    cuts = _cuts([200003, n - 200003])
    with capi.Recc(n_channels=3, sps=10, max_samples=n // decim, max_bursts=16) as twin, \
         capi.Recc(n_channels=3, sps=10, max_samples=n // decim, max_bursts=16, stream_power=True) as r:
        twin.set_xlate_shared(fs, centres, decim)
        r.set_xlate_shared(fs, centres, decim)
        ys = []
        for a, b in cuts:
            ys.append(twin.debug_xlate_shared(x[a:b]))
            r.push_raw_shared(x[a:b])
        recs = r.drain()
        assert [(int(g["channel"]), g["min"].decode()) for g in recs] == [(1, truth[0][2])]
        y = np.concatenate(ys, axis=1)
        m = _burst_checks(r, recs, spr.blocks(y[:, :y.shape[1] // 64 * 64]))
    assert 0.3 < m / (3.0 * A_BURST) ** 2 < 1.1                      # gain 3; what the +-8 kHz deviation puts beyond the pass band is lost


# ---- 6. off means off
def test_off_means_off(gpu):
    L = capi.load()
    with _iq(4, 4096, stream_power=False) as r:
        out, cnt = np.zeros((4, 1), np.float32), np.zeros(1, np.uint32)
        recs = np.zeros(1, capi.BURST_DTYPE)
        r.push_iq(_noise(1, (4, 4096)))
        assert r.power_ring_snaps == 0
        assert L.amps_recc_channel_power(r._h, 0, 0, None, 0, None, None) == -38                       # -ENOSYS
        assert L.amps_recc_channel_power(r._h, 0, 1, out.ctypes.data, 1, None, None) == -38
        assert L.amps_recc_burst_power(r._h, recs.ctypes.data, 1, out.ctypes.data, cnt.ctypes.data) == -38
    for kw in (dict(n_channels=832, sps=3, max_samples=256, wideband={"channels": 1024, "decim": 512, "taps_per_branch": 8, "first_channel": 96}),
               dict(n_channels=832, sps=3, max_samples=256, unfused_wideband=True,
                    wideband={"channels": 1024, "decim": 512, "taps_per_branch": 8, "first_channel": 96}),
               dict(n_channels=832, sps=3, max_samples=256, channel_power=True,
                    wideband={"channels": 1024, "decim": 512, "taps_per_branch": 8, "first_channel": 96}),
               dict(n_channels=4, sps=10, max_samples=0),                                              # the symbol seam only
               dict(n_channels=4, sps=10, max_samples=4096, channel_power=True)):
        with pytest.raises(capi.AmpsError) as e:
            capi.Recc(max_bursts=16, stream_power=True, **kw)
        assert e.value.code == -22, kw
    # the records of a two-burst stream, flag off and on
    n = 90000
    iq, truth = synth.make_channel_block(n, 2, seed=44, sps=10, snr_db=30.0, first=2000)
    assert len(truth) == 2
    rows = np.stack([iq, _noise(45, n, 0.03)])
    got = []
    for on in (False, True):
        with _iq(2, n, stream_power=on) as r:
            r.push_iq(np.ascontiguousarray(rows[:, :33333]))
            r.push_iq(np.ascontiguousarray(rows[:, 33333:]))
            got.append(r.drain())
    assert len(got[0]) == 2 and got[0].tobytes() == got[1].tobytes()


# ---- 7. behind a split drain, on the second turn of the ring
def test_a_record_drained_behind_later_pushes_still_has_its_power(gpu):
    y, truth = _burst200()
    lead = 70000                                                     # the burst lies beyond one span of the ring (65536)
    x = np.concatenate([_noise(46, lead, 0.01), y, _noise(47, 8192, 0.01)])[None, :]
    n = x.shape[1]
    model = spr.blocks(x[:, :n // 64 * 64])
    with _iq(1, n, max_samples=8192) as r:
        snaps = r.power_ring_snaps
        assert snaps * 256 == 65536
        edge = lead + y.size
        for a in range(0, edge, 8192):
            r.push_iq(np.ascontiguousarray(x[:, a:min(a + 8192, edge)]))
        r.drain_begin()
        r.push_iq(np.ascontiguousarray(x[:, edge:]))                 # streaming use: the next push is enqueued before the drain ends
        recs = r.drain_end()
        assert [g["min"].decode() for g in recs] == [truth[0][2]] and int(recs[0]["position"]) > 65536
        _, first = r.channel_power()
        assert first == n // 64 * 64 // 256 - snaps > 0
        _burst_checks(r, recs, model[:, first:], first=first)


# ---- 8. the burst mean is the stated reduction of the ring, bit for bit, across the ring's wrap
def test_burst_means_are_the_stated_reduction_of_the_ring_bit_for_bit(gpu):
    """amps_recc_burst_power against tests/gatherref.py on the very floats amps_recc_channel_power returns: no tolerance.  The records
    are fabricated (the entry point takes any channel and position); held and unheld ones alternate in one call."""
    C, sps, push, pushes = 3, 12, 4096, 27
    y = _noise(48, (C, push * pushes))
    with _iq(C, push, sps=sps) as r:
        snaps = r.power_ring_snaps
        assert snaps == 256                                          # R = 65536: the smallest power of two >= 4096 + 12 * 3586 + 1024
        for a in range(0, y.shape[1], push):
            r.push_iq(np.ascontiguousarray(y[:, a:a + push]))
        ring, lo = r.channel_power()
        # position -> (first block, blocks): 158 blocks from 200 cross slot 255 -> 0 and give three values to the first lanes; 157 is
        # the other count class; block 172 has left the window; block 469 is not produced yet
        cases = {51200: (200, 158), 44000: (172, 0), 51201: (201, 157), 80000: (313, 0)}
        recs = np.zeros(len(cases) * C, capi.BURST_DTYPE)
        recs["position"] = np.repeat(list(cases), C)
        recs["channel"] = np.tile(np.arange(C), len(cases))
        mean, cnt = r.burst_power(recs)
    assert lo == 176 and ring.shape == (C, 256)                      # 110 592 samples: blocks [176, 432) are held
    assert (44000 + 255) // 256 < lo and (80000 + 3374 * sps) // 256 > lo + 256
    held = 0
    for g, m, c in zip(recs, mean, cnt):
        j0, count = cases[int(g["position"])]
        assert j0 == (int(g["position"]) + 255) // 256 and int(c) == count, (g["position"], int(c))
        if count == 0:
            assert gatherref.bits(m) == 0
            continue
        assert count == spr.burst_window(int(g["position"]), sps)[1] and j0 < 256 < j0 + count
        want = gatherref.gather_mean(ring[int(g["channel"]), j0 - lo:j0 - lo + count])
        print("\nchannel %d at %d: %d blocks, mean %.9g, stated reduction %.9g" % (g["channel"], g["position"], count, m, want))
        assert gatherref.bits(m) == gatherref.bits(want)
        held += 1
    assert held == 2 * C
