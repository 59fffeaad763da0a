"""-m gpu: per-channel received power of the wideband seam (AMPS_RECC_FLAG_CHANNEL_POWER: amps_recc_channel_power, amps_recc_burst_power)
against the float64 model tests/powerref.py, at both decimations (conftest.py: `decim`).

Tolerance.  The project holds the channelizer to |y_gpu - y_ref| <= eps S with eps = 2e-5 and S = max |y_ref|
(tests/test_gpu_channelizer.py:34-36).  With P = |y|^2 it follows that |P_gpu - P_ref| <= eps S (2 sqrt(P_ref) + eps S), per entry; no
other number is used.  A wrong tap, bin, frame or row gives errors of order S^2."""
import numpy as np
import pytest

import gatherref
import powerref
from gr_amps_amd import capi, synth_wideband as sw
from conftest import wb_cfg

pytestmark = pytest.mark.gpu

EPS = 2e-5


def _handle(D, C, first, max_frames, max_bursts=64, channel_power=True, **kw):
    groups = {k: kw.pop(k) for k in ("groups", "group") if k in kw}
    wb, sps = wb_cfg(D, first, **groups)
    return capi.Recc(n_channels=C, sps=sps, max_samples=max_frames, max_bursts=max_bursts, wideband=wb, channel_power=channel_power, **kw)


def _bound(P_ref):
    """per-entry bound on |P_gpu - P_ref|, S taken over the block the model was computed for"""
    S = np.sqrt(P_ref.max())
    return EPS * S * (2.0 * np.sqrt(P_ref) + EPS * S)


def _check(got, want):
    assert got.shape == want.shape and got.dtype == np.float32
    err, bound = np.abs(got.astype(np.float64) - want), _bound(want)
    print("\nworst |P_gpu - P_ref| / bound = %.4f" % (err / bound).max())
    assert np.all(err <= bound), np.unravel_index(np.argmax(err / bound), err.shape)


def _tones(D, nframes, seed=1):
    """the inputs of test_channelizer_matches_numpy_filter_bank, longer"""
    rng = np.random.default_rng(seed)
    n = nframes * D
    t = np.arange(n)
    x = 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for k, a in ((3, 1.0), (100, 0.5), (511, 0.7), (900, 0.3)):
        x += a * np.exp(2j * np.pi * (sw.bin_freq(k) + 5e3) * t / sw.FS_WIDE)
    return x.astype(np.complex64)


def _noise(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n, np.float32) + 1j * rng.standard_normal(n, np.float32)).astype(np.complex64)


@pytest.fixture(scope="module")
def tones():
    """per decimation: (stream, model snapshots of all 1024 bins) -- computed once, never modified"""
    cache = {}

    def get(D):
        if D not in cache:
            x = _tones(D, 1100)
            P = powerref.snapshots(x, D, 0, 1024)
            x.setflags(write=False)
            P.setflags(write=False)
            cache[D] = (x, P)
        return cache[D]
    return get


def test_snapshots_equal_the_model(gpu, decim, tones):
    D = decim
    x, want = tones(D)
    assert want.shape == (1024, 5)
    with _handle(D, 1024, 0, 1100 + 8) as r:
        assert r.power_ring_snaps * 256 >= 1100
        r.push_wideband(x)
        got, first = r.channel_power()
    assert first == 0 and got.shape == (1024, 5)                     # 1100 frames -> 1088 consumed: snapshots 0, 256, 512, 768, 1024
    _check(got, want)
    # the tones stand where they were put: 5 kHz off centre is inside the pass band (snapshot 0 still sees the zeros before the stream)
    for k, a in ((3, 1.0), (100, 0.5), (511, 0.7), (900, 0.3)):
        assert np.all(np.abs(got[k, 1:] / a ** 2 - 1.0) < 0.2), (k, got[k])
    # a band selection: row i is bin 96 + i
    with _handle(D, 832, 96, 1100 + 8) as r:
        r.push_wideband(x)
        got, first = r.channel_power()
    assert first == 0
    _check(got, want[96:96 + 832])


def test_history_does_not_depend_on_chunking_or_sample_type(gpu, decim):
    D = decim
    n = 1100 * D
    rng = np.random.default_rng(7)
    q = rng.integers(-20000, 20000, size=(n, 2), dtype=np.int16)    # an int16 stream and its exact fc32 twin
    x = (q[:, 0].astype(np.float32) + 1j * q[:, 1].astype(np.float32)).astype(np.complex64)

    def run(push, pieces):
        with _handle(D, 832, 96, 1100 + 8) as r:
            off = 0
            for m in pieces:
                m = min(m, n - off)
                if m > 0:
                    push(r, off, m)
                off += m
            P, first = r.channel_power()
            rows, prod = P.shape[0], first + P.shape[1]
        assert rows == 832 and first == 0 and prod == 5
        return P.view(np.uint32)

    f32 = lambda r, off, m: r.push_wideband(x[off:off + m])
    s16 = lambda r, off, m: r.push_wideband_short(q[off:off + m])
    one = run(f32, [n])
    assert one.any()
    ragged = [1, 511, 70 * D - 13, 300 * D + 501, 3 * D + 11, n]
    assert np.array_equal(run(f32, ragged), one)
    assert np.array_equal(run(s16, [n]), one)
    assert np.array_equal(run(s16, ragged), one)
    # 64-frame launches: three in four contain no snapshot frame
    assert np.array_equal(run(f32, [64 * D] * (n // (64 * D) + 1)), one)
    mixed = lambda r, off, m: (s16 if (off // D) % 128 else f32)(r, off, m)
    assert np.array_equal(run(mixed, [64 * D] * (n // (64 * D) + 1)), one)


def test_origin_shifts_the_snapshot_frames(gpu, decim, tones):
    D = decim
    x, _ = tones(D)
    origin = 64 * 3
    want = powerref.snapshots(x, D, 96, 832, origin=origin)          # frames 64, 320, 576, 832, 1088
    with _handle(D, 832, 96, 1100 + 8) as r:
        r.set_origin(origin)
        r.push_wideband(x)
        got, first = r.channel_power()
        L = capi.load()
        out = np.zeros((832, 1), np.float32)
        assert L.amps_recc_channel_power(r._h, 0, 1, out.ctypes.data, 1, None, None) == -34   # snapshot 0 lies before the origin
    assert first == powerref.first_snapshot(origin) == 1
    assert got.shape == (832, 4)                                     # 1088 frames consumed: s < 192 + 1088 = 1280 -> j = 1 .. 4
    _check(got, want[:, :4])


def test_ring_keeps_the_newest_window(gpu, decim):
    D = decim
    nfr = 20000
    x = _noise(nfr * D, 11)
    with _handle(D, 64, 200, 2048) as r:
        snaps = r.power_ring_snaps
        assert snaps == 64                                           # R = 16384
        for off in range(0, nfr, 2048):
            r.push_wideband(x[off * D:(off + 2048) * D])
        got, first = r.channel_power()
        prod = first + got.shape[1]
        L = capi.load()
        out = np.zeros((64, snaps + 1), np.float32)
        p = out.ctypes.data
        assert L.amps_recc_channel_power(r._h, first - 1, 1, p, snaps + 1, None, None) == -34          # -ERANGE: no longer held
        assert L.amps_recc_channel_power(r._h, first - 1, snaps + 1, p, snaps + 1, None, None) == -34
        assert L.amps_recc_channel_power(r._h, first, snaps + 1, p, snaps + 1, None, None) == -34      # not yet produced
        assert L.amps_recc_channel_power(r._h, prod - 1, 2, p, snaps + 1, None, None) == -34
        assert L.amps_recc_channel_power(r._h, prod, 0, None, 0, None, None) == 0
        assert L.amps_recc_channel_power(r._h, prod - 1, 1, p, snaps + 1, None, None) == 0
        assert np.array_equal(out[:, 0], got[:, -1])
        assert L.amps_recc_channel_power(r._h, first, 1, None, 0, None, None) == -22
        assert L.amps_recc_channel_power(r._h, first, 2, p, 1, None, None) == -22
        # reset empties the window
        r.reset()
        empty, f0 = r.channel_power()
        assert empty.shape == (64, 0) and f0 == 0
    consumed = nfr // 64 * 64                                        # 19968 frames: snapshots 0 .. 77
    assert prod == -(-consumed // 256) == 78 and first == prod - 64
    want = powerref.snapshots(x, D, 200, 64)
    _check(got, want[:, first:prod])


def test_off_means_off(gpu, decim):
    D = decim
    L = capi.load()
    first, C = 96, 832
    with _handle(D, C, first, 256, channel_power=False) as r:
        out, cnt = np.zeros((C, 1), np.float32), np.zeros(1, np.uint32)
        recs = np.zeros(1, capi.BURST_DTYPE)
        assert r.power_ring_snaps == 0
        assert L.amps_recc_channel_power(r._h, 0, 0, None, 0, None, None) == -38                       # -ENOSYS
        assert L.amps_recc_channel_power(r._h, 0, 1, out.ctypes.data, 1, None, None) == -38
        assert L.amps_recc_burst_power(r._h, recs.ctypes.data, 1, out.ctypes.data, cnt.ctypes.data) == -38
    with pytest.raises(capi.AmpsError) as e:
        _handle(D, C, first, 256, unfused_wideband=True)
    assert e.value.code == -22
    with pytest.raises(capi.AmpsError) as e:
        capi.Recc(n_channels=4, sps=10, max_samples=4096, channel_power=True)       # no wideband seam
    assert e.value.code == -22
    # the records of test_wideband_bursts_decode_to_the_transmitted_words' stream, with the flag off and on
    n = int(0.2 * sw.FS_WIDE) // D * D
    bursts = [(first + 4, 200000), (first + 5, 250000), (first + 6, 300000), (first + 700, 100000), (first + 831, 400000), (first + 0, 50000)]
    x, truth = sw.make_wideband(n, bursts, seed=3)
    recs = []
    for on in (False, True):
        with _handle(D, C, first, n // D + 8, max_bursts=256, channel_power=on) as r:
            half = (n // 2) // D * D + 100
            r.push_wideband(x[:half])
            r.push_wideband(x[half:])
            recs.append(r.drain())
    assert len(recs[0]) == len(bursts) and recs[0].tobytes() == recs[1].tobytes()


def test_burst_power(gpu, decim):
    D = decim
    sps = 1536 // D
    first, C = 96, 832
    n = int(0.25 * sw.FS_WIDE) // D * D
    a, _ = sw.make_wideband(n, [(100, 300000)], seed=3)
    b, _ = sw.make_wideband(n, [(500, 700000)], seed=4, snr_db=200.0)
    x = (a + np.float32(0.25) * b).astype(np.complex64)
    model = powerref.snapshots(x, D, first, C)
    with _handle(D, C, first, n // D + 8) as r:
        R = r.power_ring_snaps * 256
        half = (n // 2) // D * D + 100                               # two ragged pushes
        r.push_wideband(x[:half])
        r.push_wideband(x[half:])
        recs = r.drain()
        assert sorted(int(g["channel"]) for g in recs) == [4, 404]   # both bursts decode
        mean, cnt = r.burst_power(recs)
        assert mean.dtype == np.float32 and cnt.dtype == np.uint32
        for g, m, c in zip(recs, mean, cnt):
            row = model[int(g["channel"])]
            want, wcnt = powerref.burst_mean(row, int(g["position"]), sps)
            j0, _ = powerref.burst_window(int(g["position"]), sps)
            assert wcnt in ((26, 27) if sps == 2 else (39, 40)) and int(c) == wcnt
            S = np.sqrt(model.max())
            tol = np.mean(EPS * S * (2.0 * np.sqrt(row[j0:j0 + wcnt]) + EPS * S))        # the mean of the per-snapshot bounds
            print("\nchannel %d: mean %.6g, model %.6g, |diff| / bound %.4f" % (g["channel"], m, want, abs(float(m) - want) / tol))
            assert abs(float(m) - want) <= tol
        # a unit-envelope FSK mobile reads somewhat below 1.0 (what the +-8 kHz deviation puts beyond the prototype's pass band is lost) or
        # a little above (256 frames are a whole number of symbols at D = 768: every snapshot of a burst samples the same phase of the
        # filtered envelope); the second mobile, at a quarter of the amplitude, a sixteenth of that
        by = {int(g["channel"]): float(m) for g, m in zip(recs, mean)}
        assert 0.3 < by[4] < 1.3 and 0.3 < by[404] / 0.0625 < 1.3
        # a channel this handle does not decode
        bad = recs.copy()
        bad["channel"][0] = C
        with pytest.raises(capi.AmpsError) as e:
            r.burst_power(bad)
        assert e.value.code == -22
        assert r.burst_power(recs[:0])[0].shape == (0,)
        # a ring's span later the captures are gone: no count, no power, no error
        zeros = np.zeros(4096 * D, np.complex64)
        for _ in range(-(-R // 4096)):
            r.push_wideband(zeros)
        mean, cnt = r.burst_power(recs)
        assert not cnt.any() and not mean.view(np.uint32).any()


def test_channel_group_rows_equal_the_whole_band_rows(gpu, decim, tones):
    D = decim
    x, _ = tones(D)
    first, C = 96, 832
    with _handle(D, C, first, 1100 + 8) as r:
        r.push_wideband(x)
        whole, f0 = r.channel_power()
    with _handle(D, C, first, 1100 + 8, groups=2, group=1) as r:
        r.push_wideband(x)
        part, f1 = r.channel_power()
        mine = [c for c in range(C) if ((first + c) % 64) // 32 == 1]
        assert r.power_ring_snaps > 0
        # records carry whole-band channel numbers: one of the other group's is not this handle's
        recs = np.zeros(2, capi.BURST_DTYPE)
        recs["channel"] = [mine[0], mine[-1]]
        mean, cnt = r.burst_power(recs)
        assert mean.shape == (2,)
        other = [c for c in range(C) if c not in set(mine)][0]
        recs["channel"][1] = other
        with pytest.raises(capi.AmpsError) as e:
            r.burst_power(recs)
        assert e.value.code == -22
    assert f0 == f1 == 0 and part.shape == (len(mine), whole.shape[1]) and len(mine) == C // 2
    assert np.array_equal(part.view(np.uint32), whole[mine].view(np.uint32))


# The burst mean is the stated reduction of the ring, bit for bit (tests/gatherref.py), on the very floats amps_recc_channel_power
# returns: no tolerance.  The gather kernel is the one the IQ and translate seams use, so the wrap of its loop round the ring's end is
# covered once, in tests/test_gpu_stream_power.py; here it would cost a ring's span of frames, and test_ring_keeps_the_newest_window
# turns this ring already.  64 channels: the fewest at which a wideband handle takes the capture form every other test of this seam
# runs (below 64 a handle queues its captures, recc_resolve.hip.h); the gather does not depend on the count.
GATHER_FRAMES = {512: 10560, 768: 7232}                              # the smallest multiples of 64 at which snapshot 41 / 28 exists
GATHER_COUNTS = {512: (40, 39), 768: (27, 26)}                       # at position 512 (j0 = 2) and 513 (j0 = 3)


@pytest.fixture(scope="module")
def gather_noise():
    cache = {}

    def get(D):
        if D not in cache:
            cache[D] = _noise(GATHER_FRAMES[D] * D, 13)
            cache[D].setflags(write=False)
        return cache[D]
    return get


def _gather_check(r, x, D, channels, row_of, foreign=None):
    for off in range(0, GATHER_FRAMES[D], 2048):
        r.push_wideband(x[off * D:(off + 2048) * D])
    ring, lo = r.channel_power()
    assert lo == 0 and ring.shape[1] == -(-GATHER_FRAMES[D] // 256) == GATHER_COUNTS[D][0] + 2
    cases = {512: (2, GATHER_COUNTS[D][0]), 256 * 60: (60, 0), 513: (3, GATHER_COUNTS[D][1])}
    recs = np.zeros(len(cases) * len(channels), capi.BURST_DTYPE)
    recs["position"] = np.repeat(list(cases), len(channels))
    recs["channel"] = np.tile(channels, len(cases))
    mean, cnt = r.burst_power(recs)
    for g, m, c in zip(recs, mean, cnt):
        j0, count = cases[int(g["position"])]
        assert int(c) == count, (int(g["position"]), int(c))
        if count == 0:
            assert gatherref.bits(m) == 0                            # beyond what is produced
            continue
        assert (j0, count) == powerref.burst_window(int(g["position"]), 1536 // D)
        want = gatherref.gather_mean(ring[row_of(int(g["channel"])), j0:j0 + count])
        print("\nchannel %d at %d: %d snapshots, mean %.9g, stated reduction %.9g" % (g["channel"], g["position"], count, m, want))
        assert gatherref.bits(m) == gatherref.bits(want)
    if foreign is not None:                                          # a channel of the other group in the same call
        recs["channel"][1] = foreign
        with pytest.raises(capi.AmpsError) as e:
            r.burst_power(recs)
        assert e.value.code == -22


def test_burst_means_are_the_stated_reduction_of_the_ring_bit_for_bit(gpu, decim, gather_noise):
    D = decim
    first, C = 96, 64
    with _handle(D, C, first, 2048) as r:
        _gather_check(r, gather_noise(D), D, [0, 31, C - 1], lambda ch: ch)


def test_burst_means_of_a_channel_group_bit_for_bit(gpu, gather_noise):
    D = 768
    first, C = 96, 64
    with _handle(D, C, first, 2048, groups=2, group=1) as r:
        mine = [c for c in range(C) if ((first + c) % 64) // 32 == 1]
        other = [c for c in range(C) if c not in set(mine)][0]
        assert len(mine) == C // 2
        _gather_check(r, gather_noise(D), D, [mine[0], mine[7], mine[-1]], mine.index, foreign=other)
