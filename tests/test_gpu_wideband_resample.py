"""-m gpu: the wideband seam behind its L / M resampler (amps_recc_set_wideband_resample, wb_resample_kernel) -- the tap against
float64, every prototype tap read back exactly, the stream under other cuts and in other sample formats, the bank behind the resampler
against a plain bank fed the tap's output, both burst blocks end to end, and the admission.  tests/wbresampleref.py holds the float64
side and the blocks."""
import ctypes as C
import errno

import numpy as np
import pytest

from gr_amps_amd import capi

import wbresampleref as wr
import xlateresampleref as rr

pytestmark = pytest.mark.gpu
FC32, SC16, SC8, CU8 = capi.SAMPLES_FC32, capi.SAMPLES_SC16, capi.SAMPLES_SC8, capi.SAMPLES_CU8
RATIOS = pytest.mark.parametrize("rate,L,M,channels", wr.RATIOS, ids=wr.RATIO_IDS)
DECIM = {500: 125, 128: 96, 1024: 768}


def _handle(rate, L, M, channels, decim=None, C=1, first=0, max_frames=4096, resample=True, **kw):
    wb = {"channels": channels, "decim": decim or DECIM[channels], "first_channel": first}
    if resample:
        wb["resample"] = (rate, L, M)
    return capi.Recc(n_channels=C, max_samples=max_frames, max_bursts=64, wideband=wb, **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _noise(seed, n, scale=1.0):
    rng = np.random.default_rng(seed)
    return (scale * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def _inputs_for(want_out, L, M):
    """the largest n that delivers at most want_out outputs: exactly want_out, or one fewer where no n delivers that"""
    n = want_out * M // L
    while wr.nout(n + 1, L, M) <= want_out:
        n += 1
    assert want_out - 1 <= wr.nout(n, L, M) <= want_out
    return n


def _tap_in_pieces(r, x, cuts, fmt=FC32):
    parts, off = [], 0
    for m in cuts:
        parts.append(r.debug_wideband_resample(x[off:off + m], fmt))
        off += m
    assert off == len(x)
    return parts


# ---- 1. the tap against float64
@RATIOS
def test_tap_meets_float64(gpu, rate, L, M, channels):
    """four tiles and 37 outputs in ragged pieces: noise plus a tone in the pass band and one inside the transition band, against
    scipy's upfirdn on the float64 prototype.  Per component |y32 - y64| <= (ntp + 2) 2^-24 max_p sum_i |h_p[i]| max|x|.  Measured
    worst ratios to that bound, printed by every run: 5/4 0.042, 6/5 0.035, 8/5 0.036, 2/1 0.035, 1/2 0.020, 5/3 0.032; an indexing error is of the order of the output itself, far above the bound."""
    n = _inputs_for(4 * wr.TILE + 37, L, M)
    want_out = wr.nout(n, L, M)
    cutoff, width = wr.default_filter(rate, channels)
    t = np.arange(n)
    x = _noise(100 + L * 10 + M, n, 0.2).astype(np.complex128)
    x += 0.7 * np.exp(2j * np.pi * (0.31 * cutoff) * t / rate) + 0.5 * np.exp(-2j * np.pi * (cutoff + 0.2 * width) * t / rate)
    x = x.astype(np.complex64)
    g = wr.prototype64(rate, L, channels)
    with _handle(rate, L, M, channels) as r:
        parts = _tap_in_pieces(r, x, wr.ragged(n, L + M))
    y = np.concatenate(parts)
    assert y.shape == (want_out,) and y.dtype == np.complex64
    want = wr.upfirdn(x, g, L, M)
    bound = wr.bound(g, L, max(np.abs(x.real).max(), np.abs(x.imag).max()))
    err = max(np.abs(y.real - want.real).max(), np.abs(y.imag - want.imag).max())
    print("\n%g Msps x %d/%d: worst |y32 - y64| = %.3g, bound %.3g, ratio %.3f, max |y64| = %.3g" % (rate / 1e6, L, M, err, bound, err / bound, np.abs(want).max()))
    assert err <= bound, (err, bound)
    assert np.abs(want).max() > 1000 * bound


# ---- 2. every tap of the prototype, exactly
@RATIOS
def test_every_prototype_tap_is_read_back_exactly(gpu, rate, L, M, channels):
    """real impulses of power-of-two amplitudes at every input residue mod M, further apart than a phase is long: output k holds
    a g[k M - L n0] and nothing else, so each g[j] is compared with == and every other output is exactly zero.  g is the oracle's
    firdes.low_pass at the up-sampled rate with gain L, rounded to float32 as the library rounds its own."""
    g = wr.prototype32(rate, L, channels)
    ntp = wr.ntp_of(g, L)
    gap = ntp + M + 3
    imp = [(m * (gap // M + 2) * M + (7 * m) % M + 5 * M, 2.0 ** (m % 5 - 2) * (-1) ** m) for m in range(M)]
    assert sorted(n0 % M for n0, _ in imp) == list(range(M))
    n = imp[-1][0] + gap
    x = np.zeros(n, np.complex64)
    for n0, a in imp:
        x[n0] = a
    want, seen = rr.impulse_expected(g, L, M, wr.nout(n, L, M), imp)
    assert seen.all()
    with _handle(rate, L, M, channels) as r:
        y = r.debug_wideband_resample(x) + np.complex64(0)
    assert y.shape == want.shape
    bad = np.flatnonzero((_bits(y).reshape(-1, 2) != _bits(want).reshape(-1, 2)).any(axis=1))
    assert bad.size == 0, (L, M, bad[:8])
    assert np.count_nonzero(want) >= np.count_nonzero(g)


# ---- 3. cuts
@pytest.mark.parametrize("rate,L,M,channels", [wr.RATIOS[0], wr.RATIOS[2], wr.RATIOS[4]], ids=["5_4", "8_5", "1_2"])
def test_streaming_is_bitwise(gpu, rate, L, M, channels):
    """pushes of one sample, of fewer than M / L samples and ragged larger pieces equal one push, a device block, and the same after
    amps_recc_reset; each call delivers the ceil(L N / M) difference"""
    import torch
    n = _inputs_for(2 * wr.TILE + 301, L, M)
    x = _noise(7 + L, n)
    with _handle(rate, L, M, channels) as r:
        one = r.debug_wideband_resample(x)
        assert one.shape == (wr.nout(n, L, M),)
        r.reset()
        dev = r.debug_wideband_resample(torch.from_numpy(x).to(gpu))
        r.reset()
        cuts = [1] * 41 + wr.ragged(n - 41, 3 * L + M)
        parts = _tap_in_pieces(r, x, cuts)
        done = np.cumsum(cuts)
        assert [len(p) for p in parts] == [wr.nout(int(b), L, M) - wr.nout(int(b - m), L, M) for b, m in zip(done, cuts)]
        if L < M:
            assert min(len(p) for p in parts) == 0                      # a push of fewer than M / L samples may deliver nothing
        r.reset()
        again = r.debug_wideband_resample(x)
    assert _same(one, dev) and _same(one, np.concatenate(parts)) and _same(one, again)


# ---- 4. formats
def _full_range(fmt, n, seed):
    rng = np.random.default_rng(seed)
    info = np.iinfo(capi.SAMPLE_DTYPES[fmt])
    a = rng.integers(info.min, info.max + 1, (n, 2)).astype(capi.SAMPLE_DTYPES[fmt])
    edge = [[info.min, info.max], [info.max, info.min], [info.min, info.min], [info.max, info.max]][:n]
    a[:len(edge)] = edge
    return a


@pytest.mark.parametrize("fmt", [SC16, SC8, CU8], ids=["sc16", "sc8", "cu8"])
def test_formats_equal_the_fc32_call_on_converted_samples(gpu, fmt):
    import torch
    rate, L, M, channels = wr.RATIOS[0]
    n = _inputs_for(wr.TILE + 97, L, M)
    a = _full_range(fmt, n + 1, 50 + fmt)
    with _handle(rate, L, M, channels) as r:
        want = r.debug_wideband_resample(capi.convert_samples(a[:n], fmt))
        r.reset()
        host = r.debug_wideband_resample(a[:n], fmt)
        r.reset()
        d = torch.from_numpy(a).to(gpu)
        dev = r.debug_wideband_resample(d[:n], fmt)
        r.reset()
        want_odd = r.debug_wideband_resample(capi.convert_samples(a[1:], fmt))
        r.reset()
        odd = r.debug_wideband_resample(d[1:], fmt)                      # a device block from an odd sample
    assert _same(want, host) and _same(want, dev) and _same(want_odd, odd)
    assert np.abs(want).max() > 16


def test_seven_pushes_in_alternating_formats(gpu):
    rate, L, M, channels = wr.RATIOS[1]
    fmts = [SC8, FC32, CU8, SC16, SC8, CU8, FC32]
    sizes = [333, 1, 2048, 77, 1500, 3, 900]
    blocks = [(_noise(60 + i, m, 40.0) if f == FC32 else _full_range(f, m, 60 + i)) for i, (f, m) in enumerate(zip(fmts, sizes))]
    whole = np.concatenate([capi.convert_samples(b, f) for b, f in zip(blocks, fmts)])
    with _handle(rate, L, M, channels) as r:
        want = r.debug_wideband_resample(whole)
        r.reset()
        got = np.concatenate([r.debug_wideband_resample(b, f) for b, f in zip(blocks, fmts)])
    assert _same(want, got)


# ---- 5. through the bank
@pytest.mark.parametrize("rate,L,M,channels,decim", [(3.2e6, 6, 5, 128, 96), (3.2e6, 6, 5, 128, 64), (4e6, 5, 4, 500, 125)], ids=["M128-D96", "M128-D64", "M500"])
@pytest.mark.parametrize("shift_hz", [0.0, 1234.5], ids=["unshifted", "shifted"])
def test_bank_behind_the_resampler_is_the_bank_on_the_taps_output(gpu, rate, L, M, channels, decim, shift_hz):
    """debug_channelize of a resampling handle == a plain handle of the same bank fed the tap's output, bit for bit, in two ragged
    pushes; again with a shift on both handles (its n counts the resampler's outputs)"""
    C, first = channels // wr.BANKS[channels][1], 3
    n = _inputs_for(130 * decim + 11, L, M)
    x = _noise(80 + decim, n)
    cuts = [n // 3 + 1, n - n // 3 - 1]
    with _handle(rate, L, M, channels, decim) as t:
        ys = _tap_in_pieces(t, x, cuts)
    with _handle(rate, L, M, channels, decim, C=C, first=first, max_frames=160) as r, \
            _handle(rate, L, M, channels, decim, C=C, first=first, max_frames=160, resample=False) as p:
        if shift_hz:
            r.set_wideband_shift(shift_hz)
            p.set_wideband_shift(shift_hz)
        off = 0
        for m, y in zip(cuts, ys):
            got, want = r.debug_channelize(x[off:off + m]), p.debug_channelize(y)
            off += m
            assert got.shape[1] > 0 and _same(got, want)
    assert np.abs(want).max() > 0


def test_fused_1024_bank_behind_the_resampler(gpu):
    """15.36 Msps x 2/1 into the 1024 bank, 256 frames: the slicer-bit ring of the fused form equals that of a plain 1024 handle fed the
    tap's output"""
    rate, L, M, D, C, first = 15.36e6, 2, 1, 768, 8, 100
    n = 256 * D // 2
    x = _noise(91, n)
    with _handle(rate, L, M, 1024, D) as t:
        y = t.debug_wideband_resample(x)
    assert y.shape == (256 * D,)
    with _handle(rate, L, M, 1024, D, C=C, first=first, max_frames=256 + 72) as r, \
            _handle(rate, L, M, 1024, D, C=C, first=first, max_frames=256 + 72, resample=False) as p:
        r.push_wideband(x)
        p.push_wideband(y)
        got, ngot = r.debug_slicer_bits(0, 0)
        _, nwant = p.debug_slicer_bits(0, 0)
        assert ngot == nwant and ngot >= 128
        got, _ = r.debug_slicer_bits(0, ngot)
        want, _ = p.debug_slicer_bits(0, ngot)
    assert got.shape == (C, ngot) and np.array_equal(got, want) and 0 < got.mean() < 1


# ---- 6. end to end
def _flush_of(b):
    return np.zeros(80 * b.decim, np.complex64)


def _records(r, pushes):
    for push in pushes:
        push()
    return r.drain()


@pytest.mark.parametrize("name", sorted(wr.BURSTS))
def test_burst_block_end_to_end(gpu, name):
    """every MIN and word back; the records byte for byte those of a plain bank handle fed the tap's output; the words those of the
    float64 chain (upfirdn -> float64 bank -> CPU model of the IQ seam)"""
    b = wr.BURSTS[name]
    x, truth = wr.burst_block(name)
    xx = np.concatenate([x, _flush_of(b)])
    frames = wr.nout(len(xx), b.L, b.M) // b.decim + 8
    with _handle(b.rate, b.L, b.M, b.channels, b.decim) as t:
        y = t.debug_wideband_resample(xx)
    with _handle(b.rate, b.L, b.M, b.channels, b.decim, C=b.C, first=b.first, max_frames=frames) as r:
        got = _records(r, [lambda: r.push_wideband(x), lambda: r.push_wideband(_flush_of(b))])
    with _handle(b.rate, b.L, b.M, b.channels, b.decim, C=b.C, first=b.first, max_frames=frames, resample=False) as p:
        cut = wr.nout(len(x), b.L, b.M)
        want = _records(p, [lambda: p.push_wideband(y[:cut]), lambda: p.push_wideband(y[cut:])])
    assert sorted(int(c) for c in got["channel"]) == sorted(b.rows)
    assert got.tobytes() == want.tobytes()
    model = wr.burst_model(name)
    assert len(model) == 6
    for i, row in enumerate(b.rows):
        kind, min10, esn, dialed, words = truth[row]
        g = got[[int(c) for c in got["channel"]].index(row)]
        m = model[[int(c) for c in model["channel"]].index(i)]
        assert g["min"].decode() == min10 and g["valid"].all(), (name, row)
        sent = [bytes(np.asarray(w, np.uint8)) for w in words]                  # every word as it was transmitted
        assert [bytes(g["word_dec"][w]) for w in range(len(sent))] == sent, (name, row)
        assert np.array_equal(g["word_dec"], m["word_dec"]) and np.array_equal(g["valid"], m["valid"]) and g["dialed"] == m["dialed"], (name, row)


def test_burst_block_as_sc8_equals_the_fc32_call(gpu):
    """the 4 Msps block as a HackRF delivers it: byte for byte the fc32 call on the converted samples (not held to the transmitted truth)"""
    b = wr.BURSTS["4M"]
    x, _ = wr.burst_block("4M")
    scale = 100.0 / max(np.abs(x.real).max(), np.abs(x.imag).max())
    a = np.stack([np.rint(x.real * scale), np.rint(x.imag * scale)], axis=1).astype(np.int8)
    flush = np.zeros((80 * b.decim, 2), np.int8)
    frames = wr.nout(len(a) + len(flush), b.L, b.M) // b.decim + 8
    out = []
    for as_sc8 in (True, False):
        with _handle(b.rate, b.L, b.M, b.channels, b.decim, C=b.C, first=b.first, max_frames=frames) as r:
            for blk in (a, flush):
                if as_sc8:
                    r.push_wideband_as(blk, SC8)
                else:
                    r.push_wideband(capi.convert_samples(blk, SC8))
            out.append(r.drain())
    assert len(out[0]) >= 1 and out[0].tobytes() == out[1].tobytes()


# ---- 7. admission
def _set(r, rate, L, M, cutoff=0.0, width=0.0, size=None):
    x = capi.WidebandResampleCfg(C.sizeof(capi.WidebandResampleCfg) if size is None else size, L, M, 0, rate, cutoff, width)
    return capi.load().amps_recc_set_wideband_resample(r._h, C.byref(x))


def test_admission_and_error_codes(gpu):
    lib = capi.load()
    rate, L, M, channels = wr.RATIOS[0]
    x = _noise(5, 4000)
    with _handle(rate, L, M, channels) as r:
        before = r.debug_wideband_resample(x)
        r.reset()
        EINVAL, E2BIG = -errno.EINVAL, -errno.E2BIG
        assert lib.amps_recc_set_wideband_resample(None, None) == EINVAL and lib.amps_recc_set_wideband_resample(r._h, None) == EINVAL
        assert _set(r, rate, L, M, size=36) == EINVAL
        for l, m in ((0, 4), (9, 4), (5, 9), (4, 4), (6, 4), (8, 1), (1, 3), (2, 5)):       # range, L = M, a common factor, beyond 4, below 1/2
            assert _set(r, 5e6 * m / max(l, 1), l, m) == EINVAL, (l, m)
        assert _set(r, 4.1e6, 5, 4) == EINVAL and _set(r, 4e6 * (1 + 3e-6), 5, 4) == EINVAL  # a rate mismatch
        for bad in (float("nan"), float("inf"), -1.0):
            assert _set(r, bad, 5, 4) == EINVAL and _set(r, rate, 5, 4, cutoff=bad) == EINVAL and _set(r, rate, 5, 4, width=bad) == EINVAL
        assert _set(r, rate, 5, 4, width=40e6) == EINVAL                                   # fewer than three taps
        assert _set(r, rate, 5, 4, cutoff=10.1e6) == EINVAL                                # above L rate / 2
        assert _set(r, rate, 5, 4, width=20e3) == E2BIG                                    # 3363 taps: 673 per phase
        # every refusal left the working stage working
        assert _same(before, r.debug_wideband_resample(x))
        # -EBUSY after a push, lifted by reset; the same for removing the stage
        assert _set(r, rate, 5, 4) == -errno.EBUSY and _set(r, rate, 5, 0) == -errno.EBUSY
        r.reset()
        assert _set(r, rate, 5, 4, width=rate / 8) == 0
        assert not _same(before, r.debug_wideband_resample(x))
        # the distributed push
        assert lib.amps_recc_push_wideband_dist(r._h, x.ctypes.data_as(C.c_void_p), len(x), capi.MEM_HOST, 0, 0, None) == -errno.ENOSYS
    # a handle without the wideband seam
    with capi.Recc(n_channels=1, sps=10, max_samples=1024, max_bursts=4) as r:
        assert _set(r, rate, 5, 4) == -errno.ENOSYS
        out, no = np.zeros(16, np.complex64), C.c_size_t(0)
        assert lib.amps_recc_debug_wideband_resample(r._h, x.ctypes.data_as(C.c_void_p), 4, FC32, capi.MEM_HOST, out.ctypes.data_as(C.c_void_p), 16, C.byref(no)) == -errno.ENOSYS


def test_too_large_a_push_consumes_nothing_and_decim_0_is_the_parent(gpu):
    rate, L, M, channels = wr.RATIOS[0]
    D, nch = DECIM[channels], 5
    n = _inputs_for(40 * D, L, M)
    x = _noise(9, n)
    with _handle(rate, L, M, channels, C=nch, first=7, max_frames=64) as r:
        one = r.debug_channelize(x)
    with _handle(rate, L, M, channels, C=nch, first=7, max_frames=24) as r:
        with pytest.raises(capi.AmpsError) as e:
            r.debug_channelize(x)
        assert e.value.code == -errno.E2BIG
        # nothing was consumed -- no index, no history moved: the same samples in two smaller pieces, straight after the refusal on the
        # state that the refusal left, give the one-push stream
        h = _inputs_for(20 * D, L, M)
        two = np.concatenate([r.debug_channelize(x[:h]), r.debug_channelize(x[h:])], axis=1)
    assert one.shape[1] == 40 and _same(one, two)
    # a separate matter: a refused push is no push, so the stage may still be reconfigured after it
    with _handle(rate, L, M, channels, C=nch, first=7, max_frames=24) as r:
        with pytest.raises(capi.AmpsError) as e:
            r.debug_channelize(x)
        assert e.value.code == -errno.E2BIG and _set(r, rate, L, M) == 0
    # decim = 0 removes the stage: the handle is a plain bank handle again, and so is one that never had a stage
    y = _noise(10, 40 * D)
    with _handle(rate, L, M, channels, C=nch, first=7, max_frames=64) as r, _handle(rate, L, M, channels, C=nch, first=7, max_frames=64, resample=False) as p:
        assert _set(r, 0.0, 0, 0) == 0
        out, no = np.zeros(16, np.complex64), C.c_size_t(0)
        assert capi.load().amps_recc_debug_wideband_resample(r._h, y.ctypes.data_as(C.c_void_p), 4, FC32, capi.MEM_HOST, out.ctypes.data_as(C.c_void_p), 16,
                                                             C.byref(no)) == -errno.ENOSYS
        r.resample = None
        assert _same(r.debug_channelize(y), p.debug_channelize(y))
