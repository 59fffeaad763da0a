"""-m gpu: the wideband seam at 15.36, 7.68 and 3.84 Msps -- the filter banks of 512, 256 and 128 branches (chz_narrow_kernel) at
D = M / 2 and 3 M / 4 -- against the float64 filter-bank model, against itself under other cuts of the stream, against the CPU model of
the IQ seam on the bank's own output, against the transmitted words, and, for received power and carrier offset, against the plain IQ
seam fed the bank's rows.  Every test runs over the six geometries (tests/narrowblock.py holds them and the burst block)."""
import errno
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import slicerbound as sb
import streampowerref as spr
from oracle import channelizer as cz
from gr_amps_amd import capi, synth_wideband as sw

import narrowblock as nb

pytestmark = pytest.mark.gpu
GEO = pytest.mark.parametrize("M,D", nb.GEOMETRIES, ids=nb.IDS)
HALF = pytest.mark.parametrize("M,D", [g for g in nb.GEOMETRIES if 2 * g[1] == g[0]], ids=[i for g, i in zip(nb.GEOMETRIES, nb.IDS) if 2 * g[1] == g[0]])
THREEQ = pytest.mark.parametrize("M,D", [g for g in nb.GEOMETRIES if 2 * g[1] != g[0]], ids=[i for g, i in zip(nb.GEOMETRIES, nb.IDS) if 2 * g[1] != g[0]])


def _handle(M, D, C, first, max_frames, max_bursts=64, **kw):
    return capi.Recc(n_channels=C, max_samples=max_frames, max_bursts=max_bursts, wideband={"channels": M, "decim": D, "first_channel": first}, **kw)


def _whole(M, D, nframes):
    """frames a stream of nframes * D samples and more has produced: launches are whole periods of the roll"""
    return nframes & ~1 if 2 * D == M else nframes & ~3


def _flush(D):
    return np.zeros(64 * D, np.complex64)


# ---- 1. against float64, bin by bin and frame by frame
@GEO
def test_bank_per_bin_error_on_a_wrapped_band(gpu, M, D):
    """|y32 - y64| <= c 2^-24 log2(M) ||Y64(frame)||_2 with c = slicerbound.FFT_C, the constant of the 1024 bank: the band wraps past
    bin M - 1, tones sit 3 kHz above the centres of bins 0, 1, M / 2 - 1, M / 2 and M - 1 over noise at 0.02; about 300 frames in
    ragged pieces, one shorter than a frame, one long enough for several workgroups (150 frames: 5 workgroups at 32 frames each, 38 at 4)."""
    fs = M * 30e3
    first, C = M - 8, M
    rng = np.random.default_rng(23 + M + D)
    n = 300 * D + 37
    t = np.arange(n)
    x = 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    tones = ((0, 1.0), (1, 0.8), (M // 2 - 1, 0.6), (M // 2, 0.9), (M - 1, 0.7))
    for k, a in tones:
        x += a * np.exp(2j * np.pi * (sw.bin_freq(k, fs, M) + 3e3) * t / fs)
    x = x.astype(np.complex64)
    pieces = [D - 5, 3 * D + 11, 150 * D + 11, 2 * D + 1]
    pieces.append(n - sum(pieces))
    with _handle(M, D, C, first, 320) as r:
        parts, off = [], 0
        for m in pieces:
            parts.append(r.debug_channelize(x[off:off + m]))
            off += m
        got = np.concatenate(parts, axis=1)
    assert parts[0].shape == (C, 0) and parts[2].shape[1] >= 148 and got.shape == (C, _whole(M, D, n // D))
    want = cz.channelize(x, P=8, M=M, D=D, taps=nb.taps(M, D))[:, :got.shape[1]]      # all M bins, float64
    norm = np.sqrt((np.abs(want) ** 2).sum(0))
    rows = (first + np.arange(C)) % M
    ratio = np.abs(got - want[rows]) / (sb.U32 * np.log2(M) * norm)
    print(f"\nM={M} D={D}: worst |y32 - y64| / (2^-24 log2(M) ||Y64(frame)||) = {ratio.max():.3f}")
    assert ratio.max() <= sb.FFT_C, (ratio.max(), np.unravel_index(np.argmax(ratio), ratio.shape))
    # the tones come out at full scale (unit DC gain, 3 kHz inside the pass band) on the rows the wrap says
    for k, a in tones:
        level = np.abs(got[(k - first) % M, 100:]).mean()
        assert 0.9 * a < level < 1.1 * a, (k, level)
    quiet = np.ones(C, bool)
    for k, _ in tones:
        quiet[[(k - first + d) % M for d in (-1, 0, 1)]] = False
    assert np.abs(got[quiet, 100:]).mean() < 0.02


# ---- 2. streaming equals one-shot
@GEO
def test_bank_streaming_equals_one_shot(gpu, M, D):
    rng = np.random.default_rng(2 + M + D)
    n = 20000 + 96 * D + 77
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    first, C = 5, M - 11
    with _handle(M, D, C, first, n // D + 8) as r:
        one = r.debug_channelize(x)
    with _handle(M, D, C, first, n // D + 8) as r:
        parts, off = [], 0
        for m in (1, D - 1, D, D + 1, 5000, 12345, n):
            m = min(m, n - off)
            assert m > 0
            parts.append(r.debug_channelize(x[off:off + m]))
            off += m
        many = np.concatenate(parts, axis=1)
    assert off == n and one.shape == (C, _whole(M, D, n // D)) and many.shape == one.shape
    assert np.array_equal(one.view(np.uint32), many.view(np.uint32))     # a frame's arithmetic does not depend on the cut
    assert np.abs(one).min() > 0                                          # every row and frame was written


# ---- 3. bursts
def _pushed_in_halves(r, x, D, short=False):
    n = x.shape[0]
    half = (n // 2) // D * D + 100
    push = r.push_wideband_short if short else r.push_wideband
    push(x[:half])
    push(x[half:])
    if short:
        push(np.zeros((64 * D, 2), np.int16))
    else:
        push(_flush(D))
    return r.drain()


@GEO
def test_narrow_bursts_decode_to_the_transmitted_words(gpu, M, D):
    sps = nb.sps_of(M, D)
    x, truth = nb.burst_block(M, D)
    n = x.shape[0]
    cap = (n + 64 * D) // D + 72
    with _handle(M, D, M, 0, cap) as r:
        assert r.sps == sps
        chan = r.debug_channelize(np.concatenate([x, _flush(D)]))
    with _handle(M, D, M, 0, cap) as r:
        got = _pushed_in_halves(r, x, D)
    assert len(got) == 6
    by_chan = {int(g["channel"]): g for g in got}
    for (k, off), (kind, min10, esn, dialed, words) in truth.items():
        g = by_chan[k]
        assert g["min"].decode() == min10 and capi.MSG_CLASSES[g["msg_class"]] == kind and g["valid"].all()
        for w, bits in enumerate(words):                       # the decoded words: at 20 dB a received bit may be one BCH has put right
            assert list(g["word_dec"][w]) == list(bits)             # (M = 128, D = 96, bin 127: one, in the float64 model's block too)
    # the kernels behind the bank are bit-exact against the CPU model when both see the bank's own output
    active = sorted(by_chan)
    want = oracle.fused_push_all(chan[active], sps=sps)
    want["channel"] = np.array(active, np.uint32)[want["channel"]]
    assert got.tobytes() == want.tobytes()
    # and the float64 bank leads to the same words
    ref = oracle.fused_push_all(nb.model_rows(M, D), sps=sps)
    assert len(ref) == 6
    for a in ref:
        g = by_chan[nb.planted(M)[int(a["channel"])][0]]
        assert a["min"] == g["min"] and np.array_equal(a["word_raw"], g["word_raw"])


# ---- 4. sc16
@GEO
def test_narrow_short_input_equals_the_converted_block(gpu, M, D):
    x, truth = nb.burst_block(M, D)
    n = x.shape[0]
    scale = 8000.0 / max(np.abs(x.real).max(), np.abs(x.imag).max())
    xi = np.rint(np.stack([x.real, x.imag], axis=1) * scale).astype(np.int16)            # [n, 2], within +-8000
    xf = np.ascontiguousarray(xi.astype(np.float32)).view(np.complex64)[:, 0]
    cap = (n + 64 * D) // D + 72
    with _handle(M, D, M, 0, cap) as r:
        want = _pushed_in_halves(r, xf, D)
    with _handle(M, D, M, 0, cap) as r:
        got = _pushed_in_halves(r, xi, D, short=True)
    assert len(want) == 6 and sorted(g["min"].decode() for g in want) == sorted(v[1] for v in truth.values())
    assert got.tobytes() == want.tobytes()
    # the two entry points push by push on one handle: the carry is fc32 whatever the block was
    with _handle(M, D, M, 0, cap) as r:
        cuts = [0, n // 5 + 3, n // 2 + D // 3, 3 * n // 4 + 1, n]
        for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            if i % 2 == 0:
                r.push_wideband_short(xi[a:b])
            else:
                r.push_wideband(xf[a:b])
        r.push_wideband(_flush(D))
        mixed = r.drain()
    assert mixed.tobytes() == want.tobytes()


# ---- 5. received power and carrier offset
def _bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


@HALF
def test_narrow_power_and_offset_equal_the_iq_seam_on_the_banks_rows(gpu, M, D):
    """D = M / 2: 60 ksps per channel, three samples per symbol, which the plain IQ seam takes too -- the narrow handle's records and
    rings are those of an IQ-seam handle fed the bank's rows.  Every mobile is planted 1500 Hz above its centre.  The offset read back
    for the burst in bin 5, the one whose neighbours on both sides are silent, is within 60 Hz of that (the IQ seam's own figure is 8 Hz
    at 10 dB; this only catches a wrong sample rate: 40 ksps for 60 would read 1000 Hz).  The other five are keyed at the same time as a
    mobile of equal power in the next channel, which pulls the unit-amplitude statistic: the float64 bank with the float64 statistic
    reads 1384 Hz in bin 0 at M = 128 (neighbours 1 and 127 both keyed; 1483 Hz in bin 5), and the device reads the same to 0.1 Hz.
    They are held to the plain IQ seam bit for bit like everything else here, and to 150 Hz against what was sent."""
    x, truth = nb.burst_block(M, D, 1500.0)
    n = x.shape[0]
    xz = np.concatenate([x, _flush(D)])
    cap = xz.shape[0] // D + 72
    with _handle(M, D, M, 0, cap) as r:
        chan = r.debug_channelize(xz)
    kw = dict(stream_power=True, stream_offset="unit")
    with _handle(M, D, M, 0, cap, **kw) as r:
        half = (n // 2) // D * D + 100
        r.push_wideband(xz[:half])
        r.push_wideband(xz[half:])
        recs = r.drain()
        power, pfirst = r.channel_power()
        ac, afirst = r.channel_autocorr()
        off_hz, off_n = r.burst_offset(recs)
        bp, bn = r.burst_power(recs)
    with capi.Recc(n_channels=M, sps=3, max_samples=chan.shape[1], max_bursts=64, **kw) as q:
        q.push_iq(chan)
        qrecs = q.drain()
        qpower, qpfirst = q.channel_power()
        qac, qafirst = q.channel_autocorr()
        qoff_hz, qoff_n = q.burst_offset(qrecs)
        qbp, qbn = q.burst_power(qrecs)
    assert len(recs) == 6 and recs.tobytes() == qrecs.tobytes()
    assert sorted(g["min"].decode() for g in recs) == sorted(v[1] for v in truth.values())
    assert pfirst == qpfirst == 0 and afirst == qafirst == 0
    assert power.shape == qpower.shape == (M, chan.shape[1] // 64 * 64 // 256) and np.array_equal(_bits32(power), _bits32(qpower))
    assert ac.shape == qac.shape == power.shape and np.array_equal(_bits32(ac), _bits32(qac))
    assert np.array_equal(_bits32(off_hz), _bits32(qoff_hz)) and np.array_equal(off_n, qoff_n) and np.array_equal(_bits32(bp), _bits32(qbp)) and np.array_equal(bn, qbn)
    print(f"\nM={M} D={D}: burst offsets {np.round(off_hz, 1)} Hz over {off_n} blocks (planted +1500)")
    assert [int(c) for c in recs["channel"]] == sorted(k for k, _ in nb.planted(M)) and off_n.min() > 30
    assert abs(float(off_hz[[int(c) for c in recs["channel"]].index(5)]) - 1500.0) <= 60.0, off_hz
    assert np.all(np.abs(off_hz - 1500.0) <= 150.0), off_hz


@THREEQ
def test_narrow_power_and_offset_rings_at_two_samples_per_symbol(gpu, M, D):
    """D = 3 M / 4: 40 ksps per channel, which the plain IQ seam does not take -- the rings are the same under another cut, and the
    power blocks are within 2e-5 relative (the bound tests/test_gpu_stream_power.py derives: 257 u) of the float64 mean of |y|^2 over
    blocks of 256 of the bank's own output."""
    x, truth = nb.burst_block(M, D)
    n = x.shape[0]
    xz = np.concatenate([x, _flush(D)])
    cap = xz.shape[0] // D + 72
    with _handle(M, D, M, 0, cap) as r:
        chan = r.debug_channelize(xz)
    outs = []
    for cuts in ([0, (n // 2) // D * D + 100, xz.shape[0]], [0, 7 * D + 5, n // 3, n // 3 + D - 1, 2 * n // 3 + 17, xz.shape[0]]):
        with _handle(M, D, M, 0, cap, stream_power=True, stream_offset="unit") as r:
            for a, b in zip(cuts[:-1], cuts[1:]):
                r.push_wideband(xz[a:b])
            recs = r.drain()
            power, pfirst = r.channel_power()
            ac, afirst = r.channel_autocorr()
            outs.append((recs, power, ac))
            assert pfirst == 0 and afirst == 0
    assert len(outs[0][0]) == 6 and outs[0][0].tobytes() == outs[1][0].tobytes()
    assert np.array_equal(_bits32(outs[0][1]), _bits32(outs[1][1])) and np.array_equal(_bits32(outs[0][2]), _bits32(outs[1][2]))
    power = outs[0][1]
    want = spr.blocks(chan[:, :chan.shape[1] // 64 * 64])
    assert power.shape == want.shape and want.min() > 0
    err = np.abs(power.astype(np.float64) - want) / want
    print(f"\nM={M} D={D}: worst |P_gpu - P_ref| / P_ref = {err.max():.3g} (bound 2e-5) over {want.size} blocks")
    assert np.all(err <= 2e-5)


# ---- 6. refusals
def test_narrow_refusals(gpu):
    def refused(wb, n_channels=4, **kw):
        with pytest.raises(capi.AmpsError) as e:
            capi.Recc(n_channels=n_channels, max_samples=1024, max_bursts=16, wideband=wb, **kw)
        return e.value.code

    assert refused({"channels": 1000}) == -errno.EINVAL
    assert refused({"channels": 64}) == -errno.EINVAL
    assert refused({"channels": 512, "decim": 768}) == -errno.EINVAL
    for M in (512, 256, 128):
        assert refused({"channels": M, "groups": 2}) == -errno.EINVAL
        assert refused({"channels": M}, channel_power=True) == -errno.EINVAL
        assert refused({"channels": M}, n_channels=M + 1) == -errno.EINVAL
    assert refused({"channels": 1024}, stream_power=True) == -errno.EINVAL               # still the IQ and translate seams' flag at M = 1024
    for M, D in nb.GEOMETRIES:
        with _handle(M, D, M, 0, 1024, unfused_wideband=(D * 2 == M)) as r:              # the flag is accepted and changes nothing
            with pytest.raises(capi.AmpsError) as e:
                r.rccl_init(bytes(128), 1, 0)
            assert e.value.code == -errno.ENOSYS


# ---- 7. host block and example
@pytest.mark.parametrize("ext", ["fc32", "sc16"])
def test_recctest_wide_with_channels_128(gpu, tmp_path, ext):
    """gr::amps::recc_wideband::make(128, 0, ..., channels = 128) through recctest: a 3.84 Msps capture file in, the lines of the six
    bursts out, as the C ABI's own records give them"""
    from gr_amps_amd.host import build_host
    from test_gpu_host_blocks import _expected_lines
    M, D = 128, 96                                               # the default decimation
    x, truth = nb.burst_block(M, D)
    p = tmp_path / ("block." + ext)
    if ext == "sc16":
        scale = 8000.0 / max(np.abs(x.real).max(), np.abs(x.imag).max())
        xi = np.rint(np.stack([x.real, x.imag], axis=1) * scale).astype(np.int16)
        xi.tofile(p)
        x = np.ascontiguousarray(xi.astype(np.float32)).view(np.complex64)[:, 0]
    else:
        x.tofile(p)
    with capi.Recc(n_channels=M, max_samples=(x.shape[0] + 64 * 768) // D + 72, max_bursts=64, wideband={"channels": M}) as r:
        assert r.decim == D and r.sps == 2
        r.push_wideband(x)
        r.push_wideband(np.zeros(64 * 768, np.complex64))        # recctest's own tail of silence
        recs = r.drain()
    assert sorted(int(g["channel"]) for g in recs) == sorted(k for k, _ in nb.planted(M))
    want = []
    for g in recs:
        want.append("MSG channel %d" % int(g["channel"]))
        want += _expected_lines(recs[recs["channel"] == g["channel"]])
    _, exe = build_host()
    out = subprocess.run([exe, "wide", str(p), "777777", "channels=128"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = [l for l in out.stdout.splitlines() if l.startswith("MSG ")]
    assert sorted(got) == sorted(want) and len([l for l in got if l.startswith("MSG channel")]) == 6


def test_example_decodes_a_3_84_msps_stream(gpu):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "decode_wideband.py"), "--channels", "128"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "MISMATCH" not in out.stdout and " decoded" in out.stdout
