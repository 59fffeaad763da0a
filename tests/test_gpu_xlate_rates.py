"""-m gpu: the shared translate seam at the rates SDRs deliver -- decimations 5, 6, 10, 12, 16 and 20 (1.0 ... 3.2 Msps, filters of up
to 2400 taps) through xlate_shared_wide_kernel.

No older kernel has these decimations, so the stage is held to its definition directly: the exact formula in float64 within the bound
tests/test_gpu_xlate_shared.py derived for decimation 8; bit identity across pushes, tiles, grids, channel groups and sample formats;
the words against the restated reference chain behind the restated filter (oracle.freq_xlating_fir + oracle.chain_iq200); and, at an
output rate other than 200 ksps, the records of a plain IQ-seam handle fed the stage's own output."""
import errno
import functools
import subprocess

import numpy as np
import pytest

import oracle
from gr_amps_amd import capi, synth
from gr_amps_amd.host import build_host

pytestmark = pytest.mark.gpu

SPACING = 3456 + 74 + 4096 + 600      # symbols between two bursts of a channel, as tests/test_gpu_xlate.py plants them
FS24 = 2.4e6
CENTRES_24 = [-1.05e6, -615e3, 15e3, 45e3, 1.11e6]    # two of them adjacent
FIELDS = ("msg_class", "a_MIN1", "b_MIN2", "esn", "dialed", "min")


def _exact(x, taps, fc, fs, decim):
    """the float64 formula of tests/test_gpu_xlate.py"""
    n = np.arange(x.size)
    z = x.astype(np.complex128) * np.exp(-2j * np.pi * fc * n / fs)
    full = np.convolve(z, np.asarray(taps, np.float64))[: x.size]
    return full[::decim][: x.size // decim]


def _noise(seed, n, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) * np.float32(scale)


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 1. the exact formula at every new decimation
@pytest.mark.parametrize("fs,decim,sps", [(1.0e6, 5, 10), (1.2e6, 6, 10), (2.0e6, 10, 10), (2.4e6, 12, 10), (3.2e6, 16, 10), (2.4e6, 20, 6)],
                         ids=["1000k_d5", "1200k_d6", "2000k_d10", "2400k_d12", "3200k_d16", "2400k_d20"])
def test_new_decimations_meet_the_exact_formula(gpu, fs, decim, sps):
    """2048 outputs: eight tiles of 256 and a ragged end.  The bound is that of test_decim_8_meets_the_exact_formula
    (tests/test_gpu_xlate_shared.py): (ntaps + 16) * 2^-24 * sum|h| * max|x| per output sample; an indexing error (a tap or a sample
    off by one) is of the order of the output itself, which the second assertion keeps far above the bound."""
    n = 2048 * decim + 1
    centres = [-0.384375 * fs, 15e3, 0.4375 * fs]
    x = _noise(12, n, 0.5)
    taps = oracle.firdes_low_pass(3, fs, 10e3, 4.5e3)
    assert (decim, sps, len(taps)) in capi.subband_plan(fs)
    with capi.Recc(n_channels=3, sps=sps, max_samples=n, max_bursts=4) as r:
        r.set_xlate_shared(fs, centres, decim)
        y = r.debug_xlate_shared(x)
    assert y.shape == (3, 2048)
    bound = (len(taps) + 16) * 2.0 ** -24 * np.abs(taps.astype(np.float64)).sum() * np.abs(x).max()
    for c, fc in enumerate(centres):
        e = _exact(x, taps, fc, fs, decim)
        err = np.abs(y[c] - e).max()
        print("%g Msps / %d, centre %+.1f kHz: max |y - exact| = %.3g, bound %.3g, max |exact| = %.3g" % (fs / 1e6, decim, fc / 1e3, err, bound, np.abs(e).max()))
        assert err <= bound, (fc, err, bound)
        assert np.abs(e).max() > 100 * bound


# ---- 2. streaming
@pytest.mark.parametrize("decim", [5, 12, 20])
@pytest.mark.parametrize("blocks", [[1, 2, 3, 298, 299, 300, 4097], [2047, 2049, 1, 1, 1], [7777] * 5, [3, 1, 7, 2, 19, 4001]],
                         ids=["ragged", "tile_edges", "even", "short_of_one_output"])
def test_streaming_is_bitwise(gpu, blocks, decim):
    """ragged pushes (pieces smaller than the decimation produce no output, several in a row) equal one push; a host block equals a
    device block; reset restarts the stream"""
    import torch
    n = sum(blocks)
    x = _noise(13, n)
    sps = 6 if decim == 20 else 10                                 # 2.4 Msps / 20: 4 Msps would need a wider transition
    fs = 20e3 * sps * decim
    centres = [-0.4 * fs, 0.09375 * fs, 0.4 * fs]
    with capi.Recc(n_channels=3, sps=sps, max_samples=n, max_bursts=4) as r:
        r.set_xlate_shared(fs, centres, decim)
        whole = r.debug_xlate_shared(x)
        r.reset()
        parts, o = [], 0
        for b in blocks:
            parts.append(r.debug_xlate_shared(x[o:o + b]))
            o += b
        ragged = np.concatenate(parts, axis=1)
        r.reset()
        dev = r.debug_xlate_shared(torch.from_numpy(x).to(gpu))
        r.reset()
        again = r.debug_xlate_shared(x)
    assert whole.shape == (3, n // decim) and np.abs(whole).max() > 0
    ends = np.cumsum(blocks)
    assert [p.shape[1] for p in parts] == [int(e // decim - (e - b) // decim) for e, b in zip(ends, blocks)]   # zeros among them
    for name, got in (("ragged", ragged), ("device", dev), ("after reset", again)):
        assert _bits_equal(got, whole), name


# ---- 3. independence of the grid
def test_a_row_does_not_depend_on_the_other_channels(gpu):
    """row c of a five-centre handle (one centre twice) == row 0 of a one-channel shared handle with centre c: neither the number of
    workgroups nor a channel's place in the grid reaches the bits"""
    fs, decim, n = FS24, 12, 30001
    centres = [-1.05e6, 37.5e3, 0.0, 37.5e3, 1.11e6]
    x = _noise(11, n, 0.5)
    with capi.Recc(n_channels=5, sps=10, max_samples=n, max_bursts=4) as r:
        r.set_xlate_shared(fs, centres, decim)
        y = r.debug_xlate_shared(x)
    assert y.shape == (5, n // decim)
    for c, fc in enumerate(centres):
        with capi.Recc(n_channels=1, sps=10, max_samples=n, max_bursts=4) as r:
            r.set_xlate_shared(fs, [fc], decim)
            one = r.debug_xlate_shared(x)
        assert _bits_equal(one[0], y[c]), c
    assert _bits_equal(y[1], y[3]) and not _bits_equal(y[1], y[2])


# ---- 4. sample formats
FORMATS = {"sc16": capi.SAMPLES_SC16, "sc8": capi.SAMPLES_SC8, "cu8": capi.SAMPLES_CU8}
CONFIGS = {"2400k_d12": (FS24, 12, (-1.05e6, 15e3, 615e3)), "2000k_d10": (2.0e6, 10, (-615e3, 15e3))}


def _ints(fmt, n, seed=31):
    """[n, 2] random samples over the whole range of the format, both extremes planted in I and in Q"""
    info = np.iinfo(capi.SAMPLE_DTYPES[fmt])
    rng = np.random.default_rng(seed + fmt)
    a = rng.integers(info.min, info.max + 1, size=(n, 2)).astype(capi.SAMPLE_DTYPES[fmt])
    for i, pair in zip((0, 1, 2, 3, 300, 2047, 2048, n - 1),
                       ((info.min, info.max), (info.max, info.min), (info.min, info.min), (info.max, info.max)) * 2):
        a[i % n] = pair
    return a


def _shared(cfg, max_samples):
    fs, D, centres = CONFIGS[cfg]
    r = capi.Recc(n_channels=len(centres), sps=10, max_samples=max_samples, max_bursts=4)
    r.set_xlate_shared(fs, list(centres), D)
    return r


@pytest.mark.parametrize("name,cfg", [("cu8", "2400k_d12"), ("sc16", "2400k_d12"), ("sc8", "2000k_d10")])
def test_integer_blocks_equal_the_fc32_path(gpu, name, cfg):
    """three output tiles, the last one partial.  As a host array, as a device tensor, and as a device tensor that starts at an odd
    sample (aligned to one sample only): each the bits of the fc32 call on the converted block"""
    import torch
    fmt, D = FORMATS[name], CONFIGS[cfg][1]
    n = 2 * 256 * D + 301
    x = _ints(fmt, n)
    xf = capi.convert_samples(x, fmt)
    t = torch.from_numpy(x).to(gpu)
    with _shared(cfg, n) as r:
        want = r.debug_xlate_shared(xf)
        r.reset()
        want_odd = r.debug_xlate_shared(xf[1:])
        r.reset()
        host = r.debug_xlate_shared_as(x, fmt)
        r.reset()
        dev = r.debug_xlate_shared_as(t, fmt)
        r.reset()
        odd = r.debug_xlate_shared_as(t[1:], fmt)
    assert want.shape == (len(CONFIGS[cfg][2]), n // D) and np.abs(want).max() > 0
    assert _bits_equal(host, want), "host block"
    assert _bits_equal(dev, want), "device block"
    assert _bits_equal(odd, want_odd), "device block from an odd sample"


def test_formats_mix_on_one_handle(gpu):
    """seven pushes, each in another format over its own full range: the rows of ONE fc32 push of the converted stream"""
    blocks = [1, 2, 3, 298, 299, 300, 4097]
    order = [capi.SAMPLES_CU8, capi.SAMPLES_FC32, capi.SAMPLES_SC16, capi.SAMPLES_SC8, capi.SAMPLES_CU8, capi.SAMPLES_FC32, capi.SAMPLES_SC16]
    rng = np.random.default_rng(59)
    raw = [(rng.standard_normal((b, 2)) * 1000).astype(np.float32) if f == capi.SAMPLES_FC32 else _ints(f, b, seed=59 + i)
           for i, (f, b) in enumerate(zip(order, blocks))]
    whole = np.concatenate([capi.convert_samples(a, f) for a, f in zip(raw, order)])
    with _shared("2400k_d12", whole.size) as r:
        want = r.debug_xlate_shared(whole)
        r.reset()
        parts = [r.debug_xlate_shared_as(a, f) for a, f in zip(raw, order)]
    assert want.shape[1] == whole.size // 12 and np.abs(want).max() > 0
    assert _bits_equal(np.concatenate(parts, axis=1), want)


# ---- 5. words against the restated reference chain at 2.4 Msps / 12
@functools.lru_cache(maxsize=None)
def _stream24(s):
    """five mobiles' channels in one second of a 2.4 Msps stream, bursts overlapping in time, two of the channels adjacent"""
    n = 2400000
    k = np.arange(n)
    x = np.zeros(n, np.complex128)
    truth = []
    for c, fc in enumerate(CENTRES_24):
        iq, t = synth.make_channel_block(n, 5, seed=s + c, sps=120, snr_db=30, first=4000 + 54000 * c, spacing=SPACING * 120)
        x += iq * np.exp(2j * np.pi * fc * k / FS24)
        truth.append(t)
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x, truth


def _sent(truth):
    return sorted((c, b[2]) for c, t in enumerate(truth) for b in t)


@pytest.mark.parametrize("s", [6100, 6200])
def test_words_equal_the_reference_chain_channel_by_channel(gpu, s):
    x, truth = _stream24(s)
    assert len(_sent(truth)) == 11
    with capi.Recc(n_channels=5, sps=10, max_samples=x.size // 12, max_bursts=64) as r:
        r.set_xlate_shared(FS24, CENTRES_24, 12)
        for part in np.array_split(x, 5):                           # ragged pushes
            r.push_raw_shared(part)
        got = r.drain()
    assert sorted((int(g["channel"]), g["min"].decode()) for g in got) == _sent(truth)
    taps = oracle.firdes_low_pass(3, FS24, 10e3, 4.5e3)
    assert len(taps) == 1793
    n_ref = 0
    for c, fc in enumerate(CENTRES_24):
        by_min = {g["min"]: g for g in got[got["channel"] == c]}
        ref = oracle.chain_iq200(oracle.freq_xlating_fir(x, taps, fc, FS24, 12), chunk=4096)
        for rr in ref:
            assert rr["min"] in by_min, "reference decoded a burst the GPU path missed on channel %d" % c
            g = by_min[rr["min"]]
            assert np.array_equal(rr["word_raw"], g["word_raw"])
            assert np.array_equal(rr["word_dec"], g["word_dec"])
            assert np.array_equal(rr["valid"], g["valid"]) and np.array_equal(rr["dcc"], g["dcc"])
            for f in FIELDS:
                assert rr[f] == g[f], f
        n_ref += len(ref)
    print("seed %d: the reference chain decoded %d of the 11 bursts the GPU path decoded" % (s, n_ref))
    assert n_ref >= 10, n_ref


# ---- 6. an output rate other than 200 ksps: 2.4 Msps / 20, six samples per symbol
def test_six_samples_per_symbol_records_are_those_of_the_iq_seam(gpu):
    """the stage's plumbing into the fused chain at 120 ksps: the records of set_xlate_shared + push_raw_shared are, byte for byte,
    those of a plain IQ-seam handle given the rows a second handle's debug_xlate_shared makes of the same pushes.  Condition: the CPU
    model on the restated filter's output decodes the 11 planted bursts and nothing else."""
    x, truth = _stream24(7100)
    sent = _sent(truth)
    assert len(sent) == 11
    parts = np.array_split(x, 5)
    nmax = x.size // 20
    with capi.Recc(n_channels=5, sps=6, max_samples=nmax, max_bursts=64) as r:
        r.set_xlate_shared(FS24, CENTRES_24, 20)
        for part in parts:
            r.push_raw_shared(part)
        got = r.drain()
    with capi.Recc(n_channels=5, sps=6, max_samples=nmax, max_bursts=64) as stage, \
         capi.Recc(n_channels=5, sps=6, max_samples=nmax, max_bursts=64) as plain:
        stage.set_xlate_shared(FS24, CENTRES_24, 20)
        for part in parts:
            rows = stage.debug_xlate_shared(part)
            if rows.shape[1]:
                plain.push_iq(np.ascontiguousarray(rows))
        want = plain.drain()
    assert got.tobytes() == want.tobytes()
    assert sorted((int(g["channel"]), g["min"].decode()) for g in got) == sent
    taps = oracle.firdes_low_pass(3, FS24, 10e3, 4.5e3)
    model = oracle.fused_push_all(np.stack([oracle.freq_xlating_fir(x, taps, fc, FS24, 20) for fc in CENTRES_24]), sps=6)
    assert sorted((int(m["channel"]), m["min"].decode()) for m in model) == sent


# ---- 7. errors
def test_errors(gpu):
    L = capi.load()
    cen = (capi.C.c_double * 2)(-60e3, 60e3)

    def cfg(decim, rate, width=0.0):
        return capi.XlateSharedCfg(capi.C.sizeof(capi.XlateSharedCfg), decim, 2, 0, rate, 0.0, 0.0, width, cen)

    def rc(r, x):
        return L.amps_recc_set_xlate_shared(r._h, capi.C.byref(x))

    x = _noise(17, 4800, 0.5)
    with capi.Recc(n_channels=2, sps=10, max_samples=4096, max_bursts=4) as r:
        for decim in (3, 7, 9, 24):                                # no such decimation, at a rate that would match
            assert rc(r, cfg(decim, 200e3 * decim)) == -errno.EINVAL, decim
        assert rc(r, cfg(12, 2.0e6)) == -errno.EINVAL              # 166.7 ksps is not 10 samples per symbol
        assert rc(r, cfg(16, 3.2e6, 2.25e3)) == -errno.E2BIG       # 4783 taps
        assert rc(r, cfg(8, 1.6e6, 2.25e3)) == -errno.E2BIG        # 2391 taps: the limit of decimation 8 did not move
        assert L.amps_recc_push_raw_shared(r._h, capi._hostptr(x), 16, capi.MEM_HOST) == -errno.ENOSYS   # nothing was configured
        # a refused configuration leaves the stage as it was
        assert rc(r, cfg(12, FS24)) == 0
        before = r.debug_xlate_shared(x)
        for bad in (cfg(7, 1.4e6), cfg(12, 2.0e6), cfg(16, 3.2e6, 2.25e3)):
            assert rc(r, bad) < 0
        r.reset()
        assert _bits_equal(r.debug_xlate_shared(x), before) and before.shape == (2, 400) and np.abs(before).max() > 0
        # the limit of one push
        big = np.zeros(12 * 4096 + 1, np.complex64)
        assert L.amps_recc_push_raw_shared(r._h, capi._hostptr(big), 12 * 4096, capi.MEM_HOST) == 0
        assert L.amps_recc_push_raw_shared(r._h, capi._hostptr(big), 12 * 4096 + 1, capi.MEM_HOST) == -errno.E2BIG
        # the per-row form keeps 1, 2 and 4
        one = capi.XlateCfg(capi.C.sizeof(capi.XlateCfg), 12, FS24, 15e3, 0.0, 0.0, 0.0)
        assert L.amps_recc_set_xlate(r._h, capi.C.byref(one)) == -errno.EINVAL
        assert L.amps_recc_push_raw_shared(r._h, capi._hostptr(x), 16, capi.MEM_HOST) == 0               # and refusing left the shared stage


# ---- 8. recctest sub
def _bits(a):
    return "".join(str(int(b)) for b in a)


def _expected_lines(records):
    """what recc_decode publishes for these records, as recctest prints it (tests/test_gpu_host_blocks.py)"""
    lines = []
    for rec in records:
        r = oracle.reply_words(rec)
        if r.has_focc:
            lines.append(f"MSG focc_words stream={r.focc_stream} n={r.focc_nwords} w1={_bits(r.focc_word1)} w2={_bits(r.focc_word2)}")
        if r.has_fvc:
            lines.append(f"MSG fvc_words n={r.fvc_count} w1={_bits(r.fvc_word1)} repeat={r.fvc_repeat}")
        if r.has_mutes:
            lines.append(f"MSG fvc_mute {r.fvc_mute}")
            lines.append(f"MSG audio_mute {r.audio_mute}")
        if r.has_command:
            lines.append("MSG command_out " + r.command.decode())
    return lines


def test_recctest_sub_at_an_rtl_sdr_rate(gpu, tmp_path):
    """gr::amps::recc_subband through `recctest sub capture.cu8 <chunk> 2400000 12 <centres>`: the five-channel stream quantised as
    an RTL-SDR would (offset binary, 16 per unit amplitude: the five carriers sum to well under 127), in ragged work() calls; per
    channel the lines of the bursts the binding returns for the same samples, in order"""
    x, truth = _stream24(6100)
    v = np.stack([x.real, x.imag], -1).astype(np.float64) * 16.0
    assert np.abs(v).max() < 127.0
    q = np.floor(v + 128.0).astype(np.uint8)
    with capi.Recc(n_channels=5, sps=10, max_samples=x.size // 12, max_bursts=64) as r:
        r.set_xlate_shared(FS24, CENTRES_24, 12)
        for part in np.array_split(q, 5):
            r.push_raw_shared_as(part, capi.SAMPLES_CU8)
        recs = r.drain()
    assert sorted((int(g["channel"]), g["min"].decode()) for g in recs) == _sent(truth)
    p = tmp_path / "capture.cu8"
    q.tofile(p)
    _, exe = build_host()
    out = subprocess.run([exe, "sub", str(p), "777777", "2400000", "12", ",".join("%g" % c for c in CENTRES_24)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got, ch = {}, None
    for line in out.stdout.splitlines():
        if line.startswith("MSG channel "):
            ch = int(line.split()[2])
            got.setdefault(ch, [])
        elif line.startswith("MSG "):
            got[ch].append(line)
    want = {c: _expected_lines(recs[recs["channel"] == c]) for c in range(5)}
    assert got == want and all(len(v) >= 2 for v in want.values())
    assert sum(out.stdout.count("MSG channel %d\n" % c) for c in range(5)) == len(recs) == 11


# ---- 9. the example
def test_example_decodes_both_systems_from_one_rtl_sdr_stream(gpu):
    """examples/decode_subband.py --rtl: the 42 control channels of both systems from one 2.4 Msps cu8 stream at / 12, every MIN back"""
    import os
    import sys
    script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "decode_subband.py")
    p = subprocess.run([sys.executable, script, "--rtl"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert "42 bursts sent, 42 decoded" in p.stdout and "MISMATCH" not in p.stdout
    assert p.stdout.count("  MIN ") == 42
