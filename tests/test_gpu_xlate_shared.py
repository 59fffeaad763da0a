"""-m gpu: the shared form of the translate seam (amps_recc_set_xlate_shared / _push_raw_shared / _debug_xlate_shared): ONE narrowband
fc32 stream holding many 30 kHz channels, every centre translated, filtered and decimated by xlate_shared_kernel and decoded by the
fused IQ seam behind it.

The definition (include/amps_recc.h) is an identity: row c of the shared stage is, bit for bit, what the existing one-channel stage
(amps_recc_set_xlate with centre c + amps_recc_debug_xlate / _push_raw) makes of the same samples.  Most checks here hold the new
kernel to that; decimation 8, which the existing kernel does not have, is held to the exact formula in float64 within a derived bound;
the words are held to the restated reference chain (oracle.chain_iq400) channel by channel."""
import errno
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle
from gr_amps_amd import capi, synth
from gr_amps_amd.host import build_host

pytestmark = pytest.mark.gpu

TOL_EXACT = 2.0e-5                    # tests/test_gpu_xlate.py: unit-amplitude input, taps of DC gain 3, 299 fp32 fma + the fp32 mix
SPACING = 3456 + 74 + 4096 + 600      # symbols between two bursts of a channel, as tests/test_gpu_xlate.py plants them
CENTRES_400 = [-160e3, -70e3, 20e3, 50e3, 160e3]


def _exact(x, taps, fc, fs, decim):
    """the float64 formula of tests/test_gpu_xlate.py"""
    n = np.arange(x.size)
    z = x.astype(np.complex128) * np.exp(-2j * np.pi * fc * n / fs)
    full = np.convolve(z, np.asarray(taps, np.float64))[: x.size]
    return full[::decim][: x.size // decim]


def _noise(seed, n, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) * np.float32(scale)


def _one_channel_rows(x, fs, centres, decim, sps, **filt):
    """what the existing kernel gives a one-channel handle per centre"""
    rows = []
    for fc in centres:
        with capi.Recc(n_channels=1, sps=sps, max_samples=x.size, max_bursts=4) as r:
            r.set_xlate(rate_hz=fs, center_hz=fc, decim=decim, **filt)
            rows.append(r.debug_xlate(x[None, :])[0])
    return np.stack(rows)


# ---- 1. bit identity with the existing kernel
@pytest.mark.parametrize("fs,decim,sps,centres,filt", [
    (400e3, 2, 10, [-160e3, 37.5e3, 0.0, 37.5e3, 160e3], {}),
    (200e3, 1, 10, [-90e3, 12.5e3, 60e3], {}),
    (400e3, 4, 5, [-160e3, 44e3, 130e3], {"gain": 1.0, "cutoff_hz": 12e3, "width_hz": 6e3}),
], ids=["400k_d2", "200k_d1", "400k_d4"])
def test_rows_are_bit_identical_to_the_one_channel_kernel(gpu, fs, decim, sps, centres, filt):
    n = 30001
    x = _noise(11, n, 0.5)
    with capi.Recc(n_channels=len(centres), sps=sps, max_samples=n, max_bursts=4) as r:
        r.set_xlate_shared(fs, centres, decim, **filt)
        y = r.debug_xlate_shared(x)
    want = _one_channel_rows(x, fs, centres, decim, sps, **filt)
    assert y.shape == want.shape == (len(centres), n // decim)
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32))
    if not filt and decim == 2:
        taps = oracle.firdes_low_pass(3, fs, 10e3, 4.5e3)
        assert len(taps) == 299
        for c, fc in enumerate(centres):
            err = np.abs(y[c] - _exact(x, taps, fc, fs, decim)).max()
            print("centre %+.1f kHz: max |y - exact| = %.3g" % (fc / 1e3, err))
            assert err <= TOL_EXACT, (fc, err)


# ---- 2. decimation 8: no existing kernel to compare with
def test_decim_8_meets_the_exact_formula(gpu):
    """1.6 Msps at 10 samples per symbol: the flow graph's filter spec gives 1195 taps.  Bound on |y - exact| per output sample: every
    product and every sum of the chain is rounded once (relative 2^-24; the running sum never exceeds sum|h| max|x|), that is at most
    ntaps roundings, and the mix adds the cmul's roundings and a phase exact to 2^-24 turn (2 pi 2^-24 relative) -- fewer than 16 more
    units of the same size: (ntaps + 16) * 2^-24 * sum|h| * max|x|.  Loose by the square root of ntaps or so, but an indexing error
    (a tap or a sample off by one) is of the order of the output itself."""
    fs, n, centres = 1.6e6, 40001, [-615e3, 15e3, 700e3]
    x = _noise(12, n, 0.5)
    taps = oracle.firdes_low_pass(3, fs, 10e3, 4.5e3)
    assert len(taps) == 1195
    with capi.Recc(n_channels=3, sps=10, max_samples=n, max_bursts=4) as r:
        r.set_xlate_shared(fs, centres, 8)
        y = r.debug_xlate_shared(x)
    assert y.shape == (3, n // 8)
    bound = (len(taps) + 16) * 2.0 ** -24 * np.abs(taps.astype(np.float64)).sum() * np.abs(x).max()
    for c, fc in enumerate(centres):
        e = _exact(x, taps, fc, fs, 8)
        err = np.abs(y[c] - e).max()
        print("centre %+.1f kHz: max |y - exact| = %.3g, bound %.3g, max |exact| = %.3g" % (fc / 1e3, err, bound, np.abs(e).max()))
        assert err <= bound, (fc, err, bound)
        assert np.abs(e).max() > 100 * bound                     # the bound is far below the signal: an indexing error cannot hide in it


# ---- 3. streaming
@pytest.mark.parametrize("decim", [2, 8])
@pytest.mark.parametrize("blocks", [[1, 2, 3, 298, 299, 300, 4097], [2047, 2049, 1, 1, 1], [7777] * 5])
def test_streaming_is_bitwise(gpu, blocks, decim):
    """ragged pushes (odd sizes leave samples waiting for the decimator) equal one push; a host block equals a device block; reset
    restarts the stream"""
    import torch
    n = sum(blocks)
    x = _noise(13, n)
    fs = 200e3 * decim
    centres = [-0.4 * fs, 0.09375 * fs, 0.4 * fs]
    with capi.Recc(n_channels=3, sps=10, max_samples=n, max_bursts=4) as r:
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
    assert whole.shape == (3, n // decim)
    for name, got in (("ragged", ragged), ("device", dev), ("after reset", again)):
        assert got.shape == whole.shape, name
        assert np.array_equal(got.view(np.uint32), whole.view(np.uint32)), name


# ---- 4. words against the restated reference chain
@functools.lru_cache(maxsize=None)
def _stream400(s):
    """five mobiles' channels in one 400 ksps stream: two bursts each, overlapping in time, two of the channels adjacent"""
    n = 400000
    k = np.arange(n)
    x = np.zeros(n, np.complex128)
    truth = []
    for c, fc in enumerate(CENTRES_400):
        iq, t = synth.make_channel_block(n, 5, seed=s + c, sps=20, first=4000 + 9000 * c, spacing=SPACING * 20)
        x += iq * np.exp(2j * np.pi * fc * k / 400e3)
        truth.append(t)
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x, truth


def _push_stream400(x):
    with capi.Recc(n_channels=len(CENTRES_400), sps=10, max_samples=x.size // 2, max_bursts=64) as r:
        r.set_xlate_shared(400e3, CENTRES_400, 2)
        for part in np.array_split(x, 5):                       # ragged pushes
            r.push_raw_shared(part)
        return r.drain()


@pytest.mark.parametrize("s", [4100, 4200, 4300])
def test_words_equal_the_reference_chain_channel_by_channel(gpu, s):
    x, truth = _stream400(s)
    assert [len(t) for t in truth] == [2] * 5
    got = _push_stream400(x)
    assert len(got) == 10
    n_ref = 0
    for c, fc in enumerate(CENTRES_400):
        mine = got[got["channel"] == c]
        assert sorted(g["min"].decode() for g in mine) == sorted(t[2] for t in truth[c])
        by_min = {g["min"]: g for g in mine}
        ref = oracle.chain_iq400(x, fc, chunk=4096)
        for rr in ref:
            assert rr["min"] in by_min, "reference decoded a burst the GPU path missed on channel %d" % c
            g = by_min[rr["min"]]
            assert np.array_equal(rr["word_raw"], g["word_raw"])
            assert np.array_equal(rr["word_dec"], g["word_dec"])
            assert np.array_equal(rr["valid"], g["valid"]) and np.array_equal(rr["dcc"], g["dcc"])
            for f in ("msg_class", "a_MIN1", "b_MIN2", "esn", "dialed", "min"):
                assert rr[f] == g[f], f
        n_ref += len(ref)
    print("seed %d: the reference chain decoded %d of the 10 bursts the GPU path decoded" % (s, n_ref))
    assert n_ref >= 9, n_ref


# ---- 5. a system's 21 control channels from one 800 ksps stream
@pytest.mark.parametrize("base", [5100, 5200])
def test_a_systems_control_channels(gpu, base):
    n, fs = 800000, 800e3
    centres = [-300e3 + 30e3 * i for i in range(21)]
    k = np.arange(n)
    x = np.zeros(n, np.complex128)
    sent = []
    for c, fc in enumerate(centres):
        iq, t = synth.make_channel_block(n, 2, seed=base + c, sps=40, snr_db=40, first=4000 + 7000 * c, spacing=SPACING * 40)
        x += iq * np.exp(2j * np.pi * fc * k / fs)
        assert len(t) == 2
        sent += [(c, b[2]) for b in t]
    x = x.astype(np.complex64)
    with capi.Recc(n_channels=21, sps=10, max_samples=n // 4, max_bursts=128) as r:
        r.set_xlate_shared(fs, centres, 4)
        r.push_raw_shared(x)
        got = r.drain()
    assert sorted((int(g["channel"]), g["min"].decode()) for g in got) == sorted(sent) and len(sent) == 42
    want = []
    for c, fc in enumerate(centres):
        with capi.Recc(n_channels=1, sps=10, max_samples=n // 4, max_bursts=16) as r:
            r.set_xlate(rate_hz=fs, center_hz=fc, decim=4)
            r.push_raw(x[None, :])
            w = r.drain()
        w["channel"] = c
        want.append(w)
    want = np.concatenate(want)
    assert got.tobytes() == want.tobytes()


# ---- 6. errors
def test_argument_errors_and_mutual_exclusion(gpu):
    L = capi.load()
    cen = (capi.C.c_double * 2)(-60e3, 60e3)

    def cfg(decim=2, n=2, rate=400e3, centers=cen, size=None, width=0.0):
        return capi.XlateSharedCfg(capi.C.sizeof(capi.XlateSharedCfg) if size is None else size, decim, n, 0, rate, 0.0, 0.0, width, centers)

    def rc(r, x):
        return L.amps_recc_set_xlate_shared(r._h, capi.C.byref(x) if x is not None else None)

    z = np.zeros(16, np.complex64)
    out = np.zeros((2, 64), np.complex64)
    no = capi.C.c_size_t(0)
    with capi.Recc(n_channels=2, sps=10, max_samples=4096, max_bursts=4) as r:
        # -EINVAL
        assert L.amps_recc_set_xlate_shared(None, capi.C.byref(cfg())) == -errno.EINVAL
        assert rc(r, None) == -errno.EINVAL
        assert rc(r, cfg(size=8)) == -errno.EINVAL
        assert rc(r, cfg(n=3)) == -errno.EINVAL                                   # n_centers != n_channels
        assert rc(r, cfg(centers=None)) == -errno.EINVAL
        assert rc(r, cfg(decim=3, rate=600e3)) == -errno.EINVAL
        assert rc(r, cfg(decim=4)) == -errno.EINVAL                               # 100 ksps != 10 samples per symbol
        assert rc(r, cfg(centers=(capi.C.c_double * 2)(0.0, 400e3 + 1.0))) == -errno.EINVAL   # a centre beyond the rate
        # -E2BIG: 2391 taps
        assert rc(r, cfg(decim=8, rate=1.6e6, width=2.25e3)) == -errno.E2BIG
        # both translate seams answer -ENOSYS on an unconfigured handle
        assert L.amps_recc_push_raw_shared(r._h, capi._hostptr(z), 16, capi.MEM_HOST) == -errno.ENOSYS
        assert L.amps_recc_push_raw(r._h, capi._hostptr(z), 8, 8, capi.MEM_HOST) == -errno.ENOSYS
        assert L.amps_recc_debug_xlate_shared(r._h, capi._hostptr(z), 16, capi.MEM_HOST, capi._hostptr(out), 64, capi.C.byref(no)) == -errno.ENOSYS
        assert L.amps_recc_push_raw_shared(None, capi._hostptr(z), 16, capi.MEM_HOST) == -errno.EINVAL
        # configured: the limit of one push, and the other stage is gone
        assert rc(r, cfg()) == 0
        assert L.amps_recc_push_raw_shared(r._h, capi._hostptr(z), 16, capi.MEM_HOST) == 0
        assert L.amps_recc_push_raw_shared(r._h, None, 16, capi.MEM_HOST) == -errno.EINVAL
        big = np.zeros(2 * 4096 + 2, np.complex64)
        assert L.amps_recc_push_raw_shared(r._h, capi._hostptr(big), big.size, capi.MEM_HOST) == -errno.E2BIG
        assert L.amps_recc_push_raw(r._h, capi._hostptr(z), 8, 8, capi.MEM_HOST) == -errno.ENOSYS
        # the one-row-per-channel stage removes the shared one ...
        r.set_xlate(rate_hz=400e3, center_hz=160e3, decim=2)
        assert L.amps_recc_push_raw_shared(r._h, capi._hostptr(z), 16, capi.MEM_HOST) == -errno.ENOSYS
        assert L.amps_recc_push_raw(r._h, capi._hostptr(z), 8, 8, capi.MEM_HOST) == 0
        # ... and the other way round; decim 0 removes the stage
        assert rc(r, cfg()) == 0
        assert L.amps_recc_push_raw(r._h, capi._hostptr(z), 8, 8, capi.MEM_HOST) == -errno.ENOSYS
        assert L.amps_recc_push_raw_shared(r._h, capi._hostptr(z), 16, capi.MEM_HOST) == 0
        assert rc(r, cfg(decim=0)) == 0
        assert L.amps_recc_push_raw_shared(r._h, capi._hostptr(z), 16, capi.MEM_HOST) == -errno.ENOSYS
    # -ENOSYS: a handle without the IQ seam, and a channel-group handle
    with capi.Recc(n_channels=2, max_bursts=4) as r:
        assert rc(r, cfg()) == -errno.ENOSYS
    wb = {"channels": 1024, "decim": 512, "taps_per_branch": 8, "first_channel": 96, "groups": 2, "group": 0}
    with capi.Recc(n_channels=832, sps=3, max_samples=64 + 72, max_bursts=4, wideband=wb) as r:
        many = (capi.C.c_double * 832)()
        assert rc(r, cfg(decim=1, n=832, rate=60e3, centers=many)) == -errno.ENOSYS


def test_a_dead_communicator_makes_the_seam_stale_until_reset(gpu):
    """-ESTALE as the data seams: after the handle's communicator has died its stream state is void until amps_recc_reset"""
    L = capi.load()
    wb = {"channels": 1024, "decim": 512, "taps_per_branch": 8, "first_channel": 96}
    z = np.zeros(256, np.complex64)
    with capi.Recc(n_channels=832, sps=3, max_samples=1024 + 72, max_bursts=4, wideband=wb) as r:
        r.set_xlate_shared(60e3, [0.0] * 832, 1)
        assert L.amps_recc_push_raw_shared(r._h, capi._hostptr(z), 0, capi.MEM_HOST) == 0
        r.rccl_init(capi.Recc.rccl_unique_id(), 1, 0)
        r.rccl_abort()
        assert L.amps_recc_push_raw_shared(r._h, capi._hostptr(z), z.size, capi.MEM_HOST) == -errno.ESTALE
        assert L.amps_recc_push_raw_shared(r._h, capi._hostptr(z), 0, capi.MEM_HOST) == -errno.ESTALE
        r.reset()
        assert L.amps_recc_push_raw_shared(r._h, capi._hostptr(z), 0, capi.MEM_HOST) == 0
        assert r.debug_xlate_shared(z).shape == (832, 256)      # the stage itself runs again


# ---- 7. host block and recctest
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


def test_recctest_sub_prints_what_the_binding_returns(gpu, tmp_path):
    """gr::amps::recc_subband through `recctest sub`: the five channels of the 400 ksps stream from a file, in ragged work() calls;
    per channel the lines of the bursts the binding returns for the same stream, in order"""
    x, truth = _stream400(4100)
    recs = _push_stream400(x)
    assert len(recs) == 10
    p = tmp_path / "five.raw"
    x.tofile(p)
    _, exe = build_host()
    out = subprocess.run([exe, "sub", str(p), "77777", "400e3", "2", ",".join("%g" % c for c in CENTRES_400)],
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
    # every one of the ten bursts was published under its channel
    assert sum(out.stdout.count("MSG channel %d\n" % c) for c in range(5)) == 10
