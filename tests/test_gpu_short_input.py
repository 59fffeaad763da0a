"""-m gpu: 16-bit I/Q through the wideband seam (amps_recc_push_wideband_short, include/amps_recc.h).

The call is DEFINED as amps_recc_push_wideband on the plainly converted block, and the fused filter bank that reads the 16-bit block
in place (chz12_short_kernel) runs the same fp32 operations on the same values as its fc32 twin: every comparison here is exact --
no tolerance, no excluded channel, frame or record.

The stream is the one of tests/test_gpu_wideband_bits.py (832 channels from bin 700, wrapping; six bursts), quantised as
q = rint(x * s) with s the largest power of two that keeps every component below 30 000 in magnitude; xf = q as complex64 is the fc32
twin.  Every test runs at both decimations and, where it has the parameter, for all four slicer specs."""
import errno
import os
import subprocess

import numpy as np
import pytest

import oracle
from gr_amps_amd import capi, synth_wideband as sw
from conftest import wb_cfg

pytestmark = pytest.mark.gpu

FIRST, C, M = 700, 832, 1024
NFR = 4500
SPECS = [("atan", 0), ("product", 1), ("sine", 2), ("exact", 3)]
BURST_ROWS = (0, C - 1, (1023 - FIRST) % M, (0 - FIRST) % M, 100, 600)
BURST_FRAMES = (80, 600, 1200, 2000, 2800, 3500)
RAGGED = lambda D: [10 * D + 100, 55 * D - 93, 96 * D, 94 * D + 500, D - 504, 64 * D, 4100 * D, None]   # test_gpu_wideband_bits.py
LIMIT = 30000

_cache = {}


def quantise(x):
    """(q int16 [n, 2], xf complex64, s): q = rint(x * s), s the largest power of two with every |component| * s < LIMIT"""
    peak = max(np.abs(x.real).max(), np.abs(x.imag).max())
    s = 2.0 ** np.floor(np.log2(LIMIT / peak))
    if peak * s >= LIMIT:
        s /= 2
    assert peak * s < LIMIT <= peak * 2 * s
    v = np.rint(np.stack([x.real, x.imag], axis=1).astype(np.float64) * s)
    assert np.abs(v).max() < LIMIT                                     # nothing clipped
    q = v.astype(np.int16)
    assert np.array_equal(q.astype(np.float64), v)
    xf = (q[:, 0].astype(np.float32) + 1j * q[:, 1].astype(np.float32)).astype(np.complex64)
    return q, xf, s


def _handle(D, max_frames=NFR + 72, **kw):
    wb, sps = wb_cfg(D, FIRST, groups=kw.pop("groups", 0), group=kw.pop("group", 0))
    return capi.Recc(n_channels=C, sps=sps, max_samples=max_frames, max_bursts=64, wideband=wb, **kw)


def _block(D):
    if ("block", D) not in _cache:
        n = NFR * D + 333
        bursts = [((FIRST + r) % M, f * D + 17 * i) for i, (r, f) in enumerate(zip(BURST_ROWS, BURST_FRAMES))]
        x, truth = sw.make_wideband(n, bursts, seed=77)
        q, xf, s = quantise(x)
        print(f"\nD={D}: quantised with s = {s:g}, peak component {np.abs(q).max()}")
        _cache[("block", D)] = (q, xf)
    return _cache[("block", D)]


def _bits(r, first=0):
    n = r.debug_slicer_bits(0, 0)[1] - first
    return r.debug_slicer_bits(first, n)


def _twin(D, spec):
    """slicer bits of push_wideband(xf), one shot"""
    if ("twin", D, spec) not in _cache:
        xf = _block(D)[1]
        with _handle(D, slicer=spec) as r:
            r.push_wideband(xf)
            _cache[("twin", D, spec)] = _bits(r)
    return _cache[("twin", D, spec)]


def _mism(a, b, k=8):
    assert a.shape == b.shape, (a.shape, b.shape)
    r, f = np.nonzero(a != b)
    return r.size, list(zip(r[:k].tolist(), f[:k].tolist()))


def _ragged(D, spec, kind):
    """the RAGGED schedule pushed as sc16 (kind 's'), fc32 ('f') or alternating, push by push, starting with sc16 ('sf') / fc32 ('fs')"""
    q, xf = _block(D)
    off, k = 0, 0
    with _handle(D, slicer=spec) as r:
        for m in RAGGED(D):
            m = len(q) - off if m is None else m
            if kind[k % len(kind)] == "s":
                r.push_wideband_short(q[off:off + m])
            else:
                r.push_wideband(xf[off:off + m])
            off += m
            k += 1
            assert r.debug_slicer_bits(0, 0)[1] == (off // D) & ~63
        assert off == len(q)
        return _bits(r)


@pytest.mark.parametrize("spec,sid", SPECS)
def test_short_bits_equal_the_fc32_twin_one_shot(gpu, decim, spec, sid):
    D = decim
    q, xf = _block(D)
    want, produced = _twin(D, spec)
    assert produced == (len(q) // D) & ~63 and produced // 64 >= 65 and want.shape == (C, produced)
    with _handle(D, slicer=spec) as r:
        r.push_wideband_short(q)
        got, p = _bits(r)
    assert p == produced
    count, where = _mism(got, want)
    assert count == 0, (count, where)


@pytest.mark.parametrize("spec,sid", SPECS)
def test_short_bits_ragged_pushes(gpu, decim, spec, sid):
    D = decim
    want, produced = _twin(D, spec)
    got, p = _ragged(D, spec, "s")
    assert p == produced
    count, where = _mism(got, want)
    assert count == 0, (count, where)


def test_extreme_components_ragged_pushes(gpu, decim):
    """quantise() keeps every component below 30 000, so the 16-bit reader's sign-extending conversion never meets the ends of its
    range there: here a random 1 % of the block's components are -32768, -32767, -1, 0, 1 or 32767, pushed as sc16 in the RAGGED
    schedule; the bits are exactly those of the fc32 twin of the same values"""
    D = decim
    q = _block(D)[0].copy()
    rng = np.random.default_rng(16)
    flat = q.reshape(-1)
    idx = np.nonzero(rng.random(flat.size) < 0.01)[0]
    flat[idx] = rng.choice(np.array([-32768, -32767, -1, 0, 1, 32767], np.int16), idx.size)
    assert flat.min() == -32768 and flat.max() == 32767 and abs(idx.size / flat.size - 0.01) < 1e-3
    assert all((flat[idx] == v).sum() > 1000 for v in (-32768, -32767, -1, 0, 1, 32767))
    xf = (q[:, 0].astype(np.float32) + 1j * q[:, 1].astype(np.float32)).astype(np.complex64)
    with _handle(D) as r:
        r.push_wideband(xf)
        want, produced = _bits(r)
    assert produced == (len(q) // D) & ~63
    off = 0
    with _handle(D) as r:
        for m in RAGGED(D):
            m = len(q) - off if m is None else m
            r.push_wideband_short(q[off:off + m])
            off += m
        assert off == len(q)
        got, p = _bits(r)
    assert p == produced
    count, where = _mism(got, want)
    assert count == 0, (count, where)


@pytest.mark.parametrize("order", ["sf", "fs"])
@pytest.mark.parametrize("spec,sid", SPECS)
def test_short_and_fc32_pushes_alternate_on_one_handle(gpu, decim, spec, sid, order):
    D = decim
    want, produced = _twin(D, spec)
    got, p = _ragged(D, spec, order)
    assert p == produced
    count, where = _mism(got, want)
    assert count == 0, (order, count, where)


@pytest.mark.parametrize("spec,sid", SPECS)
def test_device_blocks_and_an_odd_slice_give_the_host_blocks_bits(gpu, decim, spec, sid):
    import torch
    D = decim
    q, xf = _block(D)
    want, produced = _twin(D, spec)
    t = torch.from_numpy(q).to(gpu)                                   # [n, 2]
    with _handle(D, slicer=spec) as r:
        r.push_wideband_short(t)
        got, p = _bits(r)
    assert p == produced
    count, where = _mism(got, want)
    assert count == 0, (count, where)
    # a device slice that starts at sample 1 (4-byte aligned, not 8): the stream's first sample goes in on its own, from the host;
    # flat [2n] shape this time
    pad = torch.from_numpy(np.concatenate([np.zeros((1, 2), np.int16), q])).to(gpu)
    sl = pad.reshape(-1)[2:]
    assert sl.data_ptr() % 8 == 4
    with _handle(D, slicer=spec) as r:
        r.push_wideband_short(sl)
        got, p = _bits(r)
    assert p == produced
    count, where = _mism(got, want)
    assert count == 0, (count, where)
    # ... and one that starts at sample 1 of the stream itself, behind a one-sample host push
    dq = torch.from_numpy(q).to(gpu)
    with _handle(D, slicer=spec) as r:
        r.push_wideband_short(q[:1])
        r.push_wideband_short(dq[1:])
        got, p = _bits(r)
    assert p == produced
    count, where = _mism(got, want)
    assert count == 0, (count, where)


@pytest.mark.parametrize("G", [2, 4, 8])
@pytest.mark.parametrize("spec,sid", SPECS)
def test_channel_group_handles_give_the_whole_band_rows(gpu, decim, spec, sid, G):
    D = decim
    q, xf = _block(D)
    whole, produced = _twin(D, spec)
    seen = np.zeros(C, int)
    for g in range(G):
        rows = [c for c in range(C) if (((FIRST + c) % M) & 63) // (64 // G) == g]
        with _handle(D, slicer=spec, groups=G, group=g) as r:
            r.push_wideband_short(q)
            bits, p = _bits(r)
        assert p == produced and bits.shape == (len(rows), produced), (g, bits.shape)
        count, where = _mism(bits, whole[rows])
        assert count == 0, (g, count, where)
        seen[rows] += 1
    assert (seen == 1).all()


@pytest.mark.parametrize("spec,sid", SPECS)
def test_unfused_handle_gives_the_fused_bits(gpu, decim, spec, sid):
    D = decim
    q, xf = _block(D)
    one, produced_one = _twin(D, spec)
    off, prev = 0, 0
    with _handle(D, slicer=spec, unfused_wideband=True) as r:
        for m in RAGGED(D):
            m = len(q) - off if m is None else m
            r.push_wideband_short(q[off:off + m])
            off += m
            produced = r.debug_slicer_bits(0, 0)[1]
            assert produced == (off // D) & ~63, (off, produced)
            if produced > prev:
                hi = min(produced, produced_one)
                bits, _ = r.debug_slicer_bits(prev, hi - prev)
                count, where = _mism(bits, one[:, prev:hi])
                assert count == 0, (off, count, where)
                prev = hi
    assert prev == produced_one


def test_short_bits_equal_the_cpu_model_on_the_iq_forms_output(gpu, decim):
    """an anchor that does not pass through the fc32 filter-bank kernel's slicer: spec `exact`, the bits of the sc16 push against
    oracle.Fused run on debug_channelize(xf), row by row"""
    D = decim
    q, xf = _block(D)
    with _handle(D) as r:
        chan = r.debug_channelize(xf)
    with _handle(D, slicer="exact") as r:
        r.push_wideband_short(q)
        bits, produced = _bits(r)
    assert bits.shape == (C, produced) and produced == (len(q) // D) & ~63
    model = []
    for row in range(C):
        f = oracle.Fused(row, 1536 // D, slicer=3)
        f.push(chan[row])
        model.append(f.taps()[2])
    model = np.stack(model)
    assert model.shape[1] >= produced
    count, where = _mism(bits, model[:, :produced])
    assert count == 0, (count, where)
    assert bits[:, :1536 // D].all()


def test_records_of_the_example_stream_are_byte_equal(gpu, decim):
    """examples/decode_wideband.py's stream (twelve mobiles, 20 dB, 50 ppm) in its ragged blocks: drain() of the sc16 form is byte-equal
    to the fc32 twin's, and the twin finds the true MIN of as many mobiles as the unquantised stream does"""
    D = decim
    first_bin, channels, nsamp = 96, 832, 12 * (1 << 20)
    rng = np.random.default_rng(7)
    plan = [(first_bin + int(c), int(rng.integers(4000, nsamp - 3456 * 1536 - 4000))) for c in rng.choice(channels, 12, replace=False)]
    x, truth = sw.make_wideband(nsamp, plan, seed=7, snr_db=20.0, sym_ppm=50.0)
    q, xf, s = quantise(x)
    print(f"\nexample stream: s = {s:g}")
    cuts, pos = [], 0
    while pos < nsamp:
        n = min(int(rng.integers(100_000, 3_000_000)), nsamp - pos)
        cuts.append((pos, n))
        pos += n
    sent = {k - first_bin: v[1] for (k, _), v in truth.items()}

    def run(push, data, flush):
        wb, sps = wb_cfg(D, first_bin)
        with capi.Recc(n_channels=channels, sps=sps, max_samples=nsamp // 512 + 72, max_bursts=256, wideband=wb) as r:
            for pos, n in cuts:
                getattr(r, push)(data[pos:pos + n])
            getattr(r, push)(flush)
            return r.drain()

    rs = run("push_wideband_short", q, np.zeros((64 * D, 2), np.int16))
    rf = run("push_wideband", xf, np.zeros(64 * D, np.complex64))
    ru = run("push_wideband", x, np.zeros(64 * D, np.complex64))
    assert len(rs) == len(rf) and rs.tobytes() == rf.tobytes()
    right = lambda recs: sum(1 for r in recs if sent.get(int(r["channel"])) == r["min"].decode())
    assert right(rf) == right(ru) and len(rf) == len(ru), (right(rf), right(ru), len(rf), len(ru))
    if D == int(capi.load().amps_recc_default_wideband_decim()):
        assert right(ru) == 12                                         # the example's own exit status at the default decimation


def test_error_codes(gpu, decim):
    D = decim
    L = capi.load()
    buf = np.zeros((8, 2), np.int16)
    # no wideband seam on this handle
    with capi.Recc(n_channels=1, sps=10, max_samples=4096, max_bursts=16) as r:
        with pytest.raises(capi.AmpsError) as e:
            r.push_wideband_short(buf)
        assert e.value.code == -errno.ENOSYS
    with _handle(D, max_frames=128) as r:
        assert L.amps_recc_push_wideband_short(r._h, None, 16, capi.MEM_HOST) == -errno.EINVAL
        assert L.amps_recc_push_wideband_short(r._h, None, 0, capi.MEM_HOST) == 0
        r.push_wideband_short(np.zeros((0, 2), np.int16))
        assert r.debug_slicer_bits(0, 0)[1] == 0
        for bad in (np.zeros(16, np.float32), np.zeros(8, np.complex64), np.zeros((8, 2), np.int32), np.zeros((8, 3), np.int16), [1, 2]):
            with pytest.raises(TypeError):
                r.push_wideband_short(bad)
        # -E2BIG at the block size at which the fc32 call answers it, not one frame earlier
        ok, big = 128 * D + D - 1, 192 * D
        r.push_wideband_short(np.zeros((ok, 2), np.int16))
    for push, zeros in (("push_wideband_short", lambda n: np.zeros((n, 2), np.int16)), ("push_wideband", lambda n: np.zeros(n, np.complex64))):
        with _handle(D, max_frames=128) as r:
            getattr(r, push)(zeros(ok))
        with _handle(D, max_frames=128) as r:
            with pytest.raises(capi.AmpsError) as e:
                getattr(r, push)(zeros(big))
            assert e.value.code == -errno.E2BIG, push


def test_recctest_wide_reads_a_short_file(gpu, tmp_path):
    """gr::amps::recc_wideband with 16-bit items: `recctest wide` on an interleaved int16 capture (.sc16) prints what it prints on the
    fc32 twin of the same samples"""
    from gr_amps_amd.host import build_host
    n = int(0.26 * sw.FS_WIDE) // 512 * 512
    planted = [(96 + 7, 150000), (96 + 500, 90000), (96 + 831, 230000)]
    x, truth = sw.make_wideband(n, planted, seed=41)
    q, xf, s = quantise(x)
    ps, pf = tmp_path / "band.sc16", tmp_path / "band.fc32"
    q.tofile(ps)
    xf.tofile(pf)
    assert os.path.getsize(ps) * 2 == os.path.getsize(pf)
    _, exe = build_host()
    outs = []
    for p in (ps, pf):
        out = subprocess.run([exe, "wide", str(p), "777777"], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        outs.append([l for l in out.stdout.splitlines() if l.startswith("MSG ")])
    assert outs[0] == outs[1]
    assert sorted(int(l.split()[2]) for l in outs[0] if l.startswith("MSG channel")) == [7, 500, 831]
