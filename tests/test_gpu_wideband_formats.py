"""-m gpu: 8-bit I/Q (sc8, cu8) through the wideband seam (amps_recc_push_wideband_as / amps_recc_debug_channelize_as, include/amps_recc.h).

Each call is DEFINED as the fc32 call on the block converted by capi.convert_samples, and the kernels that read the 8-bit block in place
(chz_narrow_b8_kernel at 512, 256 and 128 branches; a conversion pre-pass in front of the 1024 bank) run the same fp32 operations on
the same values as their fc32 twins: every comparison here is exact -- no tolerance, no excluded row, frame, record or ring slot.
tests/narrowblock.py holds the geometries and the burst block, tests/formatblock.py the quantisers."""
import errno
import os
import subprocess
import sys

import numpy as np
import pytest

from gr_amps_amd import capi, synth_wideband as sw
from conftest import wb_cfg

import formatblock as fb
import narrowblock as nb

pytestmark = pytest.mark.gpu
SC8, CU8 = fb.SC8, fb.CU8
GEO_FMT = pytest.mark.parametrize("M,D,fmt", [(M, D, f) for M, D in nb.GEOMETRIES for f in (SC8, CU8)],
                                  ids=["%s-%s" % (i, fb.FORMAT_IDS[f]) for i in nb.IDS for f in (SC8, CU8)])
REC_CASES = [(M, D, SC8) for M, D in nb.GEOMETRIES] + [(128, 96, CU8), (512, 256, CU8)]
REC_FMT = pytest.mark.parametrize("M,D,fmt", REC_CASES, ids=["M%d-D%d-%s" % (M, D, fb.FORMAT_IDS[f]) for M, D, f in REC_CASES])


def _handle(M, D, C, first, max_frames, max_bursts=64, **kw):
    return capi.Recc(n_channels=C, max_samples=max_frames, max_bursts=max_bursts, wideband={"channels": M, "decim": D, "first_channel": first}, **kw)


def _bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _extremes(q, fmt):
    """plant the format's extreme codes, both components, a few samples apart"""
    lo, hi = (-128, 127) if fmt == SC8 else (0, 255)
    n = q.shape[0]
    for i, pair in ((5, (lo, hi)), (6, (hi, lo)), (n // 2, (lo, lo)), (n // 2 + 1, (hi, hi)), (n - 3, (hi, lo))):
        q[i] = pair
    return q


def _pieces_of(r, block, pieces, fmt=None):
    parts, off = [], 0
    for m in pieces:
        piece = block[off:off + m]
        parts.append(r.debug_channelize(piece) if fmt is None else r.debug_channelize_as(piece, fmt))
        off += m
    assert off == block.shape[0]
    return parts


# ---- 1. the bank's output, bit for bit
@GEO_FMT
def test_bank_output_equals_the_converted_blocks(gpu, M, D, fmt):
    """tones 3 kHz above the centres of bins 0, 1, M / 2 - 1, M / 2 and M - 1 over noise, at a full scale of 100 with the extreme codes
    planted; about 300 frames in ragged pieces -- one shorter than a frame (the carry-only path), one of a single sample, one odd, one
    of 150 frames (several workgroups) -- first as host blocks, then as slices of a device tensor that starts at sample 1 of a larger
    one: 2-byte aligned and not 4-byte aligned, with other values in front of and behind it."""
    import torch
    fs = M * 30e3
    first, C = M - 8, M
    rng = np.random.default_rng(29 + M + D)
    n = 300 * D + 37
    t = np.arange(n)
    x = 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for k, a in ((0, 1.0), (1, 0.8), (M // 2 - 1, 0.6), (M // 2, 0.9), (M - 1, 0.7)):
        x += a * np.exp(2j * np.pi * (sw.bin_freq(k, fs, M) + 3e3) * t / fs)
    q = _extremes(fb.quantise(x, fmt), fmt)
    assert q.min() == (-128 if fmt == SC8 else 0) and q.max() == (127 if fmt == SC8 else 255)
    xf = capi.convert_samples(q, fmt)
    pieces = [D - 5, 1, 3 * D + 11, 150 * D + 11, 2 * D + 1]
    pieces.append(n - sum(pieces))
    assert pieces[2] % 2 == 1 and pieces[-1] > 0
    with _handle(M, D, C, first, 320) as r:
        want = _pieces_of(r, xf, pieces)
    with _handle(M, D, C, first, 320) as r:
        got = _pieces_of(r, q, pieces, fmt)
    assert want[0].shape == (C, 0) and want[3].shape[1] >= 148 and sum(p.shape[1] for p in want) == ((n // D) & (~1 if 2 * D == M else ~3))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(_bits32(g), _bits32(w)), (i, pieces[i])
    assert np.abs(np.concatenate(want, axis=1)).min() > 0                  # every row and frame was written
    # device blocks: the block sits at sample 1 of a larger tensor whose other samples hold other values
    big = np.full((n + 3, 2), 77 if fmt == SC8 else 200, q.dtype)
    big[1:n + 1] = q
    dev = torch.from_numpy(big).to(gpu)[1:n + 1]
    assert dev.data_ptr() % 4 == 2 and dev.is_contiguous()
    with _handle(M, D, C, first, 320) as r:
        got = _pieces_of(r, dev, pieces, fmt)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(_bits32(g), _bits32(w)), ("device", i, pieces[i])


# ---- 2. records
def _halves(n, D):
    return (n // 2) // D * D + 100


def _fc32_records(M, D, xf, tail, **kw):
    n = xf.shape[0]
    with _handle(M, D, M, 0, (n + 64 * D) // D + 72, **kw) as r:
        r.push_wideband(xf[:_halves(n, D)])
        r.push_wideband(xf[_halves(n, D):])
        r.push_wideband(tail)
        return r.drain()


@REC_FMT
def test_records_equal_the_fc32_handle_on_the_converted_block(gpu, M, D, fmt):
    q, xf, truth = fb.burst_block_as(M, D, fmt)
    n = q.shape[0]
    cap = (n + 64 * D) // D + 72
    tail = fb.silence(64 * D, fmt)
    want = _fc32_records(M, D, xf, capi.convert_samples(tail, fmt))
    with _handle(M, D, M, 0, cap) as r:
        r.push_wideband_as(q[:_halves(n, D)], fmt)
        r.push_wideband_as(q[_halves(n, D):], fmt)
        if fmt == CU8:
            r.push_wideband_as(tail, fmt)
        else:
            r.push_wideband(np.zeros(64 * D, np.complex64))                # an fc32 zero block is the same silence
        got = r.drain()
    assert len(want) == 6 and got.tobytes() == want.tobytes()
    by_chan = {int(g["channel"]): g for g in got}
    for (k, off), (kind, min10, esn, dialed, words) in truth.items():
        assert by_chan[k]["min"].decode() == min10 and by_chan[k]["valid"].all(), (k, off)


@REC_FMT
def test_formats_alternate_push_by_push_on_one_handle(gpu, M, D, fmt):
    """fc32, sc16, sc8 and cu8 pushes in turn over five ragged cuts (the case's own format first): every piece is pushed in its format
    and, converted, is a piece of the stream the one-format handle gets as fc32.  (A cu8 piece holds half-odd values, the others whole
    numbers: the stream is made of the pieces as they convert, half a step apart at most.)"""
    x, truth = nb.burst_block(M, D)
    n = x.shape[0]
    cuts = [0, n // 5 + 3, n // 2 + D // 3, 3 * n // 4 + 1, n - D - 1, n]
    order = {SC8: [SC8, capi.SAMPLES_FC32, capi.SAMPLES_SC16, CU8, SC8], CU8: [CU8, capi.SAMPLES_SC16, SC8, capi.SAMPLES_FC32, CU8]}[fmt]
    q8, xf8, _ = fb.burst_block_as(M, D, SC8)
    qu, xfu, _ = fb.burst_block_as(M, D, CU8)
    pieces, conv = [], []
    for f, a, b in zip(order, cuts[:-1], cuts[1:]):
        if f == CU8:
            pieces.append(qu[a:b])
            conv.append(xfu[a:b])
        else:
            conv.append(xf8[a:b])
            pieces.append(q8[a:b] if f == SC8 else q8[a:b].astype(np.int16) if f == capi.SAMPLES_SC16 else xf8[a:b])
    stream = np.concatenate(conv)
    flush = np.zeros(64 * D, np.complex64)
    want = _fc32_records(M, D, stream, flush)
    with _handle(M, D, M, 0, (n + 64 * D) // D + 72) as r:
        for i, (f, p) in enumerate(zip(order, pieces)):
            if i == 1 and f == capi.SAMPLES_FC32:
                r.push_wideband(p)                                         # the existing entry points take their turn too
            elif f == capi.SAMPLES_SC16 and i == 2:
                r.push_wideband_short(p)
            else:
                r.push_wideband_as(p, f)
        r.push_wideband_as(flush, capi.SAMPLES_FC32)
        got = r.drain()
    assert len(want) == 6 and got.tobytes() == want.tobytes()
    assert sorted(g["min"].decode() for g in got) == sorted(v[1] for v in truth.values())


# ---- 3. rings
def test_power_and_offset_rings_equal_the_fc32_handles(gpu):
    M, D = 256, 128
    q, xf, truth = fb.burst_block_as(M, D, SC8)
    n = q.shape[0]
    cap = (n + 64 * D) // D + 72
    kw = dict(stream_power=True, stream_offset="unit")
    outs = []
    for data, push in ((xf, lambda r, a: r.push_wideband(a)), (q, lambda r, a: r.push_wideband_as(a, SC8))):
        with _handle(M, D, M, 0, cap, **kw) as r:
            push(r, data[:_halves(n, D)])
            push(r, data[_halves(n, D):])
            push(r, np.zeros(64 * D, np.complex64) if data is xf else fb.silence(64 * D, SC8))
            recs = r.drain()
            outs.append((recs, r.channel_power(), r.channel_autocorr(), r.burst_power(recs), r.burst_offset(recs)))
    (wr, wp, wa, wbp, wbo), (gr, gp, ga, gbp, gbo) = outs
    assert len(wr) == 6 and gr.tobytes() == wr.tobytes()
    assert gp[1] == wp[1] and gp[0].shape == wp[0].shape and wp[0].shape[1] > 20 and np.array_equal(_bits32(gp[0]), _bits32(wp[0]))
    assert ga[1] == wa[1] and ga[0].shape == wa[0].shape and np.array_equal(_bits32(ga[0]), _bits32(wa[0]))
    assert np.array_equal(_bits32(gbp[0]), _bits32(wbp[0])) and np.array_equal(gbp[1], wbp[1]) and wbp[1].min() > 0
    assert np.array_equal(_bits32(gbo[0]), _bits32(wbo[0])) and np.array_equal(gbo[1], wbo[1])
    assert wp[0].max() > 1.0                                               # received power in int8 units squared, not in units of full scale


# ---- 4. the 1024 bank: a conversion pre-pass, then everything as for an fc32 block
@pytest.mark.parametrize("fmt", [SC8, CU8], ids=["sc8", "cu8"])
def test_1024_bank_output_equals_the_converted_blocks(gpu, decim, fmt):
    D, first, C = decim, 1000, 96                                          # the band wraps past bin 1023
    n = 64 * D * 3 + 11
    rng = np.random.default_rng(5 + D)
    t = np.arange(n)
    x = 0.1 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) + np.exp(2j * np.pi * (sw.bin_freq(3, sw.FS_WIDE) + 3e3) * t / sw.FS_WIDE)
    q = _extremes(fb.quantise(x, fmt), fmt)
    xf = capi.convert_samples(q, fmt)
    wb, sps = wb_cfg(D, first)
    pieces = [D - 7, 1, 70 * D + 5, n - 71 * D + 1]
    outs = []
    for block, f in ((xf, None), (q, fmt)):
        with capi.Recc(n_channels=C, sps=sps, max_samples=256, max_bursts=16, wideband=wb) as r:
            outs.append(np.concatenate(_pieces_of(r, block, pieces, f), axis=1))
    assert outs[0].shape == (C, (n // D) & ~1 if D == 512 else (n // D) & ~3) and np.abs(outs[0]).min() > 0
    assert np.array_equal(_bits32(outs[0]), _bits32(outs[1]))


def test_1024_fused_records_equal_the_fc32_handles(gpu):
    """one planted burst through the fused form at the default decimation, the stream of tests/test_gpu_short_input.py (832 channels from
    bin 700, sw.make_wideband) cut to the one burst and its flush: the sc8 records are the fc32 ones on the converted block"""
    D = int(capi.load().amps_recc_default_wideband_decim())
    first, C = 700, 832
    n = int(0.18 * sw.FS_WIDE) // D * D
    x, truth = sw.make_wideband(n, [((first + 100) % 1024, 30000)], seed=77)
    q = fb.quantise(x, SC8)
    xf = capi.convert_samples(q, SC8)
    wb, sps = wb_cfg(D, first)
    cut = n // 3 + 5
    outs = []
    for data, push in ((xf, lambda r, a: r.push_wideband(a)), (q, lambda r, a: r.push_wideband_as(a, SC8))):
        with capi.Recc(n_channels=C, sps=sps, max_samples=n // D + 64 + 72, max_bursts=16, wideband=wb) as r:
            push(r, data[:cut])
            push(r, data[cut:])
            push(r, np.zeros(64 * D, np.complex64) if data is xf else fb.silence(64 * D, SC8))
            outs.append(r.drain())
    assert len(outs[0]) == 1 and outs[0]["min"][0].decode() == list(truth.values())[0][1] and int(outs[0]["channel"][0]) == 100
    assert outs[1].tobytes() == outs[0].tobytes()


# ---- 5. refusals
def test_refusals(gpu):
    L = capi.load()
    M, D = 128, 96
    q, xf, truth = fb.burst_block_as(M, D, SC8)
    n = q.shape[0]
    cap = (n + 64 * D) // D + 72
    # no wideband seam on this handle
    with capi.Recc(n_channels=1, sps=10, max_samples=4096, max_bursts=16) as r:
        with pytest.raises(capi.AmpsError) as e:
            r.push_wideband_as(q[:64], SC8)
        assert e.value.code == -errno.ENOSYS
        with pytest.raises(capi.AmpsError) as e:
            r.debug_channelize_as(q[:64], SC8)
        assert e.value.code == -errno.ENOSYS
    with _handle(M, D, M, 0, cap) as r:
        for bad in (4, 7, -1):                                             # an unknown format
            with pytest.raises(capi.AmpsError) as e:
                r.push_wideband_as(q[:64], bad)
            assert e.value.code == -errno.EINVAL
            with pytest.raises(capi.AmpsError) as e:
                r.debug_channelize_as(q[:64], bad)
            assert e.value.code == -errno.EINVAL
        assert L.amps_recc_push_wideband_as(r._h, None, 16, SC8, capi.MEM_HOST) == -errno.EINVAL
        assert L.amps_recc_push_wideband_as(r._h, None, 0, SC8, capi.MEM_HOST) == 0
        r.push_wideband_as(np.zeros((0, 2), np.uint8), CU8)
        # -E2BIG consumes nothing: the stream goes on as if the refused block had never been offered
        r.push_wideband_as(q[:_halves(n, D)], SC8)
        with pytest.raises(capi.AmpsError) as e:
            r.push_wideband_as(np.full(((cap + 8) * D, 2), 50, np.int8), SC8)
        assert e.value.code == -errno.E2BIG
        r.push_wideband_as(q[_halves(n, D):], SC8)
        r.push_wideband_as(fb.silence(64 * D, SC8), SC8)
        got = r.drain()
    want = _fc32_records(M, D, xf, np.zeros(64 * D, np.complex64))
    assert len(want) == 6 and got.tobytes() == want.tobytes()


# ---- 6. host block and example
@pytest.mark.parametrize("fmt", [SC8, CU8], ids=["sc8", "cu8"])
def test_recctest_wide_reads_an_8_bit_file(gpu, tmp_path, fmt):
    """gr::amps::recc_wideband::make(128, 0, ..., channels = 128, input_format) through recctest: a 3.84 Msps capture file of 8-bit pairs
    in, the lines of the six bursts out, as the C ABI's own records give them"""
    from gr_amps_amd.host import build_host
    from test_gpu_host_blocks import _expected_lines
    M, D = 128, 96                                               # the default decimation
    q, xf, truth = fb.burst_block_as(M, D, fmt)
    p = tmp_path / ("block." + fb.FORMAT_IDS[fmt])
    q.tofile(p)
    assert os.path.getsize(p) == 2 * q.shape[0]
    tail = fb.silence(64 * 768, fmt)                             # recctest's own tail of silence
    with capi.Recc(n_channels=M, max_samples=(q.shape[0] + 64 * 768) // D + 72, max_bursts=64, wideband={"channels": M}) as r:
        assert r.decim == D and r.sps == 2
        r.push_wideband(xf)
        r.push_wideband(capi.convert_samples(tail, fmt))
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


def test_example_decodes_a_3_84_msps_sc8_stream(gpu):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "decode_wideband.py"), "--channels", "128", "--sc8"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "MISMATCH" not in out.stdout and " decoded" in out.stdout
