"""-m gpu: the translate seams on an SDR's integer samples, read in place (amps_recc_push_raw_shared_as / _push_raw_as /
_debug_xlate_shared_as / _debug_xlate_as with AMPS_RECC_SAMPLES_SC16 / _SC8 / _CU8).

The definition (include/amps_recc.h) is an identity: each call is the fc32 call on the block converted by the plain conversion
(capi.convert_samples), which is exact in binary32.  So every comparison of stage output here is equality of the bits
(np.array_equal on .view(np.uint32)) and every comparison of records equality of the bytes: there is no tolerance in this file.
Inputs are random integers over the format's FULL range with the extreme values planted."""
import errno
import functools
import subprocess

import numpy as np
import pytest

from gr_amps_amd import capi
from gr_amps_amd.host import build_host
from test_cpu_xlate_formats import CENTRES_400, quantised400, stream400

pytestmark = pytest.mark.gpu

FORMATS = {"sc16": capi.SAMPLES_SC16, "sc8": capi.SAMPLES_SC8, "cu8": capi.SAMPLES_CU8}
# (rate, decimation, centres): the default filter has 299 taps at 400 ksps and 1195 at 1.6 Msps; one centre of the first is a duplicate
CONFIGS = {"400k_d2": (400e3, 2, (-160e3, 37.5e3, 0.0, 37.5e3)), "1600k_d8": (1.6e6, 8, (-615e3, 15e3))}
BLOCK_LISTS = {"a": [1, 2, 3, 298, 299, 300, 4097], "b": [2047, 2049, 1, 1, 1]}


@functools.lru_cache(maxsize=None)
def _ints(fmt, n, seed=31, rows=None):
    """[n, 2] (or [rows, n, 2]) random samples over the whole range of the format, both extremes planted in I and in Q"""
    info = np.iinfo(capi.SAMPLE_DTYPES[fmt])
    rng = np.random.default_rng(seed + fmt)
    a = rng.integers(info.min, info.max + 1, size=((n, 2) if rows is None else (rows, n, 2))).astype(capi.SAMPLE_DTYPES[fmt])
    flat = a.reshape(-1, 2)
    for i, pair in zip((0, 1, 2, 3, 300, 2047, 2048, flat.shape[0] - 1),
                       ((info.min, info.max), (info.max, info.min), (info.min, info.min), (info.max, info.max)) * 2):
        flat[i % flat.shape[0]] = pair
    a.setflags(write=False)
    return a


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _shared(cfg, max_samples):
    fs, D, centres = CONFIGS[cfg]
    r = capi.Recc(n_channels=len(centres), sps=10, max_samples=max_samples, max_bursts=4)
    r.set_xlate_shared(fs, list(centres), D)
    return r


@functools.lru_cache(maxsize=None)
def _fc32_rows(cfg, fmt, n, skip=0):
    """the reference of this file, computed once per case: the fc32 call on the converted block, on a fresh handle"""
    x = capi.convert_samples(_ints(fmt, n), fmt)[skip:]
    with _shared(cfg, n) as r:
        y = r.debug_xlate_shared(x)
    y.setflags(write=False)
    return y


# ---- 1. rows equal the fc32 path
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("name", list(FORMATS))
def test_rows_equal_the_fc32_path(gpu, name, cfg):
    """three input tiles, the last one partial: the first tile's history comes from the carry, the later ones' from the block.  As a
    host array, as a device tensor, and as a device tensor that starts at an odd sample (aligned to one sample only)."""
    import torch
    fmt, n = FORMATS[name], 2 * 2048 + 301
    D = CONFIGS[cfg][1]
    x = _ints(fmt, n)
    want = _fc32_rows(cfg, fmt, n)
    assert want.shape == (len(CONFIGS[cfg][2]), n // D) and np.abs(want).max() > 0
    with _shared(cfg, n) as r:
        host = r.debug_xlate_shared_as(x, fmt)
        r.reset()
        flat = r.debug_xlate_shared_as(x.reshape(-1), fmt)                      # the [2n] shape
    t = torch.from_numpy(np.array(x)).to(gpu)
    with _shared(cfg, n) as r:
        dev = r.debug_xlate_shared_as(t, fmt)
    with _shared(cfg, n) as r:
        odd = r.debug_xlate_shared_as(t[1:], fmt)
    assert t[1:].data_ptr() - t.data_ptr() == 2 * x.dtype.itemsize
    assert _bits_equal(host, want), "host block"
    assert _bits_equal(flat, want), "host block, flat"
    assert _bits_equal(dev, want), "device block"
    assert _bits_equal(odd, _fc32_rows(cfg, fmt, n, 1)), "device block from an odd sample"


# ---- 2. streaming and mixing
@pytest.mark.parametrize("blocks", list(BLOCK_LISTS))
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("name", list(FORMATS))
def test_streaming_and_mixing_formats_is_bitwise(gpu, name, cfg, blocks):
    """ragged pushes alternating between the integer format and fc32 of the converted slice, the same all-integer, one whole integer
    push, and the same after reset: each equals ONE fc32 push of the converted whole (the stage's carry is fc32)"""
    fmt, blocks = FORMATS[name], BLOCK_LISTS[blocks]
    n = sum(blocks)
    x = _ints(fmt, n, seed=47)
    xf = capi.convert_samples(x, fmt)
    with _shared(cfg, n) as r:
        want = r.debug_xlate_shared(xf)
        got = {}
        for what in ("alternating", "all integer", "alternating, fc32 first"):
            r.reset()
            parts, o = [], 0
            for i, b in enumerate(blocks):
                as_int = what == "all integer" or (i % 2 == (0 if what == "alternating" else 1))
                parts.append(r.debug_xlate_shared_as(x[o:o + b], fmt) if as_int else r.debug_xlate_shared(xf[o:o + b]))
                o += b
            got[what] = np.concatenate(parts, axis=1)
        r.reset()
        got["one integer push"] = r.debug_xlate_shared_as(x, fmt)
        r.reset()
        got["after reset"] = r.debug_xlate_shared_as(x, fmt)
    assert want.shape == (len(CONFIGS[cfg][2]), n // CONFIGS[cfg][1])
    for what, y in got.items():
        assert _bits_equal(y, want), what


def test_formats_mix_with_each_other_on_one_handle(gpu):
    """every block of a ragged list in another format -- sc16, cu8, fc32, sc8, ... -- each over its own full range: the rows of ONE
    fc32 push of the concatenation of the converted blocks"""
    blocks = BLOCK_LISTS["a"]
    order = [capi.SAMPLES_SC16, capi.SAMPLES_CU8, capi.SAMPLES_FC32, capi.SAMPLES_SC8, capi.SAMPLES_CU8, capi.SAMPLES_SC16, capi.SAMPLES_SC8]
    rng = np.random.default_rng(59)
    raw = [(rng.standard_normal((b, 2)) * 1000).astype(np.float32) if f == capi.SAMPLES_FC32 else _ints(f, b, seed=59 + i)
           for i, (f, b) in enumerate(zip(order, blocks))]
    whole = np.concatenate([capi.convert_samples(a, f) for a, f in zip(raw, order)])
    with _shared("400k_d2", whole.size) as r:
        want = r.debug_xlate_shared(whole)
        r.reset()
        parts = [r.debug_xlate_shared_as(a, f) for a, f in zip(raw, order)]
    assert _bits_equal(np.concatenate(parts, axis=1), want)


# ---- 3. per-row form
@pytest.mark.parametrize("name", ["sc16", "cu8"])
def test_per_row_form_equals_the_fc32_path(gpu, name):
    """C = 3 rows with a pitch ld > nsamp, decimation 2: one whole push (host and device) and a ragged list"""
    import torch
    fmt, C, blocks = FORMATS[name], 3, BLOCK_LISTS["a"]
    n = sum(blocks)
    ld = n + 37
    x = _ints(fmt, ld, seed=83, rows=C)                                         # [C, ld, 2]; the last 37 samples of a row are not pushed
    xf = capi.convert_samples(x, fmt)[:, :n]

    def handle():
        r = capi.Recc(n_channels=C, sps=10, max_samples=n, max_bursts=4)
        r.set_xlate(rate_hz=400e3, center_hz=-70e3, decim=2)
        return r

    with handle() as r:
        want = r.debug_xlate(np.ascontiguousarray(xf))
    with handle() as r:
        whole = r.debug_xlate_as(x, fmt, nsamp=n)
        r.reset()
        flat = r.debug_xlate_as(x.reshape(C, 2 * ld), fmt, nsamp=n)             # the [C, 2n] shape
        r.reset()
        dev = r.debug_xlate_as(torch.from_numpy(np.array(x)).to(gpu), fmt, nsamp=n)
        r.reset()
        parts, o = [], 0
        for b in blocks:
            parts.append(r.debug_xlate_as(x[:, o:], fmt, nsamp=b))              # pitch ld - o > b
            o += b
        ragged = np.concatenate(parts, axis=1)
    assert want.shape == (C, n // 2) and np.abs(want).max() > 0
    for what, y in (("whole", whole), ("flat", flat), ("device", dev), ("ragged", ragged)):
        assert _bits_equal(y, want), what


# ---- 4. records end to end
def _cuts(n):
    return [0, 70001, 150002, 150003, 333334, n]


@functools.lru_cache(maxsize=None)
def _records400(fmt):
    """(records of the integer pushes, records of the fc32 twin): the five-channel stream of tests/test_cpu_xlate_formats.py in
    ragged blocks on two handles"""
    q = quantised400(fmt)
    y = capi.convert_samples(q, fmt)
    cuts = _cuts(q.shape[0])
    out = []
    for as_int in (True, False):
        with capi.Recc(n_channels=len(CENTRES_400), sps=10, max_samples=q.shape[0] // 2, max_bursts=64) as r:
            r.set_xlate_shared(400e3, CENTRES_400, 2)
            for a, b in zip(cuts[:-1], cuts[1:]):
                if as_int:
                    r.push_raw_shared_as(q[a:b], fmt)
                else:
                    r.push_raw_shared(y[a:b])
            out.append(r.drain())
    return tuple(out)


@pytest.mark.parametrize("name", list(FORMATS))
def test_records_equal_the_fc32_twin_byte_for_byte(gpu, name):
    """Five channels of one 400 ksps stream, two bursts each, two channels adjacent with bursts overlapping in time, quantised at a
    fixed scale -- 4096 per unit amplitude for sc16, 16 for sc8 and cu8; the peak per component is 5.03, so nothing clips -- and
    pushed in ragged blocks through push_raw_shared_as; convert_samples of the same integers goes through push_raw_shared on a twin.
    The drained record arrays are equal byte for byte.  Condition, not a measurement: every planted burst is among the records.
    That the fc32 path decodes all ten from the QUANTISED samples at these scales and this seed was checked beforehand on the CPU
    with oracle.chain_iq400 per centre; tests/test_cpu_xlate_formats.py::test_the_quantised_stream_still_decodes_on_the_cpu keeps
    checking it."""
    fmt = FORMATS[name]
    _, truth = stream400()
    got, twin = _records400(fmt)
    assert got.tobytes() == twin.tobytes()
    sent = sorted((c, b[2]) for c, t in enumerate(truth) for b in t)
    assert len(sent) == 10
    assert sorted((int(g["channel"]), g["min"].decode()) for g in got) == sent


# ---- 5. errors and types
def test_errors_and_types(gpu):
    L = capi.load()
    z = np.zeros((64, 2), np.int16)
    out = np.zeros((2, 128), np.complex64)
    no = capi.C.c_size_t(0)
    hp = capi._hostptr

    def push_s(r, fmt, n=16, p=z):
        return L.amps_recc_push_raw_shared_as(r._h, hp(p) if p is not None else None, n, fmt, capi.MEM_HOST)

    def push_r(r, fmt, n=8, p=z):
        return L.amps_recc_push_raw_as(r._h, hp(p) if p is not None else None, n, n, fmt, capi.MEM_HOST)

    def dbg_s(r, fmt, n=16):
        return L.amps_recc_debug_xlate_shared_as(r._h, hp(z), n, fmt, capi.MEM_HOST, hp(out), 128, capi.C.byref(no))

    def dbg_r(r, fmt, n=8):
        return L.amps_recc_debug_xlate_as(r._h, hp(z), n, n, fmt, capi.MEM_HOST, hp(out), 128, capi.C.byref(no))

    ints = (capi.SAMPLES_SC16, capi.SAMPLES_SC8, capi.SAMPLES_CU8)
    with capi.Recc(n_channels=2, sps=10, max_samples=4096, max_bursts=4) as r:
        # -ENOSYS on an unconfigured handle; an unknown format is -EINVAL there too
        for fmt in ints:
            assert push_s(r, fmt) == push_r(r, fmt) == dbg_s(r, fmt) == dbg_r(r, fmt) == -errno.ENOSYS
        for bad in (4, -1):
            assert push_s(r, bad) == push_r(r, bad) == dbg_s(r, bad) == dbg_r(r, bad) == -errno.EINVAL
        # shared-configured: formats 4 and -1, the per-row calls, the limit of one push, nsamp == 0, a null block
        r.set_xlate_shared(400e3, [-60e3, 60e3], 2)
        for bad in (4, -1):
            assert push_s(r, bad) == dbg_s(r, bad) == -errno.EINVAL
            with pytest.raises(capi.AmpsError) as e:
                r.push_raw_shared_as(z, bad)
            assert e.value.code == -errno.EINVAL
        big = np.zeros((2 * 4096 + 1, 2), np.int16)                              # one sample past decim * max_samples_per_push
        for fmt in ints:
            assert push_r(r, fmt) == dbg_r(r, fmt) == -errno.ENOSYS
            assert push_s(r, fmt) == 0 and dbg_s(r, fmt) == 0
            assert push_s(r, fmt, n=0) == 0 and push_s(r, fmt, n=0, p=None) == 0
            assert push_s(r, fmt, p=None) == -errno.EINVAL
            assert push_s(r, fmt, n=2 * 4096, p=big) == 0
            assert push_s(r, fmt, n=2 * 4096 + 1, p=big) == -errno.E2BIG
            assert L.amps_recc_debug_xlate_shared_as(r._h, hp(big), 2 * 4096 + 1, fmt, capi.MEM_HOST, hp(out), 128, capi.C.byref(no)) == -errno.E2BIG
        # per-row-configured: the reverse
        r.set_xlate(rate_hz=400e3, center_hz=160e3, decim=2)
        for fmt in ints:
            assert push_s(r, fmt) == dbg_s(r, fmt) == -errno.ENOSYS
            assert push_r(r, fmt) == 0 and dbg_r(r, fmt) == 0
            assert push_r(r, fmt, n=0) == 0
            assert L.amps_recc_push_raw_as(r._h, hp(z), 4, 8, fmt, capi.MEM_HOST) == -errno.EINVAL        # ld < nsamp
            assert L.amps_recc_push_raw_as(r._h, hp(big), 2 * 4096 + 1, 2 * 4096 + 1, fmt, capi.MEM_HOST) == -errno.E2BIG
        for bad in (4, -1):
            assert push_r(r, bad) == dbg_r(r, bad) == -errno.EINVAL


def test_fc32_through_as_is_the_plain_call(gpu):
    x = capi.convert_samples(_ints(capi.SAMPLES_SC16, 5000, seed=97), capi.SAMPLES_SC16)
    with _shared("400k_d2", 5000) as r:
        want = r.debug_xlate_shared(x)
        r.reset()
        as_complex = r.debug_xlate_shared_as(x, capi.SAMPLES_FC32)
        r.reset()
        as_pairs = r.debug_xlate_shared_as(x.view(np.float32).reshape(-1, 2), capi.SAMPLES_FC32)
    assert _bits_equal(as_complex, want) and _bits_equal(as_pairs, want)
    rows = np.ascontiguousarray(np.stack([x, x[::-1]]))
    with capi.Recc(n_channels=2, sps=10, max_samples=5000, max_bursts=4) as r:
        r.set_xlate(rate_hz=400e3, center_hz=50e3, decim=2)
        want = r.debug_xlate(rows)
        r.reset()
        got = r.debug_xlate_as(rows, capi.SAMPLES_FC32)
    assert _bits_equal(got, want)


def test_the_binding_refuses_a_mismatched_dtype(gpu):
    import torch
    f = np.zeros((64, 2), np.float32)
    with _shared("400k_d2", 4096) as r:
        with pytest.raises(TypeError):
            r.push_raw_shared_as(f, capi.SAMPLES_SC16)                           # a float array: never a silent cast
        with pytest.raises(TypeError):
            r.debug_xlate_shared_as(np.zeros(64, np.complex64), capi.SAMPLES_SC16)
        with pytest.raises(TypeError):
            r.push_raw_shared_as(np.zeros((64, 2), np.int8), capi.SAMPLES_CU8)
        with pytest.raises(TypeError):
            r.push_raw_shared_as(np.zeros((64, 2), np.uint8), capi.SAMPLES_SC8)
        with pytest.raises(TypeError):
            r.push_raw_shared_as(np.zeros((64, 2), np.int16), capi.SAMPLES_FC32)
        with pytest.raises(TypeError):
            r.push_raw_shared_as(torch.zeros((64, 2), dtype=torch.float32, device=gpu), capi.SAMPLES_SC16)
        with pytest.raises(TypeError):
            r.push_raw_shared_as(torch.zeros((64, 2), dtype=torch.int16), capi.SAMPLES_SC16)   # a CPU tensor
        with pytest.raises(TypeError):
            r.push_raw_shared_as(np.zeros((64, 3), np.int16), capi.SAMPLES_SC16)
        r.push_raw_shared_as(np.zeros((64, 2), np.int16), capi.SAMPLES_SC16)     # the handle is still good
    with capi.Recc(n_channels=2, sps=10, max_samples=4096, max_bursts=4) as r:
        r.set_xlate(rate_hz=400e3, center_hz=50e3, decim=2)
        with pytest.raises(TypeError):
            r.push_raw_as(np.zeros((2, 64, 2), np.float32), capi.SAMPLES_SC16)
        with pytest.raises(TypeError):
            r.debug_xlate_as(np.zeros((3, 64, 2), np.int16), capi.SAMPLES_SC16)  # three rows for two channels
        r.push_raw_as(np.zeros((2, 64, 2), np.int16), capi.SAMPLES_SC16)


# ---- 6. recctest sub
def _lines_by_channel(stdout):
    got, ch = {}, None
    for line in stdout.splitlines():
        if line.startswith("MSG channel "):
            ch = int(line.split()[2])
            got.setdefault(ch, [])
        elif line.startswith("MSG "):
            got[ch].append(line)
    return got


@pytest.mark.parametrize("name", ["sc16", "cu8"])
def test_recctest_sub_reads_the_format_from_the_extension(gpu, tmp_path, name):
    """gr::amps::recc_subband with input_format through `recctest sub`: the quantised five-channel stream as a .sc16 / .cu8 file prints,
    per channel, the lines the tool prints for the fc32 file of the converted samples"""
    fmt = FORMATS[name]
    q = quantised400(fmt)
    p_int, p_f = tmp_path / ("five." + name), tmp_path / "five.raw"
    q.tofile(p_int)
    capi.convert_samples(q, fmt).tofile(p_f)
    _, exe = build_host()
    outs = []
    for p in (p_int, p_f):
        o = subprocess.run([exe, "sub", str(p), "77777", "400e3", "2", ",".join("%g" % c for c in CENTRES_400)],
                           capture_output=True, text=True, timeout=300)
        assert o.returncode == 0, o.stderr
        outs.append(o.stdout)
    got, want = _lines_by_channel(outs[0]), _lines_by_channel(outs[1])
    assert got == want and sorted(want) == list(range(5)) and all(len(v) >= 2 for v in want.values())
    assert sum(outs[0].count("MSG channel %d\n" % c) for c in range(5)) == 10
