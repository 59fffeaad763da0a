"""The translate seams on an SDR's integer samples (AMPS_RECC_SAMPLES_SC16 / _SC8 / _CU8; amps_recc_push_raw_shared_as / _push_raw_as /
_debug_xlate_shared_as / _debug_xlate_as), the part that needs no GPU: the header's definition, the exports, the null-handle answer,
and capi.convert_samples -- the definition in numpy, which tests/test_gpu_xlate_formats.py states every identity with."""
import errno
import os
import re

import numpy as np
import pytest

from gr_amps_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("amps_recc_push_raw_shared_as", "amps_recc_push_raw_as", "amps_recc_debug_xlate_shared_as", "amps_recc_debug_xlate_as")
INT_FORMATS = [(capi.SAMPLES_SC16, np.int16), (capi.SAMPLES_SC8, np.int8), (capi.SAMPLES_CU8, np.uint8)]


def _header():
    with open(os.path.join(ROOT, "include", "amps_recc.h")) as f:
        return f.read()


def test_header_carries_the_formats_and_the_prototypes():
    h = _header()
    for name, value in (("FC32", 0), ("SC16", 1), ("SC8", 2), ("CU8", 3)):
        assert re.search(r"#define\s+AMPS_RECC_SAMPLES_%s\s+%d\b" % (name, value), h), name
        assert getattr(capi, "SAMPLES_" + name) == value
    flat = " ".join(h.split())
    for proto in (
        "int amps_recc_push_raw_shared_as(amps_recc_t *h, const void *iq, size_t nsamp, int format, int mem);",
        "int amps_recc_push_raw_as(amps_recc_t *h, const void *iq, size_t ld, size_t nsamp, int format, int mem);",
        "int amps_recc_debug_xlate_shared_as(amps_recc_t *h, const void *iq, size_t nsamp, int format, int mem, float *out, size_t out_ld, size_t *nout);",
        "int amps_recc_debug_xlate_as(amps_recc_t *h, const void *iq, size_t ld, size_t nsamp, int format, int mem, float *out, size_t out_ld, size_t *nout);",
    ):
        assert proto in flat, proto
    assert re.search(r"#define\s+AMPS_RECC_ABI_VERSION\s+4\b", h)                  # entry points added, nothing changed


def test_library_exports_the_entry_points():
    L = capi.load()
    for name in NAMES:
        assert name in capi.EXPORTS
        assert getattr(L, name) is not None
    assert L.amps_recc_abi_version() == 4


def test_a_null_handle_is_einval():
    L = capi.load()
    z = np.zeros((16, 2), np.int16)
    out = np.zeros((1, 64), np.complex64)
    no = capi.C.c_size_t(0)
    for fmt in (capi.SAMPLES_FC32, capi.SAMPLES_SC16, capi.SAMPLES_SC8, capi.SAMPLES_CU8):
        assert L.amps_recc_push_raw_shared_as(None, capi._hostptr(z), 4, fmt, capi.MEM_HOST) == -errno.EINVAL
        assert L.amps_recc_push_raw_as(None, capi._hostptr(z), 4, 4, fmt, capi.MEM_HOST) == -errno.EINVAL
        assert L.amps_recc_debug_xlate_shared_as(None, capi._hostptr(z), 4, fmt, capi.MEM_HOST, capi._hostptr(out), 64, capi.C.byref(no)) == -errno.EINVAL
        assert L.amps_recc_debug_xlate_as(None, capi._hostptr(z), 4, 4, fmt, capi.MEM_HOST, capi._hostptr(out), 64, capi.C.byref(no)) == -errno.EINVAL


@pytest.mark.parametrize("fmt,dtype", INT_FORMATS, ids=["sc16", "sc8", "cu8"])
def test_convert_samples_is_exact(fmt, dtype):
    """every value of the format is a binary32 number after the plain conversion: compared in float64, at the extremes and at random"""
    info = np.iinfo(dtype)
    rng = np.random.default_rng(21 + fmt)
    a = rng.integers(info.min, info.max + 1, size=(4096, 2)).astype(dtype)
    a[0] = (info.min, info.max)
    a[1] = (info.max, info.min)
    off = 127.5 if fmt == capi.SAMPLES_CU8 else 0.0
    y = capi.convert_samples(a, fmt)
    assert y.dtype == np.complex64 and y.shape == (4096,)
    assert np.array_equal(y.real.astype(np.float64), a[:, 0].astype(np.float64) - off)
    assert np.array_equal(y.imag.astype(np.float64), a[:, 1].astype(np.float64) - off)
    want = {capi.SAMPLES_SC16: (-32768.0, 32767.0), capi.SAMPLES_SC8: (-128.0, 127.0), capi.SAMPLES_CU8: (-127.5, 127.5)}[fmt]
    assert (float(y[0].real), float(y[0].imag)) == want and (float(y[1].real), float(y[1].imag)) == want[::-1]
    # the flat shape [2n] and rows [C, n, 2] / [C, 2n] are the same samples
    assert np.array_equal(capi.convert_samples(a.reshape(-1), fmt), y)
    assert np.array_equal(capi.convert_samples(a.reshape(4, 1024, 2), fmt), y.reshape(4, 1024))
    assert np.array_equal(capi.convert_samples(a.reshape(4, 2048), fmt), y.reshape(4, 1024))


def test_convert_samples_fc32_is_the_block_itself():
    x = (np.arange(12, dtype=np.float32) - 5.5).reshape(6, 2)
    y = capi.convert_samples(x, capi.SAMPLES_FC32)
    assert y.dtype == np.complex64 and np.array_equal(y.view(np.float32).reshape(6, 2), x)
    z = y.copy()
    assert capi.convert_samples(z, capi.SAMPLES_FC32) is z


def test_convert_samples_refuses_a_mismatched_dtype():
    for fmt, dtype in INT_FORMATS:
        for other in (np.float32, np.float64, np.complex64, np.int32) + tuple(d for _, d in INT_FORMATS if d is not dtype):
            with pytest.raises(TypeError):
                capi.convert_samples(np.zeros((8, 2), other), fmt)
    with pytest.raises(TypeError):
        capi.convert_samples(np.zeros((8, 2), np.int16), capi.SAMPLES_FC32)
    with pytest.raises(TypeError):
        capi.convert_samples(np.zeros(7, np.int16), capi.SAMPLES_SC16)          # half a sample
    with pytest.raises(TypeError):
        capi.convert_samples([[1, 2]], capi.SAMPLES_SC16)                       # not an array: nothing to take a dtype from


# ---- the five-channel stream tests/test_gpu_xlate_formats.py decodes end to end, quantised as a converter would
SPACING = 3456 + 74 + 4096 + 600      # symbols between two bursts of a channel, as tests/test_gpu_xlate.py plants them
CENTRES_400 = [-160e3, -70e3, 20e3, 50e3, 160e3]
STREAM_SEED = 4100
# fixed scales: the five unit-amplitude mobiles sum to a peak of 5.03 per component with this seed, so nothing clips
# (5.03 * 4096 = 20 600 of 32 767; 5.03 * 16 = 80.5 of 127), and the 8-bit step of 1/16 leaves each mobile about 32 dB over its share
# of the quantisation noise
SCALES = {capi.SAMPLES_SC16: 4096.0, capi.SAMPLES_SC8: 16.0, capi.SAMPLES_CU8: 16.0}
_streams = {}


def stream400():
    """five mobiles' channels in one 400 ksps stream, as tests/test_gpu_xlate_shared.py builds its own: two bursts each, overlapping
    in time, two of the channels adjacent.  Returns (complex128 [400000], truth per channel)."""
    from gr_amps_amd import synth
    if "x" not in _streams:
        n = 400000
        k = np.arange(n)
        x = np.zeros(n, np.complex128)
        truth = []
        for c, fc in enumerate(CENTRES_400):
            iq, t = synth.make_channel_block(n, 5, seed=STREAM_SEED + c, sps=20, first=4000 + 9000 * c, spacing=SPACING * 20)
            x += iq * np.exp(2j * np.pi * fc * k / 400e3)
            truth.append(t)
        x.setflags(write=False)
        _streams["x"] = (x, truth)
    return _streams["x"]


def quantised400(fmt):
    """the stream in an integer format at SCALES[fmt], [400000, 2]: round to nearest (cu8: to the nearest half-odd level, i.e.
    floor(v + 128), offset binary)"""
    if fmt not in _streams:
        x, _ = stream400()
        v = np.stack([x.real, x.imag], -1) * SCALES[fmt]
        if fmt == capi.SAMPLES_CU8:
            q = np.clip(np.floor(v + 128.0), 0, 255).astype(np.uint8)
        else:
            info = np.iinfo(capi.SAMPLE_DTYPES[fmt])
            q = np.clip(np.rint(v), info.min, info.max).astype(capi.SAMPLE_DTYPES[fmt])
        q.setflags(write=False)
        _streams[fmt] = q
    return _streams[fmt]


@pytest.mark.parametrize("fmt", [capi.SAMPLES_SC16, capi.SAMPLES_SC8, capi.SAMPLES_CU8], ids=["sc16", "sc8", "cu8"])
def test_the_quantised_stream_still_decodes_on_the_cpu(fmt):
    """the condition of the end-to-end GPU test, checked where no GPU is needed: the restated reference chain (oracle.chain_iq400 per
    centre) on the CONVERTED quantised samples decodes every planted burst, and nothing clipped"""
    import oracle
    x, truth = stream400()
    q = quantised400(fmt)
    info = np.iinfo(q.dtype)
    assert q.min() > info.min and q.max() < info.max
    y = capi.convert_samples(q, fmt)
    assert [len(t) for t in truth] == [2] * 5
    for c, fc in enumerate(CENTRES_400):
        ref = oracle.chain_iq400(y, fc, chunk=4096)
        assert sorted(r["min"].decode() for r in ref) == sorted(t[2] for t in truth[c]), (fmt, c)
