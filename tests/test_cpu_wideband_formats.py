"""not gpu: 8-bit I/Q (sc8, cu8) through the wideband seam (amps_recc_push_wideband_as / amps_recc_debug_channelize_as) as far as it
goes without a device: the declarations and the definition in the header, the binding and its refusals, the resources of the twelve
chz_narrow_b8_kernel instantiations, and the float64 model on the quantised burst blocks tests/test_gpu_wideband_formats.py decodes."""
import ctypes as C
import errno
import os
import re
import shutil

import numpy as np
import pytest

import oracle
from oracle import channelizer as cz
from gr_amps_amd import build, capi

import formatblock as fb
import narrowblock as nb

NAMES = ("amps_recc_push_wideband_as", "amps_recc_debug_channelize_as")


def _header():
    with open(os.path.join(build._ROOT, "include", "amps_recc.h")) as f:
        return f.read()


def test_header_declares_and_defines_the_entry_points():
    text = _header()
    assert re.search(r"int amps_recc_push_wideband_as\(amps_recc_t \*h, const void \*iq, size_t nsamp, int format, int mem\);", text)
    assert re.search(r"int amps_recc_debug_channelize_as\(amps_recc_t \*h, const void \*iq, size_t nsamp, int format, int mem,\s*"
                     r"float \*out, size_t out_ld, size_t \*nframes\);", text)
    assert re.search(r"#define AMPS_RECC_ABI_VERSION 4\b", text)
    assert "still 4, two entry points added and nothing changed: amps_recc_push_wideband_as" in text
    # the definition, in the words of the translate seams' paragraph
    flat = " ".join(text.replace("\n *", " ").split())
    i = flat.index("wideband seam on an SDR's integer samples")
    para = flat[i:flat.index("int amps_recc_push_wideband_as(", i)]
    for phrase in ("DEFINITION.  Each _as call is the fc32 call of the same name", "no scaling", "127.5", "exact in binary32", "the same fc32 carry",
                   "-EINVAL", "-ENOSYS", "-E2BIG", "-ESTALE", "nsamp == 0 returns 0", "IS amps_recc_push_wideband,", "IS amps_recc_push_wideband_short",
                   "an unknown format is -EINVAL", "alternate push by push", "nsamp counts SAMPLES", "2 bytes for sc8 and cu8", "odd sample",
                   "staged as it is", "input's own units squared"):
        assert " ".join(phrase.split()) in para, phrase
    # what is still not offered, and no longer the 8-bit wideband input
    assert "8-bit input on the wideband seam" not in text
    assert re.search(r"Not offered in integer formats: amps_recc_push_iq[^/]*distributed pushes", flat)


def test_binding_and_library_export_both():
    L = capi.load()
    assert L.amps_recc_abi_version() == 4
    for name in NAMES:
        assert name in capi.EXPORTS and hasattr(L, name)
    assert L.amps_recc_push_wideband_as.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int]
    assert L.amps_recc_debug_channelize_as.argtypes == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    assert "push_wideband_as" in capi.convert_samples.__doc__


def test_null_handle_is_einval_whatever_the_rest():
    L = capi.load()
    buf = np.zeros((8, 2), np.int8)
    out = np.zeros((4, 8), np.complex64)
    nf = C.c_size_t(0)
    for fmt in (0, 1, 2, 3, 7, -1):
        for n in (0, 8):
            for mem in (capi.MEM_HOST, capi.MEM_DEVICE):
                assert L.amps_recc_push_wideband_as(None, capi._hostptr(buf), n, fmt, mem) == -errno.EINVAL
                assert L.amps_recc_push_wideband_as(None, None, n, fmt, mem) == -errno.EINVAL
                assert L.amps_recc_debug_channelize_as(None, capi._hostptr(buf), n, fmt, mem, capi._hostptr(out), 8, C.byref(nf)) == -errno.EINVAL


def test_binding_refuses_a_dtype_that_does_not_match_the_format():
    """before any device is needed: the check stands in front of the handle's first use"""
    r = capi.Recc.__new__(capi.Recc)              # no handle behind it: a TypeError must come before one is touched
    r._h, r.sync_torch, r.n_channels, r.decim = None, False, 4, 96
    bad = [(np.zeros((8, 2), np.float32), capi.SAMPLES_SC8), (np.zeros(8, np.complex64), capi.SAMPLES_SC8), (np.zeros((8, 2), np.uint8), capi.SAMPLES_SC8),
           (np.zeros((8, 2), np.int8), capi.SAMPLES_CU8), (np.zeros((8, 2), np.int16), capi.SAMPLES_CU8), (np.zeros((8, 2), np.int8), capi.SAMPLES_SC16),
           (np.zeros((8, 2), np.int8), capi.SAMPLES_FC32), (np.zeros((8, 3), np.int8), capi.SAMPLES_SC8), (np.zeros(7, np.int8), capi.SAMPLES_SC8),
           ([1, 2], capi.SAMPLES_SC8)]
    for a, fmt in bad:
        with pytest.raises(TypeError):
            r.push_wideband_as(a, fmt)
        with pytest.raises(TypeError):
            r.debug_channelize_as(a, fmt)


def test_b8_kernel_resources():
    if not os.path.exists(build.hipcc()) or not shutil.which("c++filt"):
        if not os.path.exists(build.RESOURCES):
            pytest.skip("hipcc / c++filt not installed and no cached kernel_resources.json")
    allk = build.kernel_resources()
    res = {k: v for k, v in allk.items() if k.startswith("void amps::chz_narrow_b8_kernel<")}
    assert len(res) == 12, sorted(res)                                   # three M x two D x two sample types
    seen = set()
    for name, r in res.items():
        m = re.match(r"void amps::chz_narrow_b8_kernel<(\d+), (\d+), amps::xl_(sc8|cu8)>\(amps::ChzNarrowArgs\)$", name)
        assert m, name
        M, D = int(m.group(1)), int(m.group(2))
        assert (M, D) in nb.GEOMETRIES, name
        seen.add((M, D, m.group(3)))
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["lds_bytes"] <= 80 * 1024, (name, r)                   # two workgroups per CU
        assert r["waves_per_simd"] >= 2, (name, r)
    assert len(seen) == 12
    assert len([k for k in allk if k.startswith("void amps::chz_narrow_kernel<")]) == 12   # the fc32 and sc16 kernels keep their name and number


def test_quantisers_are_within_half_a_step():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(4096) + 1j * rng.standard_normal(4096)).astype(np.complex64)
    peak = max(np.abs(x.real).max(), np.abs(x.imag).max())
    v = np.stack([x.real, x.imag], axis=1).astype(np.float64) * (100.0 / peak)
    for fmt in (fb.SC8, fb.CU8):
        q = fb.quantise(x, fmt)
        back = capi.convert_samples(q, fmt)
        err = np.abs(np.stack([back.real, back.imag], axis=1) - v)
        assert q.dtype == capi.SAMPLE_DTYPES[fmt] and err.max() <= 0.5
    half = capi.convert_samples(fb.quantise(x, fb.CU8), fb.CU8)
    assert np.all(np.abs(half.real % 1.0) == 0.5)                        # cu8 levels are half-odd
    s = capi.convert_samples(fb.silence(6, fb.CU8), fb.CU8)
    assert np.array_equal(s, np.array([-0.5 + 0.5j, 0.5 - 0.5j] * 3, np.complex64))
    assert not capi.convert_samples(fb.silence(6, fb.SC8), fb.SC8).any()


CASES = [(M, D, fmt, fs) for M, D in nb.GEOMETRIES for fmt, fs in ((fb.SC8, 100.0), (fb.SC8, 24.0), (fb.CU8, 100.0))]


@pytest.mark.parametrize("M,D,fmt,full_scale", CASES, ids=["%s-%s-fs%d" % (i, fb.FORMAT_IDS[f], s) for i in nb.IDS for f, s in ((fb.SC8, 100), (fb.SC8, 24), (fb.CU8, 100))])
def test_model_decodes_the_quantised_burst_block(M, D, fmt, full_scale):
    """guards the inputs of the GPU tests: the quantised block, converted by capi.convert_samples, through the float64 bank and the CPU
    model of the IQ seam returns all six MINs with every word valid"""
    q, xf, truth = fb.burst_block_as(M, D, fmt, full_scale)
    assert q.dtype == capi.SAMPLE_DTYPES[fmt] and xf.dtype == np.complex64 and xf.shape == (q.shape[0],)
    chan = cz.channelize(xf, P=8, M=M, D=D, taps=nb.taps(M, D))
    rows = chan[[k for k, _ in nb.planted(M)]].astype(np.complex64)
    recs = oracle.fused_push_all(rows, sps=nb.sps_of(M, D))
    assert len(recs) == 6
    for i, (k, off) in enumerate(nb.planted(M)):
        kind, min10, esn, dialed, words = truth[(k, off)]
        r = recs[[int(c) for c in recs["channel"]].index(i)]
        assert r["min"].decode() == min10 and r["valid"].all(), (k, off)
