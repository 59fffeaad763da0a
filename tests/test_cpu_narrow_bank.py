"""not gpu: the narrow filter banks (wideband seam at 15.36, 7.68 and 3.84 Msps) as far as they go without a device: the plan call and
its binding, the resources of the twelve chz_narrow_kernel instantiations, and the float64 model on the burst blocks the GPU tests use."""
import ctypes as C
import errno
import os
import re
import shutil

import numpy as np
import pytest

import oracle
from gr_amps_amd import build, capi

import narrowblock as nb

PLANS = {
    30.72e6: [(1024, 768, 2, 8192), (1024, 512, 3, 8192)],
    15.36e6: [(512, 384, 2, 4096), (512, 256, 3, 4096)],
    7.68e6: [(256, 192, 2, 2048), (256, 128, 3, 2048)],
    3.84e6: [(128, 96, 2, 1024), (128, 64, 3, 1024)],
    10e6: [], 20e6: [], 1.92e6: [],
}


def test_header_declares_the_plan_call():
    with open(os.path.join(build._ROOT, "include", "amps_recc.h")) as f:
        text = f.read()
    assert re.search(r"typedef struct amps_recc_wideband_plan \{ uint32_t channels, decim, samples_per_symbol, taps; \} amps_recc_wideband_plan_t;", text)
    assert re.search(r"int amps_recc_wideband_plan\(double rate_hz, amps_recc_wideband_plan_t \*out, size_t cap\);", text)
    assert re.search(r"#define AMPS_RECC_ABI_VERSION 4\b", text)


def test_plan_call_answers_per_rate():
    L = capi.load()
    assert "amps_recc_wideband_plan" in capi.EXPORTS and L.amps_recc_abi_version() == 4
    for rate, want in PLANS.items():
        assert L.amps_recc_wideband_plan(rate, None, 0) == len(want), rate            # cap = 0: how many the rate admits
        out = (capi.WidebandPlan * 4)()
        assert L.amps_recc_wideband_plan(rate, out, 4) == len(want)
        assert [(p.channels, p.decim, p.samples_per_symbol, p.taps) for p in out[:len(want)]] == want, rate
        assert capi.wideband_plan(rate) == want
    # a cap below the count: only that many are written, the count is still returned
    out = (capi.WidebandPlan * 2)()
    assert L.amps_recc_wideband_plan(3.84e6, out, 1) == 2
    assert (out[0].channels, out[0].decim) == (128, 96) and (out[1].channels, out[1].decim) == (0, 0)
    # within half a hertz of the rate, not beyond
    assert len(capi.wideband_plan(3.84e6 + 0.4)) == 2 and capi.wideband_plan(3.84e6 + 0.6) == []
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert L.amps_recc_wideband_plan(bad, None, 0) == -errno.EINVAL
    assert L.amps_recc_wideband_plan(3.84e6, None, 2) == -errno.EINVAL


def test_narrow_kernel_resources():
    if not os.path.exists(build.hipcc()) or not shutil.which("c++filt"):
        if not os.path.exists(build.RESOURCES):
            pytest.skip("hipcc / c++filt not installed and no cached kernel_resources.json")
    res = {k: v for k, v in build.kernel_resources().items() if k.startswith("void amps::chz_narrow_kernel<")}
    assert len(res) == 12, sorted(res)                                   # three M x two D x two sample types
    seen = set()
    for name, r in res.items():
        m = re.match(r"void amps::chz_narrow_kernel<(\d+), (\d+), (.*)>\(amps::ChzNarrowArgs\)$", name)
        assert m, name
        M, D = int(m.group(1)), int(m.group(2))
        assert (M, D) in nb.GEOMETRIES, name
        seen.add((M, D, "sc16" in m.group(3)))
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["lds_bytes"] <= 80 * 1024, (name, r)                   # two workgroups per CU
        assert r["waves_per_simd"] >= 2, (name, r)
    assert len(seen) == 12


def test_binding_fills_in_the_narrow_defaults(monkeypatch):
    """capi.Recc: decim absent = 3/4 of the channels, the samples per symbol 3 channels / (2 decim) -- seen in the cfg handed to create"""
    seen = []
    L = capi.load()

    class Fake:
        def __getattr__(self, name):
            return getattr(L, name)

        def amps_recc_create(self, out, cfg):
            c = cfg._obj
            seen.append((c.wideband_channels, c.wideband_decim, c.samples_per_symbol))
            return -errno.ENODEV

    monkeypatch.setattr(capi, "load", lambda: Fake())
    for wb, want in (({"channels": 128}, (128, 96, 2)), ({"channels": 512, "decim": 256}, (512, 256, 3)), ({"channels": 256, "decim": 0}, (256, 192, 2)),
                     ({"channels": 1024, "decim": 512}, (1024, 512, 3)), ({"channels": 1024}, (1024, 768, 2))):
        with pytest.raises(capi.AmpsError):
            capi.Recc(n_channels=4, max_samples=1024, wideband=wb)
        assert seen[-1] == want, wb


@pytest.mark.parametrize("M,D", nb.GEOMETRIES, ids=nb.IDS)
def test_model_decodes_the_burst_block(M, D):
    """guards the inputs of the GPU tests: the float64 bank and the CPU model of the IQ seam return all six MINs"""
    _, truth = nb.burst_block(M, D)
    recs = oracle.fused_push_all(nb.model_rows(M, D), sps=nb.sps_of(M, D))
    assert len(recs) == 6
    for i, (k, off) in enumerate(nb.planted(M)):
        kind, min10, esn, dialed, words = truth[(k, off)]
        r = recs[[int(c) for c in recs["channel"]].index(i)]
        assert r["min"].decode() == min10 and r["valid"].all(), (k, off)
