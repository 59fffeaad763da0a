"""not gpu: the wideband seam's L / M resampler (amps_recc_set_wideband_resample) as far as it goes without a device: the header and
the binding, the plan call, the admission rule stand-alone under sanitizers against the rule in Python, scipy's upfirdn against the
definition's double sum, the float64 chain on the burst blocks the GPU tests decode, and the kernels' resources."""
import ctypes as C
import errno
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from gr_amps_amd import build, capi

import wbresampleref as wr

ROOT = build._ROOT
CSRC = os.path.join(ROOT, "gr_amps_amd", "csrc")
NEW = ("amps_recc_set_wideband_resample", "amps_recc_wideband_resample_plan", "amps_recc_debug_wideband_resample")
# (interp, decim, channels, bank_decim) the issue expects by the rule
PLANS = {
    8e6: [(5, 2, 2000, 500), (5, 4, 1000, 250), (5, 8, 500, 125)],
    12.5e6: [(2, 1, 2500, 625), (4, 5, 1000, 250), (8, 5, 2000, 500)],
    3.2e6: [(6, 5, 128, 96), (6, 5, 128, 64)],
    56e6: [],
}


def test_header_binding_and_exports():
    hdr = open(os.path.join(ROOT, "include", "amps_recc.h")).read()
    assert re.search(r"typedef struct amps_recc_wideband_resample_cfg \{\s*uint32_t struct_size, interp, decim, _pad;[^}]*double\s+rate_hz;[^}]*"
                     r"double\s+cutoff_hz, width_hz;[^}]*\} amps_recc_wideband_resample_cfg_t;", hdr)
    assert "int amps_recc_set_wideband_resample(amps_recc_t *h, const amps_recc_wideband_resample_cfg_t *r);" in hdr
    assert re.search(r"typedef struct amps_recc_wideband_resample_plan \{\s*uint32_t interp, decim, channels, bank_decim, samples_per_symbol, ntaps_per_phase, "
                     r"bin_hz, channel_stride, usable_hz, _pad;\s*\} amps_recc_wideband_resample_plan_t;", hdr)
    assert "int amps_recc_wideband_resample_plan(double rate_hz, amps_recc_wideband_resample_plan_t *out, size_t cap);" in hdr
    assert ("int amps_recc_debug_wideband_resample(amps_recc_t *h, const void *iq, size_t nsamp, int format, int mem, float *out, size_t cap, "
            "size_t *nout);") in hdr
    assert re.search(r"#define AMPS_RECC_ABI_VERSION 4\b", hdr)
    assert C.sizeof(capi.WidebandResampleCfg) == 40 and C.sizeof(capi.WidebandResamplePlan) == 40
    L = capi.load()
    assert L.amps_recc_abi_version() == 4
    for name in NEW:
        assert name in capi.EXPORTS and hasattr(L, name)


def test_plan_answers_per_rate():
    L = capi.load()
    for rate, want in PLANS.items():
        assert L.amps_recc_wideband_resample_plan(rate, None, 0) == len(want), rate
        got = capi.wideband_resample_plan(rate)
        assert [g[:4] for g in got] == want, rate
        for interp, decim, ch, bd, sps, npp, bin_hz, stride, usable in got:
            f_low = min(rate, wr.bank_rate(ch))
            cutoff, width = wr.default_filter(rate, ch)
            assert (bin_hz, stride) == (int(wr.BANKS[ch][0]), wr.BANKS[ch][1]) and sps == int(wr.bank_rate(ch) / bd / 20e3)
            assert npp == -(-wr.prototype_ntaps(rate, interp, width) // interp) and usable == round(2 * (f_low / 2 - width))
    # the defaults give 54 taps per phase when resampling up and about 108 at 1 / 2
    assert {g[5] for g in capi.wideband_resample_plan(12.5e6) if g[0] > g[1] and g[2] != 1000} == {54}
    # a bank's own rate lists only true resamplings
    own = capi.wideband_resample_plan(7.68e6)
    assert [g[:4] for g in own] == [(1, 2, 128, 96), (1, 2, 128, 64), (2, 1, 512, 384), (2, 1, 512, 256), (4, 1, 1024, 768), (4, 1, 1024, 512)]
    assert own[0][5] == 107 and all(g[0] != g[1] for g in own)
    # 4 Msps: the GPU tests' block takes the second entry
    assert [g[:4] for g in capi.wideband_resample_plan(4e6)] == [(5, 2, 1000, 250), (5, 4, 500, 125)]
    # cap and error conventions of amps_recc_wideband_grid_plan
    out = (capi.WidebandResamplePlan * 3)()
    assert L.amps_recc_wideband_resample_plan(8e6, out, 1) == 3
    assert (out[0].interp, out[0].decim, out[0].channels) == (5, 2, 2000) and (out[1].interp, out[1].channels) == (0, 0)
    assert L.amps_recc_wideband_resample_plan(8e6, out, 3) == 3 and all(p._pad == 0 for p in out)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert L.amps_recc_wideband_resample_plan(bad, None, 0) == -errno.EINVAL
    assert L.amps_recc_wideband_resample_plan(8e6, None, 1) == -errno.EINVAL
    # the existing plan calls know nothing of these rates
    for rate in (8e6, 12.5e6, 3.2e6, 4e6):
        assert capi.wideband_grid_plan(rate) == [] and capi.wideband_plan(rate) == []


def test_binding_hands_the_fields_through(monkeypatch):
    seen = []
    L = capi.load()

    class Fake:
        def __getattr__(self, name):
            return getattr(L, name)

        def amps_recc_create(self, out, cfg):
            c = cfg._obj
            seen.append(("create", c.wideband_channels, c.wideband_decim, c.samples_per_symbol, c.wideband_taps_per_branch, c.wideband_first_channel))
            out._obj.value = 0x1000
            return 0

        def amps_recc_destroy(self, h):
            seen.append(("destroy",))

        def amps_recc_set_wideband_resample(self, h, x):
            c = x._obj
            seen.append(("set", c.struct_size, c.interp, c.decim, c._pad, c.rate_hz, c.cutoff_hz, c.width_hz))
            return -errno.EBUSY if c.interp == 7 else 0

    monkeypatch.setattr(capi, "load", lambda: Fake())
    monkeypatch.setattr(capi, "_lib", Fake())
    r = capi.Recc(n_channels=4, max_samples=1024, wideband={"channels": 500, "decim": 125, "first_channel": 7, "resample": (4e6, 5, 4)})
    assert seen == [("create", 500, 125, 2, 3, 7), ("set", 40, 5, 4, 0, 4e6, 0.0, 0.0)] and r.resample == (5, 4)
    r.set_wideband_resample(3.2e6, 6, 5, cutoff_hz=1.5e6, width_hz=2e5)
    assert seen[-1] == ("set", 40, 6, 5, 0, 3.2e6, 1.5e6, 2e5) and r.resample == (6, 5)
    r.set_wideband_resample(0.0, 1, 0)
    assert seen[-1][1:4] == (40, 1, 0) and r.resample is None
    with pytest.raises(capi.AmpsError) as e:
        r.set_wideband_resample(4e6, 7, 4)
    assert e.value.code == -errno.EBUSY and r.resample is None
    r.close()
    # a refusal inside the constructor destroys the handle it made
    seen.clear()
    with pytest.raises(capi.AmpsError):
        capi.Recc(n_channels=4, max_samples=1024, wideband={"channels": 500, "decim": 125, "resample": (4e6, 7, 4)})
    assert [s[0] for s in seen] == ["create", "set", "destroy"]


# ---- the admission rule, stand-alone under sanitizers, against the rule written out here
def _ntaps(fs, width):
    want = 74.0 * fs / (22.0 * width)
    n = int(want) if want < 1e9 else 1000000000
    return n if n & 1 else n + 1


def _rule(channels, L, M, rate, width, cutoff):
    """(verdict, ng, npp, ntp, cutoff, width, usable) by the issue's rule"""
    refuse = (-errno.EINVAL, 0, 0, 0, 0.0, 0.0, 0.0)
    if not (1 <= L <= 8 and 1 <= M <= 8) or L == M or math.gcd(L, M) != 1 or 2 * L < M or L > 4 * M:
        return refuse
    if not (rate > 0 and math.isfinite(rate)):
        return refuse
    br = wr.bank_rate(channels)
    if abs(rate * L / M - br) > 1e-6 * br:
        return refuse
    f_low = min(rate, br)
    width = width or f_low / 16.0
    cutoff = cutoff or 0.5 * f_low - 0.5 * width
    ng = _ntaps(L * rate, width)
    if ng < 3 or not (0 < cutoff <= 0.5 * L * rate):
        return refuse
    npp = -(-ng // L)
    ntp = -(-npp // 8) * 8
    lds = 4 * L * ntp + 8 * (-(-wr.TILE * M // L) + ntp)
    verdict = -errno.E2BIG if ng > 1000000 or ntp > 512 or lds > 65536 else 0
    return (verdict, ng, npp, ntp, cutoff, width, 2.0 * (0.5 * f_low - width))


def test_admission_stand_alone_under_sanitizers(tmp_path):
    """gr_amps_amd/csrc/recc_wideband_resample.h is free of HIP: tests/wideband_resample_host.cc has its own main, is compiled with
    -fsanitize=address,undefined and run as a program of its own.  It sweeps L and M over 0 ... 9, four rates, four widths and three
    cut-offs over the eight banks; every line is compared with the rule above."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "wideband_resample_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "wideband_resample_host.cc"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert out[-1] == "wideband resample ok"
    lines = out[:-1]
    assert len(lines) == 8 * 10 * 10 * 4 * 4 * 3
    verdicts = {0: 0, -errno.EINVAL: 0, -errno.E2BIG: 0}
    for line in lines:
        a, b = line.split(" : ")
        ch, L, M, rate, width, cutoff = a.split()
        got = b.split()
        want = _rule(int(ch), int(L), int(M), float(rate), float(width), float(cutoff))
        assert (int(got[0]), int(got[1]), int(got[2]), int(got[3])) == want[:4], line
        assert [float(v) for v in got[4:]] == list(want[4:]), line
        verdicts[want[0]] += 1
    assert all(v > 0 for v in verdicts.values()), verdicts                 # the sweep meets all three answers


# ---- the reference against the definition
@pytest.mark.parametrize("rate,L,M,channels", wr.RATIOS, ids=wr.RATIO_IDS)
def test_upfirdn_is_the_definitions_double_sum(rate, L, M, channels):
    g = wr.prototype64(rate, L, channels)
    assert len(g) == wr.prototype_ntaps(rate, L, wr.default_filter(rate, channels)[1]) and abs(g.sum() - L) < 1e-9
    assert wr.ntp_of(g, L) == (112 if L < M else 56)
    g32 = wr.prototype32(rate, L, channels)
    assert len(g32) == len(g) and np.abs(g32 - g).max() <= 2.0 ** -24 * np.abs(g).max()
    rng = np.random.default_rng(L * 10 + M)
    for n in (1, 2, M, 3 * len(g) // L + 5):
        x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        y, d = wr.upfirdn(x, g, L, M), wr.definition(x, g, L, M)
        assert y.shape == d.shape == (wr.nout(n, L, M),)
        assert np.abs(y - d).max() <= 1e-12 * L * np.abs(x).max() * np.abs(g).sum()
    # the design's -6 dB point is the cut-off, half a width below f_low / 2
    cutoff, width = wr.default_filter(rate, channels)
    assert cutoff + 0.5 * width == 0.5 * min(rate, wr.bank_rate(channels))
    gain = abs(np.sum(g * np.exp(-2j * np.pi * cutoff / (L * rate) * np.arange(len(g))))) / L
    assert abs(20 * np.log10(gain) + 6.02) < 0.1, gain


@pytest.mark.parametrize("name", sorted(wr.BURSTS))
def test_float64_chain_decodes_the_burst_block(name):
    """guards the inputs of the GPU tests: upfirdn -> oracle.channelizer.channelize -> oracle.fused_push_all(sps = 2) returns all six
    MINs of the block"""
    b = wr.BURSTS[name]
    _, truth = wr.burst_block(name)
    recs = wr.burst_model(name)
    assert len(recs) == 6
    for i, row in enumerate(b.rows):
        kind, min10, esn, dialed, words = truth[row]
        r = recs[[int(c) for c in recs["channel"]].index(i)]
        assert r["min"].decode() == min10 and r["valid"].all(), (name, row)


def test_resample_kernel_resources():
    if not os.path.exists(build.hipcc()) or not shutil.which("c++filt"):
        if not os.path.exists(build.RESOURCES):
            pytest.skip("hipcc / c++filt not installed and no cached kernel_resources.json")
    all_res = build.kernel_resources()
    res = {k: v for k, v in all_res.items() if k.startswith("void amps::wb_resample_kernel<")}
    assert len(res) == 4, sorted(res)                                      # one per sample type
    carry = {k: v for k, v in all_res.items() if k.startswith("void amps::wb_resample_carry_kernel<")}
    assert len(carry) == 4, sorted(carry)
    for name, r in list(res.items()) + list(carry.items()):
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["lds_bytes"] <= 64 * 1024, (name, r)
    # ... which says little: the kernel's LDS is dynamic (extern __shared__), so the code object's static figure is 0.  What a launch
    # asks for is wbr_lds_bytes, held below 64 KB by wbr_limits (swept above against _rule, which writes the same sum out); here the
    # same sum at the longest filter admitted, for every ratio admitted: the tap limit binds first
    worst = 0
    for L in range(1, 9):
        for M in range(1, 9):
            if L != M and math.gcd(L, M) == 1 and M <= 2 * L <= 8 * M:
                worst = max(worst, 4 * L * 512 + 8 * (-(-wr.TILE * M // L) + 512))
    assert 0 < worst <= 64 * 1024, worst
    # the header of the kernel holds no inline assembly
    assert not re.search(r"\basm\b", open(os.path.join(CSRC, "recc_wideband_resample.hip.h")).read())
