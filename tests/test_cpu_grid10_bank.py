"""not gpu: the filter banks of 10 kHz bins (wideband seam at 25, 20, 10 and 5 Msps) as far as they go without a device: the plan call and
its binding, the resources of the sixteen chz_grid10_kernel instantiations, the float64 model on the burst blocks the GPU tests use, and
the kernel's pass order in complex64 against float64 on the per-bin test's input."""
import ctypes as C
import errno
import os
import re
import shutil

import numpy as np
import pytest

import oracle
import slicerbound as sb
from gr_amps_amd import build, capi

import grid10block as gb

GRID = pytest.mark.parametrize("M", gb.SIZES, ids=gb.IDS)
PLANS = {
    30.72e6: [(1024, 768, 2, 8192, 30000, 1, 1024), (1024, 512, 3, 8192, 30000, 1, 1024)],
    15.36e6: [(512, 384, 2, 4096, 30000, 1, 512), (512, 256, 3, 4096, 30000, 1, 512)],
    7.68e6: [(256, 192, 2, 2048, 30000, 1, 256), (256, 128, 3, 2048, 30000, 1, 256)],
    3.84e6: [(128, 96, 2, 1024, 30000, 1, 128), (128, 64, 3, 1024, 30000, 1, 128)],
    25e6: [(2500, 625, 2, 7500, 10000, 3, 833)],
    20e6: [(2000, 500, 2, 6000, 10000, 3, 666)],
    10e6: [(1000, 250, 2, 3000, 10000, 3, 333)],
    5e6: [(500, 125, 2, 1500, 10000, 3, 166)],
    12.5e6: [], 6.25e6: [], 2.5e6: [], 1.92e6: [],
}
FIELDS = ("channels", "decim", "samples_per_symbol", "taps", "bin_hz", "channel_stride", "max_channels")


def test_header_declares_the_grid_plan_call():
    with open(os.path.join(build._ROOT, "include", "amps_recc.h")) as f:
        text = f.read()
    assert re.search(r"typedef struct amps_recc_wideband_grid_plan \{ uint32_t channels, decim, samples_per_symbol, taps, bin_hz, channel_stride, max_channels, _pad; \} "
                     r"amps_recc_wideband_grid_plan_t;", text)
    assert re.search(r"int amps_recc_wideband_grid_plan\(double rate_hz, amps_recc_wideband_grid_plan_t \*out, size_t cap\);", text)
    assert re.search(r"#define AMPS_RECC_ABI_VERSION 4\b", text)
    assert C.sizeof(capi.WidebandGridPlan) == 32


def test_grid_plan_call_answers_per_rate():
    L = capi.load()
    assert "amps_recc_wideband_grid_plan" in capi.EXPORTS and L.amps_recc_abi_version() == 4
    for rate, want in PLANS.items():
        assert L.amps_recc_wideband_grid_plan(rate, None, 0) == len(want), rate           # cap = 0: how many the rate admits
        out = (capi.WidebandGridPlan * 4)()
        assert L.amps_recc_wideband_grid_plan(rate, out, 4) == len(want)
        assert [tuple(getattr(p, f) for f in FIELDS) for p in out[:len(want)]] == want, rate
        assert all(p._pad == 0 for p in out)
        assert capi.wideband_grid_plan(rate) == want
        # the banks of 30 kHz bins are the old call's, entry by entry; the old call knows nothing of the new rates
        assert capi.wideband_plan(rate) == [p[:4] for p in want if p[4] == 30000]
    # a cap below the count: only that many are written, the count is still returned
    out = (capi.WidebandGridPlan * 2)()
    assert L.amps_recc_wideband_grid_plan(3.84e6, out, 1) == 2
    assert (out[0].channels, out[0].decim) == (128, 96) and (out[1].channels, out[1].decim) == (0, 0)
    out = (capi.WidebandGridPlan * 1)()
    assert L.amps_recc_wideband_grid_plan(10e6, out, 1) == 1 and out[0].channels == 1000
    # within half a hertz of the rate, not beyond
    assert len(capi.wideband_grid_plan(10e6 + 0.4)) == 1 and capi.wideband_grid_plan(10e6 + 0.6) == []
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert L.amps_recc_wideband_grid_plan(bad, None, 0) == -errno.EINVAL
    assert L.amps_recc_wideband_grid_plan(10e6, None, 1) == -errno.EINVAL


def test_grid10_kernel_resources():
    if not os.path.exists(build.hipcc()) or not shutil.which("c++filt"):
        if not os.path.exists(build.RESOURCES):
            pytest.skip("hipcc / c++filt not installed and no cached kernel_resources.json")
    all_res = build.kernel_resources()
    res = {k: v for k, v in all_res.items() if k.startswith("void amps::chz_grid10_kernel<")}
    assert len(res) == 16, sorted(res)                                   # four sizes x four sample types
    seen = set()
    for name, r in res.items():
        m = re.match(r"void amps::chz_grid10_kernel<(\d+), (.*)>\(amps::ChzNarrowArgs\)$", name)
        assert m, name
        M = int(m.group(1))
        assert M in gb.SIZES, name
        seen.add((M, m.group(2)))
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0, (name, r)
        assert r["lds_bytes"] <= 163840, (name, r)
        assert r["lds_bytes"] <= 80 * 1024 and r["waves_per_simd"] >= 2, (name, r)       # two workgroups per CU: the frames take the staged input's place
    assert len(seen) == 16
    assert sum(k.startswith("void amps::chz_narrow_kernel<") for k in all_res) == 12     # the narrow banks' names are theirs alone


def test_binding_hands_create_the_grid10_geometry(monkeypatch):
    """capi.Recc: {"channels": 2000, "decim": 500} reaches create as (2000, 500, 2) with three taps per branch; an absent decim is
    still filled in as 3/4 of the channels (which the library refuses)"""
    seen = []
    L = capi.load()

    class Fake:
        def __getattr__(self, name):
            return getattr(L, name)

        def amps_recc_create(self, out, cfg):
            c = cfg._obj
            seen.append((c.wideband_channels, c.wideband_decim, c.samples_per_symbol, c.wideband_taps_per_branch, c.wideband_first_channel))
            return -errno.ENODEV

    monkeypatch.setattr(capi, "load", lambda: Fake())
    for wb, want in (({"channels": 2000, "decim": 500, "first_channel": 9}, (2000, 500, 2, 3, 9)), ({"channels": 2500, "decim": 625}, (2500, 625, 2, 3, 0)),
                     ({"channels": 1000, "decim": 250}, (1000, 250, 2, 3, 0)), ({"channels": 500, "decim": 125, "taps_per_branch": 8}, (500, 125, 2, 8, 0)),
                     ({"channels": 1000}, (1000, 750, 2, 8, 0)), ({"channels": 1000, "decim": 500}, (1000, 500, 3, 8, 0)),
                     ({"channels": 512, "decim": 128}, (512, 128, 6, 8, 0))):
        with pytest.raises(capi.AmpsError):
            capi.Recc(n_channels=4, max_samples=1024, wideband=wb)
        assert seen[-1] == want, wb


@GRID
def test_prototype_is_the_issue_s(M):
    """the geometry the tests use is the one the plan call states, and the float64 prototype has unit DC gain and -6 dB at 15 kHz"""
    (ch, D, sps, ntaps, bin_hz, stride, cmax), = capi.wideband_grid_plan(M * gb.BIN_HZ)
    assert (ch, D, sps, ntaps, bin_hz, stride, cmax) == (M, gb.decim(M), gb.SPS, gb.P * M, gb.BIN_HZ, gb.STRIDE, gb.max_channels(M))
    h = gb.taps(M)
    assert h.size == ntaps and abs(h.sum() - 1.0) < 1e-12
    gain = abs(np.sum(h * np.exp(-2j * np.pi * 15e3 / (M * gb.BIN_HZ) * np.arange(h.size))))
    assert abs(20 * np.log10(gain) + 6.02) < 0.1, gain


@GRID
def test_model_decodes_the_burst_block(M):
    """guards the inputs of the GPU tests: the float64 bank and the CPU model of the IQ seam return all six MINs"""
    _, truth = gb.burst_block(M)
    recs = oracle.fused_push_all(gb.model_rows(M).astype(np.complex64), sps=gb.SPS)
    assert len(recs) == 6
    for i, (row, off) in enumerate(gb.planted(M)):
        kind, min10, esn, dialed, words = truth[(row, off)]
        r = recs[[int(c) for c in recs["channel"]].index(i)]
        assert r["min"].decode() == min10 and r["valid"].all(), (row, off)


@GRID
def test_pass_order_in_complex64_holds_the_error_bound(M):
    """The kernel's fold and Stockham passes (radices as built, grid10block.RADICES) stated in numpy complex64, on the per-bin GPU test's
    input, against float64: |y32 - y64| <= FFT_C 2^-24 log2(M) ||Y64(frame)||_2 for every bin and frame.  Worst ratios (of the bound's
    2^-24 log2(M) ||Y64||, to hold against FFT_C = 0.54): M = 2500: 0.077, 2000: 0.081, 1000: 0.084, 500: 0.102."""
    x = gb.tone_block(M)
    want = gb.tone_model(M)
    got = gb.bank_c64(x, M)
    assert got.shape == want.shape == (M, x.size // gb.decim(M))
    norm = np.sqrt((np.abs(want) ** 2).sum(0))
    ratio = np.abs(got - want) / (sb.U32 * np.log2(M) * norm)
    print(f"\nM={M}: complex64 pass order, worst |y32 - y64| / (2^-24 log2(M) ||Y64(frame)||) = {ratio.max():.3f}")
    assert ratio.max() <= sb.FFT_C, (ratio.max(), np.unravel_index(np.argmax(ratio), ratio.shape))
    # and the statement is the bank: the same frames from numpy's FFT of the float64 fold
    assert np.allclose(got, want, rtol=0, atol=1e-5 * np.abs(want).max())
