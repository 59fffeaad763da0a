"""The shared translate seam at the rates SDRs deliver (decimations 5, 6, 10, 12, 16, 20 through xlate_shared_wide_kernel), the part
that needs no GPU: amps_recc_xlate_shared_plan -- "which decimation do I ask for?" -- in the header, the exports and the binding, its
answers for the rates the README names, and the new kernel's resource budget beside the unchanged counts of the old kernels."""
import errno
import os
import re
import shutil

import pytest

from gr_amps_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (decim, sps, ntaps) at the flow graph's transition width of 4.5 kHz
PLANS = {
    2.4e6: [(10, 12, 1793), (12, 10, 1793), (20, 6, 1793)],
    2.0e6: [(10, 10, 1495), (20, 5, 1495)],
    3.2e6: [(16, 10, 2391), (20, 8, 2391)],
    1.6e6: [(8, 10, 1195), (10, 8, 1195), (16, 5, 1195), (20, 4, 1195)],
    1.2e6: [(5, 12, 897), (6, 10, 897), (10, 6, 897), (12, 5, 897), (20, 3, 897)],
    1.0e6: [(5, 10, 747), (10, 5, 747)],
    800e3: [(4, 10, 597), (5, 8, 597), (8, 5, 597), (10, 4, 597)],
    400e3: [(2, 10, 299), (4, 5, 299), (5, 4, 299)],
    2.048e6: [],
    4e6: [],
}


def test_header_binding_and_exports():
    with open(os.path.join(ROOT, "include", "amps_recc.h")) as f:
        h = f.read()
    flat = " ".join(h.split())
    assert "typedef struct amps_recc_xlate_plan { uint32_t decim, samples_per_symbol, ntaps, _pad; } amps_recc_xlate_plan_t;" in flat
    assert "int amps_recc_xlate_shared_plan(double rate_hz, double width_hz, amps_recc_xlate_plan_t *out, size_t cap);" in flat
    assert re.search(r"#define\s+AMPS_RECC_ABI_VERSION\s+4\b", h)                  # an entry point added, nothing changed
    assert "amps_recc_xlate_shared_plan" in capi.EXPORTS
    L = capi.load()
    assert L.amps_recc_xlate_shared_plan is not None and L.amps_recc_abi_version() == 4
    assert capi.C.sizeof(capi.XlatePlan) == 16
    assert callable(capi.subband_plan)


@pytest.mark.parametrize("rate", sorted(PLANS), ids=lambda r: "%gk" % (r / 1e3))
def test_plan_for_the_rates_sdrs_deliver(rate):
    assert capi.subband_plan(rate) == PLANS[rate]
    assert capi.subband_plan(rate, 4.5e3) == PLANS[rate]                           # 0 = the flow graph's width


def test_plan_with_a_wider_transition_and_a_small_cap():
    # a 4 Msps HackRF stream: 2989 taps at 4.5 kHz exceed the limit of 2400, 2243 at 6 kHz do not; the header's 5.61 kHz is the edge
    assert capi.subband_plan(4e6, 6e3) == [(20, 10, 2243)]
    assert capi.subband_plan(4e6, 5610.0) == [(20, 10, 2399)]
    assert capi.subband_plan(4e6, 5600.0) == []                                    # 2403 taps pad to 2408
    # the old kernels' limit did not move: 2391 taps at 1.6 Msps / 8 are refused, the wide decimations of that rate take them
    assert capi.subband_plan(1.6e6, 2.25e3) == [(10, 8, 2391), (16, 5, 2391), (20, 4, 2391)]
    L = capi.load()
    out = (capi.XlatePlan * 8)()
    for i in range(8):
        out[i].decim = 99
    assert L.amps_recc_xlate_shared_plan(1.2e6, 0.0, out, 2) == 5                   # the count, whatever the cap
    assert [(p.decim, p.samples_per_symbol, p.ntaps) for p in out[:2]] == PLANS[1.2e6][:2]
    assert all(p.decim == 99 for p in out[2:])                                     # and cap entries written
    assert L.amps_recc_xlate_shared_plan(1.2e6, 0.0, None, 0) == 5


def test_plan_refuses_a_rate_that_is_not_a_positive_number():
    L = capi.load()
    out = (capi.XlatePlan * 4)()
    for bad in (float("nan"), 0.0, -2.4e6, float("inf")):
        assert L.amps_recc_xlate_shared_plan(bad, 0.0, out, 4) == -errno.EINVAL, bad
        with pytest.raises(capi.AmpsError) as e:
            capi.subband_plan(bad)
        assert e.value.code == -errno.EINVAL
    assert L.amps_recc_xlate_shared_plan(2.4e6, -1.0, out, 4) == -errno.EINVAL
    assert L.amps_recc_xlate_shared_plan(2.4e6, 0.0, None, 4) == -errno.EINVAL      # room announced, none given


def test_plan_lists_no_filter_the_design_cannot_make():
    """int(74 rate / (22 width)) made odd is 1 from a width of 74 rate / 44 (1.68 rate) upwards: the window divides by ntaps - 1 and
    every tap is NaN.  Such a width is a number, so the call succeeds, and lists nothing; three taps -- the shortest filter the formula
    makes -- are listed as before, and so is everything longer."""
    L = capi.load()
    out = (capi.XlatePlan * 8)()
    for rate in (2.4e6, 1.2e6, 400e3):
        edge = 74.0 * rate / 44.0
        assert len(PLANS[rate]) > 0
        for width in (1.0001 * edge, 1.7 * rate, 10 * rate, 1e300):                 # one tap
            assert capi.subband_plan(rate, width) == [], (rate, width)
            for i in range(8):
                out[i].decim = 99
            assert L.amps_recc_xlate_shared_plan(rate, width, out, 8) == 0
            assert all(p.decim == 99 for p in out)                                         # and nothing written
        for width, n in ((0.9999 * edge, 3), (74.0 * rate / (22.0 * 3.5), 3), (74.0 * rate / (22.0 * 5.5), 5), (74.0 * rate / (22.0 * 7.5), 7)):
            assert capi.subband_plan(rate, width) == [(d, s, n) for d, s, _ in PLANS[rate]], (rate, width)
    assert L.amps_recc_xlate_shared_plan(2.4e6, float("inf"), out, 8) == 0                 # int(0) made odd: one tap
    assert L.amps_recc_xlate_shared_plan(2.4e6, float("nan"), out, 8) == -errno.EINVAL


@pytest.fixture(scope="module")
def res():
    if not os.path.exists(build.hipcc()) or not shutil.which("c++filt"):
        if os.path.exists(build.RESOURCES):        # the report cached beside the library by the last build()
            import json
            with open(build.RESOURCES) as f:
                return json.load(f)
        pytest.skip("hipcc / c++filt not installed and no cached kernel_resources.json")
    return build.kernel_resources()


def test_wide_kernel_budget_and_the_old_kernels_counts(res):
    """2400 padded taps and a tile of 256 outputs at decimation 20 inside 80 KB of LDS -- two workgroups per CU, as the staged shared
    kernel has -- and no scratch; one instantiation per sample type.  The old kernels are as many as they were."""
    wide = {k: v for k, v in res.items() if k.startswith("void amps::xlate_shared_wide_kernel<")}
    assert len(wide) == 4, sorted(wide)
    for name, r in wide.items():
        assert r["scratch_bytes_per_lane"] == 0 and r.get("vgpr_spill", 0) == 0, (name, r)
        assert r["lds_bytes"] <= 80 * 1024, (name, r)
        assert r["waves_per_simd"] >= 2, (name, r)
    assert len([k for k in res if k.startswith("void amps::xlate_shared_kernel<")]) == 16
    assert len([k for k in res if k.startswith("void amps::xlate_fir_kernel<")]) == 12
