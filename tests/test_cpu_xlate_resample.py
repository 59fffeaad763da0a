"""The shared translate seam behind a rational L / M resampler (amps_recc_set_xlate_resampled, xlate_shared_rational_kernel), the part
that needs no GPU: the entry points in the header, the exports and the binding; amps_recc_xlate_resample_plan -- "which ratio do I
ask for?" -- for the rates no integer decimation serves; the float64 helper the GPU tests lean on (tests/xlateresampleref.py) against
the definition's own double sum; and the new kernel's resource budget beside the unchanged counts of the old kernels."""
import errno
import os
import re
import shutil

import numpy as np
import pytest

import oracle
import xlateresampleref as rr
from gr_amps_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (interp, decim, sps, taps per phase) that must be admitted at the flow graph's transition width of 4.5 kHz
MUST = {
    2.048e6: [(5, 64, 8, 1531)],
    2.5e6: [(2, 25, 10, 1869)],
    3.0e6: [(2, 25, 12, 2243)],
    1.024e6: [(5, 32, 8, 766)],
    768e3: [(5, 16, 12, 575), (5, 24, 8, 575)],
    1.25e6: [(4, 25, 10, 935)],
}


def test_header_binding_and_exports():
    with open(os.path.join(ROOT, "include", "amps_recc.h")) as f:
        h = f.read()
    flat = " ".join(h.split())
    assert "int amps_recc_set_xlate_resampled(amps_recc_t *h, const amps_recc_xlate_resample_cfg_t *x);" in flat
    assert "typedef struct amps_recc_resample_plan { uint32_t interp, decim, samples_per_symbol, ntaps_per_phase; } amps_recc_resample_plan_t;" in flat
    assert "int amps_recc_xlate_resample_plan(double rate_hz, double width_hz, amps_recc_resample_plan_t *out, size_t cap);" in flat
    m = re.search(r"typedef struct amps_recc_xlate_resample_cfg \{(.*?)\} amps_recc_xlate_resample_cfg_t;", h, re.S)
    fields = re.findall(r"(\w+)\s*(?:,|;)", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == ["struct_size", "interp", "decim", "n_centers", "_pad", "rate_hz", "gain", "cutoff_hz", "width_hz", "center_hz"]
    assert re.search(r"#define\s+AMPS_RECC_ABI_VERSION\s+4\b", h)                  # entry points added, nothing changed
    assert "there is no fractional resampler" not in h
    for name in ("amps_recc_set_xlate_resampled", "amps_recc_xlate_resample_plan"):
        assert name in capi.EXPORTS
    L = capi.load()
    assert L.amps_recc_set_xlate_resampled is not None and L.amps_recc_xlate_resample_plan is not None
    assert L.amps_recc_abi_version() == 4
    assert capi.C.sizeof(capi.XlateResampleCfg) == 64 and capi.C.sizeof(capi.ResamplePlan) == 16
    assert [f[0] for f in capi.XlateResampleCfg._fields_] == fields
    assert callable(capi.resample_plan) and callable(capi.Recc.set_xlate_resampled)


@pytest.mark.parametrize("rate", sorted(MUST), ids=lambda r: "%gk" % (r / 1e3))
def test_plan_for_the_rates_no_decimation_serves(rate):
    plan = capi.resample_plan(rate)
    for want in MUST[rate]:
        assert want in plan, (want, plan)
    assert capi.resample_plan(rate, 4.5e3) == plan                                 # 0 = the flow graph's width
    assert plan == sorted(plan)                                                    # ascending by (interp, decim)
    for L, M, sps, npp in plan:
        assert 2 <= L <= 5 and L < M <= 64 and np.gcd(L, M) == 1
        assert abs(rate * L / M - 20e3 * sps) <= 1e-6 * 20e3 * sps
        assert npp == -(-rr.prototype_ntaps(rate, 4.5e3, L) // L) and npp <= 2400
    assert capi.subband_plan(rate) == []                                           # which is why they are here


def test_plan_is_empty_where_integer_decimation_is_the_answer():
    """2.4 Msps wants L / M = sps / 120: for every sps the handle supports (3, 4, 5, 6, 8, 10, 12) the reduced fraction is 1 / D, never
    2 ... 5 over something.  (3.2 Msps is not such a rate: 12 / 160 = 3 / 40 brings it to 12 samples per symbol, which no integer
    decimation of it does.)  4 Msps under the default width is refused by both plans: 2990 taps per phase at 2/25 and more beyond."""
    for rate in (2.4e6, 4e6):
        assert capi.resample_plan(rate) == [], rate
    assert capi.subband_plan(2.4e6) != []
    assert capi.resample_plan(3.2e6) == [(3, 40, 12, 2392)]


def test_plan_limits():
    # taps per phase: 2.048 Msps x 5/64 has 1531 at 4.5 kHz; at 2.8 kHz 2461 -- beyond 2400; at 3.6 kHz 1914, within 2400, but five
    # tap sets of 1920 and the window of 64 x 64 + 1920 samples are beyond 80 KB of LDS
    assert capi.resample_plan(2.048e6, 2.8e3) == []
    assert -(-rr.prototype_ntaps(2.048e6, 2.8e3, 5) // 5) == 2461
    assert -(-rr.prototype_ntaps(2.048e6, 3.6e3, 5) // 5) == 1914
    assert capi.resample_plan(2.048e6, 3.6e3) == []
    # 2.5 Msps x 2/25: two tap sets, 25 rows: 2399 taps per phase fit
    w = 74.0 * 5.0e6 / (22.0 * (4797 + 0.5))
    assert capi.resample_plan(2.5e6, w) == [(2, 25, 10, 2399)]
    assert capi.resample_plan(2.5e6, 74.0 * 5.0e6 / (22.0 * (4803 + 0.5))) == []    # 2402 pad to 2408


def test_plan_errors_and_cap():
    L = capi.load()
    out = (capi.ResamplePlan * 8)()
    for bad in (float("nan"), 0.0, -2.048e6, float("inf")):
        assert L.amps_recc_xlate_resample_plan(bad, 0.0, out, 8) == -errno.EINVAL, bad
        with pytest.raises(capi.AmpsError) as e:
            capi.resample_plan(bad)
        assert e.value.code == -errno.EINVAL
    assert L.amps_recc_xlate_resample_plan(2.048e6, -1.0, out, 8) == -errno.EINVAL
    assert L.amps_recc_xlate_resample_plan(2.048e6, float("nan"), out, 8) == -errno.EINVAL
    assert L.amps_recc_xlate_resample_plan(2.048e6, 0.0, None, 4) == -errno.EINVAL  # room announced, none given
    assert L.amps_recc_xlate_resample_plan(2.048e6, 1e300, out, 8) == 0             # one tap: no filter, nothing listed
    full = capi.resample_plan(768e3)
    assert len(full) >= 3
    for i in range(8):
        out[i].decim = 99
    assert L.amps_recc_xlate_resample_plan(768e3, 0.0, out, 2) == len(full)         # the count, whatever the cap
    assert [(p.interp, p.decim, p.samples_per_symbol, p.ntaps_per_phase) for p in out[:2]] == full[:2]
    assert all(p.decim == 99 for p in out[2:])                                     # and cap entries written
    assert L.amps_recc_xlate_resample_plan(768e3, 0.0, None, 0) == len(full)


# ---- the float64 helper
@pytest.mark.parametrize("L,M", [(2, 25), (3, 25), (4, 25), (5, 64), (5, 16)])
def test_helper_equals_the_definitions_double_sum(L, M):
    """upfirdn(g, z, L, M) against y[k] = sum_i h_{p_k}[i] z[q_k - i] written out, on a stream that ends at every residue mod M"""
    rng = np.random.default_rng(100 * L + M)
    g = rng.standard_normal(16 * L + 3)
    for n in (1, 2, M // L, M // L + 1, 5 * M + 7, 6 * M):
        x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        a, b = rr.exact(x, g, 0.11e6, 1.0e6, L, M), rr.brute(x, g, 0.11e6, 1.0e6, L, M)
        assert a.shape == b.shape == (-(-L * n // M),)
        assert np.abs(a - b).max() <= 1e-12 * np.abs(g).sum() * np.abs(x).max()
    assert rr.nout(64, 5, 64) == 5 and rr.nout(65, 5, 64) == 6 and rr.nout(12, 5, 64) == 1 and rr.nout(13, 5, 64) == 2


def test_helper_phases_bound_and_design():
    g = np.arange(1, 12, dtype=np.float32)
    h = rr.phases(g, 3)
    assert h.shape == (3, 8) and h.dtype == np.float32
    assert h[0].tolist() == [1, 4, 7, 10, 0, 0, 0, 0] and h[2].tolist() == [3, 6, 9, 0, 0, 0, 0, 0]
    assert rr.bound(g, 3, 2.0) == (8 + 16) * 2.0 ** -24 * 26.0 * 2.0       # the phases sum to 22, 26 and 18
    # the restated design against the oracle's, where the oracle holds it: 3737 taps, the prototype of 2.5 Msps x 2/25
    a, b = rr.design(6.0, 5.0e6, 10e3, 4.5e3), oracle.firdes_low_pass(6.0, 5.0e6, 10e3, 4.5e3)
    assert len(a) == len(b) == 3737 == rr.prototype_ntaps(2.5e6, 4.5e3, 2)
    assert np.abs(a.astype(np.float64) - b).max() <= 2.0 ** -23 * np.abs(b).max()
    assert len(rr.design(15.0, 5 * 2.048e6, 10e3, 4.5e3)) == 7655


def test_helper_impulses():
    g = np.arange(1, 24, dtype=np.float32)
    L, M = 3, 7
    imp = [(40 * m + 2, 2.0 ** (m % 3)) for m in range(7)]
    x = np.zeros(300, np.complex64)
    for n0, a in imp:
        x[n0] = a
    y, seen = rr.impulse_expected(g, L, M, rr.nout(300, L, M), imp)
    assert seen.all() and np.array_equal(y, rr.exact(x, g, 0.0, 1.0, L, M).astype(np.complex64))


# ---- the kernel's budget
@pytest.fixture(scope="module")
def res():
    if not os.path.exists(build.hipcc()) or not shutil.which("c++filt"):
        if os.path.exists(build.RESOURCES):        # the report cached beside the library by the last build()
            import json
            with open(build.RESOURCES) as f:
                return json.load(f)
        pytest.skip("hipcc / c++filt not installed and no cached kernel_resources.json")
    return build.kernel_resources()


def test_rational_kernel_budget_and_the_old_kernels_counts(res):
    """five tap sets and the window of 64 x 64 + 1536 samples inside 80 KB of LDS -- two workgroups per CU, as the wide kernel has --
    and no scratch; one instantiation per sample type.  The old kernels are as many as they were."""
    rat = {k: v for k, v in res.items() if k.startswith("void amps::xlate_shared_rational_kernel<")}
    assert len(rat) == 4, sorted(rat)
    for name, r in rat.items():
        assert r["scratch_bytes_per_lane"] == 0 and r.get("vgpr_spill", 0) == 0 and r.get("sgpr_spill", 0) == 0, (name, r)
        assert r["lds_bytes"] <= 80 * 1024, (name, r)
        assert r["waves_per_simd"] >= 2, (name, r)
    assert len([k for k in res if k.startswith("void amps::xlate_shared_kernel<")]) == 16
    assert len([k for k in res if k.startswith("void amps::xlate_shared_wide_kernel<")]) == 4
    assert len([k for k in res if k.startswith("void amps::xlate_fir_kernel<")]) == 12
