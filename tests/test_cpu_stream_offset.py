"""not gpu: the carrier-offset measurement of the IQ and translate seams (AMPS_RECC_FLAG_STREAM_OFFSET, include/amps_recc.h) as far as
it can be checked without a device -- the flag and the three entry points in the header and the binding, the resources of the two
kernels, the float64 model tests/streamoffsetref.py that the GPU tests compare against, and the estimator itself on synthetic bursts.

The estimator's bounds are twice the worst error of DESIGN.md 4.7g's IQ-seam table (four seeds per point): 7 / 33 Hz at 10 samples
per symbol and 30 / 10 dB, 12 / 80 Hz at 3.  The seeds here are those of scripts/offset_estimator_cpu.py, whose own draw reads 5 / 51
and 10 / 80 Hz."""
import inspect
import os
import re
import shutil

import numpy as np
import pytest

import streamoffsetref as sor
import streampowerref as spr
from gr_amps_amd import build, capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("amps_recc_channel_autocorr", "amps_recc_burst_autocorr", "amps_recc_burst_offset")


def test_header_has_the_flag_and_the_entry_points_and_the_abi_version_stands():
    hdr = open(os.path.join(ROOT, "include", "amps_recc.h")).read()
    assert re.search(r"#define\s+AMPS_RECC_FLAG_STREAM_OFFSET\s+0x800u", hdr)
    assert re.search(r"#define\s+AMPS_RECC_ABI_VERSION\s+4\b", hdr)
    flags = re.findall(r"#define\s+(AMPS_RECC_FLAG_\w+)\s+(0x[0-9a-fA-F]+)u", hdr)
    assert [n for n, v in flags if int(v, 16) & 0x800] == ["AMPS_RECC_FLAG_STREAM_OFFSET"]      # no other flag has the bit
    assert len({int(v, 16) for _, v in flags}) == len(flags)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(amps_recc_t \*h" % name, code), name


def test_binding_has_the_flag_the_argument_and_the_three_functions():
    assert capi.FLAG_STREAM_OFFSET == 0x800
    p = inspect.signature(capi.Recc.__init__).parameters
    assert "stream_offset" in p and p["stream_offset"].default is False
    L = capi.load()
    assert L.amps_recc_abi_version() == 4
    for name in NEW:
        assert name in capi.EXPORTS and getattr(L, name) is not None
    for name in ("channel_autocorr", "burst_autocorr", "burst_offset"):
        assert callable(getattr(capi.Recc, name))
    # a null handle is refused without a device, as by the power entry points
    assert L.amps_recc_channel_autocorr(None, 0, 0, None, 0, None, None) == -22
    assert L.amps_recc_burst_autocorr(None, None, 0, None, None) == -22
    assert L.amps_recc_burst_offset(None, None, 0, None, None) == -22


@pytest.fixture(scope="module")
def res():
    if not os.path.exists(build.hipcc()) or not shutil.which("c++filt"):
        if os.path.exists(build.RESOURCES):
            import json
            with open(build.RESOURCES) as f:
                return json.load(f)
        pytest.skip("hipcc / c++filt not installed and no cached kernel_resources.json")
    return build.kernel_resources()


def test_offset_kernels_need_no_scratch_and_no_lds(res):
    block = {k: v for k, v in res.items() if "amps::stream_autocorr_kernel(" in k}
    gather = {k: v for k, v in res.items() if "amps::autocorr_ring_gather_kernel(" in k}
    assert len(block) == 1 and len(gather) == 1, (sorted(block), sorted(gather))
    for name, r in {**block, **gather}.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["lds_bytes"] == 0, (name, r)
    # the power kernels are still there, once each, and the names do not collide with the prefixes other tests count instantiations by
    assert len([k for k in res if "amps::stream_power_kernel(" in k]) == 1
    assert len([k for k in res if "amps::power_ring_gather_kernel(" in k]) == 1
    for name in list(block) + list(gather):
        assert not re.search(r"amps::(chz12_kernel<|recc_front_kernel<|recc_resolve_kernel<|chz_power_kernel<|stream_power_kernel\(|power_ring_gather_kernel\()", name), name


def test_model_reads_a_carrier_and_puts_a_zero_in_front_of_the_stream():
    a, f, fs = 0.37, 1234.0, 200e3
    n = 256 * 9 + 100
    y = a * np.exp(2j * np.pi * f * np.arange(n) / fs)
    A = sor.blocks(y)
    assert A.shape == (1, 9) and A.dtype == np.complex128
    want = a * a * np.exp(2j * np.pi * f / fs)
    assert np.all(np.abs(A[0, 1:] - want) <= 1e-12)
    assert abs(A[0, 0] - want * 255.0 / 256.0) <= 1e-12              # the first product is y[0] * conj(0)
    assert all(abs(sor.offset_hz(v, 10) - f) < 1e-6 for v in A[0])
    assert np.all(np.abs(sor.weights(y)[0, 1:] - a * a) <= 1e-12)
    # an origin moves the block edges as it moves the power blocks, and the zero stands in front of the FIRST sample, not of a block
    origin = 64 * 15
    A2 = sor.blocks(y, origin=origin)
    assert sor.first_block(origin) == spr.first_block(origin) == 4 and A2.shape == (1, 9)
    assert np.all(np.abs(A2 - want) <= 1e-12)                        # block 4 begins 64 samples into the stream: no zero in it
    A3 = sor.blocks(y, origin=1024)
    assert abs(A3[0, 0] - want * 255.0 / 256.0) <= 1e-12             # block 4 begins at the origin
    assert sor.blocks(np.zeros(255, complex)).shape == (1, 0) and sor.blocks(np.ones((3, 512), complex)).shape == (3, 2)


def test_model_burst_sums_share_the_window_of_burst_power():
    row = (np.arange(200) + 1j * np.arange(200)[::-1]).astype(np.complex128)
    for sps in (3, 10, 12):
        j0, cnt = sor.burst_window(700, sps)
        assert (j0, cnt) == spr.burst_window(700, sps)
        total, n = sor.burst_sum(row, 700, sps)
        assert n == cnt and total == complex(np.sum(row[j0:j0 + cnt]))
        assert sor.burst_sum(row[:j0 + cnt - 1], 700, sps) == (0j, 0)      # the last block is not produced yet
        assert sor.burst_sum(row, 700, sps, first=j0 + 1) == (0j, 0)       # the first block has left the window
        assert sor.burst_offset_hz(row, 700, sps, first=j0 + 1) == (0.0, 0)
    assert sor.offset_hz(0j, 10) == 0.0 and sor.offset_hz(1j, 10) == 50000.0 and sor.offset_hz(-1j, 3) == -15000.0


def test_gather_restatement_adds_each_component_in_the_stated_order():
    rng = np.random.default_rng(5)
    e = (rng.standard_normal(158) + 1j * rng.standard_normal(158)).astype(np.complex64)
    re, im = sor.gather_sum(e)
    assert re.dtype == np.float32 and im.dtype == np.float32
    exact = np.sum(e.astype(np.complex128))
    assert abs(float(re) - exact.real) <= 158 * 2.0 ** -24 * np.abs(e.real).sum()
    assert abs(float(im) - exact.imag) <= 158 * 2.0 ** -24 * np.abs(e.imag).sum()
    # 64 equal entries and one more: lane 0 holds two of them before the butterfly
    assert sor.gather_sum(np.full(65, 1 + 2j, np.complex64)) == (np.float32(65), np.float32(130))


SEEDS = (9100, 9101, 9102, 9103)
BOUND_HZ = {(10, 30.0): 14.0, (10, 10.0): 66.0, (3, 30.0): 24.0, (3, 10.0): 160.0}     # twice the table's figure


@pytest.mark.parametrize("sps,snr_db", sorted(BOUND_HZ))
def test_estimator_reads_the_offset_of_synthetic_bursts(sps, snr_db):
    """the model on the IQ seam's own input: the capture begins 82 symbols - 1 sample behind the burst's first sample (the last trigger
    symbol's decision instant, tests/test_cpu_oracle.py)"""
    worst = 0.0
    for seed in SEEDS:
        for f in (0.0, 700.0, -1500.0, 3000.0):
            n = 4000 + 1000 + (3374 + 300) * sps
            iq, truth = synth.make_channel_block(n, 1, seed=seed, sps=sps, snr_db=snr_db, first=2000, cfo_hz=f)
            assert len(truth) == 1
            hz, cnt = sor.burst_offset_hz(sor.blocks(iq)[0], truth[0][0] + 82 * sps - 1, sps)
            assert cnt in (3374 * sps // 256, 3374 * sps // 256 - 1)
            worst = max(worst, abs(hz - f))
            assert abs(hz - f) <= BOUND_HZ[(sps, snr_db)], (seed, f, hz)
    print("\n%d samples per symbol, %g dB: worst |estimate - sent| = %.1f Hz (bound %.0f)" % (sps, snr_db, worst, BOUND_HZ[(sps, snr_db)]))
