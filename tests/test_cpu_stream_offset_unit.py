"""not gpu: the unit-amplitude carrier-offset statistic (AMPS_RECC_FLAG_STREAM_OFFSET_UNIT) and amps_recc_retune_xlate as far as they can
be checked without a device -- the flag and the entry point in the header and the binding, the new kernel's resources, the float64
model tests/streamoffsetunitref.py against hand cases, the estimator on synthetic bursts and behind the default channel filter, and
the retune argument checks in a stand-alone host program under the address and undefined-behaviour sanitizers.

The estimator's bounds: the figures of profiles/stream_offset_unit/estimator_cpu.txt (scripts/offset_unit_estimator_cpu.py), rounded
up to the next hertz.  The GPU tests bound the device by these times 1.5 and never by what the device gives."""
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import streamoffsetref as sor
import streamoffsetunitref as sur
from gr_amps_amd import build, capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def test_header_has_the_flag_and_the_entry_point_and_the_abi_version_stands():
    hdr = open(os.path.join(ROOT, "include", "amps_recc.h")).read()
    assert re.search(r"#define\s+AMPS_RECC_FLAG_STREAM_OFFSET_UNIT\s+0x1000u", hdr)
    assert re.search(r"#define\s+AMPS_RECC_ABI_VERSION\s+4\b", hdr)
    flags = re.findall(r"#define\s+(AMPS_RECC_FLAG_\w+)\s+(0x[0-9a-fA-F]+)u", hdr)
    assert [n for n, v in flags if int(v, 16) & 0x1000] == ["AMPS_RECC_FLAG_STREAM_OFFSET_UNIT"]
    assert max(int(v, 16) for _, v in flags) == 0x1000 and len({int(v, 16) for _, v in flags}) == len(flags)   # the next free bit
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+amps_recc_retune_xlate\s*\(amps_recc_t \*h, const double \*center_hz, size_t n\)", code)
    for word in ("v_rsq_f32", "261 * 2^-24", "COHERENCE", "2048 channel-rate samples"):
        assert word in hdr, word


def test_binding_has_the_flag_the_keyword_value_and_retune():
    assert capi.FLAG_STREAM_OFFSET_UNIT == 0x1000
    p = inspect.signature(capi.Recc.__init__).parameters
    assert p["stream_offset"].default is False
    with pytest.raises(ValueError):
        capi.Recc(n_channels=1, sps=10, max_samples=64, stream_offset="amp")      # refused before any device is touched
    L = capi.load()
    assert L.amps_recc_abi_version() == 4
    assert "amps_recc_retune_xlate" in capi.EXPORTS and callable(capi.Recc.retune_xlate)
    assert L.amps_recc_retune_xlate(None, None, 0) == -22


@pytest.fixture(scope="module")
def res():
    if not os.path.exists(build.hipcc()) or not shutil.which("c++filt"):
        if os.path.exists(build.RESOURCES):
            import json
            with open(build.RESOURCES) as f:
                return json.load(f)
        pytest.skip("hipcc / c++filt not installed and no cached kernel_resources.json")
    return build.kernel_resources()


def test_unit_kernel_needs_no_scratch_and_no_lds(res):
    unit = {k: v for k, v in res.items() if "amps::stream_unit_autocorr_kernel(" in k}
    assert len(unit) == 1, sorted(unit)
    for name, r in unit.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["lds_bytes"] == 0, (name, r)
    assert len([k for k in res if "amps::stream_autocorr_kernel(" in k]) == 1       # its sibling under its own name
    assert len([k for k in res if "amps::xlate_steps_store_kernel(" in k]) == 1


def test_model_hand_cases():
    f, fs = 1234.0, 200e3
    n = 256 * 4 + 100
    full = np.exp(2j * np.pi * f / fs)
    # a carrier: unit amplitude whatever the carrier's
    for a in (0.37, 1e-15, 3e15):
        Ublk = sur.blocks((a * np.exp(2j * np.pi * f * np.arange(n) / fs)).astype(np.complex64))
        assert Ublk.shape == (1, 4) and Ublk.dtype == np.complex128
        assert np.all(np.abs(Ublk[0, 1:] - full) <= 2e-6), a       # the samples are rounded to fp32: 2 u of phase per product
        # the zero in front of the stream: a zero TERM, still divided by 2^8
        assert abs(Ublk[0, 0] - full * 255.0 / 256.0) <= 2e-6
    y = (0.5 * np.exp(2j * np.pi * f * np.arange(n) / fs)).astype(np.complex64)
    # an origin inside a block: no zero term in the first whole block; at a block edge: one
    assert np.all(np.abs(sur.blocks(y, origin=960) - full) <= 2e-6)
    assert abs(sur.blocks(y, origin=1024)[0, 0] - full * 255.0 / 256.0) <= 2e-6
    # an all-zero block reads exactly zero, and its neighbour loses the one product with the last zero
    z = y.copy()
    z[256:512] = 0
    Z = sur.blocks(z)
    assert Z[0, 1] == 0 and abs(Z[0, 2] - full * 255.0 / 256.0) <= 2e-6 and abs(Z[0, 3] - full) <= 2e-6
    # a sample that is not finite takes out the two products it is part of; the divisor stays 2^8
    for bad in (complex(np.inf, 0), complex(0, np.nan), complex(-np.inf, np.nan)):
        w = y.copy()
        w[600] = bad
        u = sur.units(w)[0]
        assert u[600] == 0 and u[601] == 0 and abs(abs(u[599]) - 1) < 1e-12 and abs(abs(u[602]) - 1) < 1e-12
        W = sur.blocks(w)
        assert np.isfinite(W.real).all() and abs(W[0, 2] - full * 254.0 / 256.0) <= 2e-6
    # finite samples whose product is not: judged as the device judges, on the fp32 product
    w = y.copy()
    w[600:602] = np.complex64(complex(3e38, 3e38))
    assert sur.units(w)[0][601] == 0
    # u is a unit vector: one sample, hand value
    assert abs(sur.units(np.array([1 + 0j, 3 + 4j], np.complex64))[0][1] - (0.6 + 0.8j)) < 1e-15
    assert sur.coherence(3 + 4j, 10) == 0.5 and sur.coherence(0j, 0) == 0.0


SEEDS = (9100, 9101, 9102, 9103)
# the IQ-seam table of estimator_cpu.txt: the unit statistic's worst error over these seeds and offsets
TABLE_HZ = {(10, 30.0): 2.0, (10, 10.0): 8.0, (3, 30.0): 6.0, (3, 10.0): 21.0}


@pytest.mark.parametrize("sps,snr_db", sorted(TABLE_HZ))
def test_estimator_reads_the_offset_of_synthetic_bursts_better_than_the_shipped_one(sps, snr_db):
    worst = {"amp": 0.0, "unit": 0.0}
    for seed in SEEDS:
        for f in (0.0, 700.0, -1500.0, 3000.0):
            n = 4000 + 1000 + (3374 + 300) * sps
            iq, truth = synth.make_channel_block(n, 1, seed=seed, sps=sps, snr_db=snr_db, first=2000, cfo_hz=f)
            pos = truth[0][0] + 82 * sps - 1
            for k, m in (("amp", sor), ("unit", sur)):
                hz, cnt = m.burst_offset_hz(m.blocks(iq)[0], pos, sps)
                assert cnt > 0
                worst[k] = max(worst[k], abs(hz - f))
    print("\n%d samples per symbol, %g dB: worst |estimate - sent| shipped %.1f Hz, unit %.1f Hz" % (sps, snr_db, worst["amp"], worst["unit"]))
    assert worst["unit"] <= TABLE_HZ[(sps, snr_db)] + 0.5            # the table prints whole hertz
    assert worst["unit"] < worst["amp"]


def test_model_reads_the_offset_behind_the_default_filter_where_the_shipped_statistic_has_the_wrong_sign():
    """THE assertion: 2.4 Msps / 12 behind the default 10 kHz cut-off, +1500 Hz at 30 dB.  The GPU test's bound is this one times 1.5."""
    import offset_unit_estimator_cpu as est
    got = est.filter_estimates("2400k_d12", 30.0, 1500.0)
    print("\nshipped %+.1f Hz, unit %+.1f Hz" % (got["amp"], got["unit"]))
    assert abs(got["unit"] - 1500.0) <= 5.0                          # test_gpu_stream_offset_unit.FILTER_UNIT_ERR_HZ
    assert abs(got["amp"] - (-475.0)) <= 1.0


def test_committed_estimator_table_is_the_scripts():
    """profiles/stream_offset_unit/estimator_cpu.txt holds the point above as the script prints it"""
    txt = open(os.path.join(ROOT, "profiles", "stream_offset_unit", "estimator_cpu.txt")).read()
    assert "| +700 | -417 / -438 | +699 / +698 | +701 / +701 | +703 / +702 |" in txt
    assert "shipped -475.2 Hz, unit +1495.2 Hz" in txt


def test_retune_argument_checks_stand_alone_under_sanitizers(tmp_path):
    """gr_amps_amd/csrc/recc_xlate_steps.h is free of HIP: tests/xlate_steps_host.cc has its own main, is compiled with
    -fsanitize=address,undefined and run as a program of its own"""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "xlate_steps_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "gr_amps_amd", "csrc"),
                    os.path.join(ROOT, "tests", "xlate_steps_host.cc"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "xlate steps ok" in out
