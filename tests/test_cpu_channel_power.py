"""not gpu: the received-power feature of the wideband seam (AMPS_RECC_FLAG_CHANNEL_POWER, include/amps_recc.h) as far as it can be
checked without a device -- the declarations, the argument validation, the resources of the snapshot kernel and of the gather kernel
(the one both received-power flags share), and the float64 model
tests/powerref.py that the GPU tests compare against."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest

import powerref
from oracle import channelizer as cz
from gr_amps_amd import build, capi, synth_wideband as sw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_points_and_the_flag():
    hdr = open(os.path.join(ROOT, "include", "amps_recc.h")).read()
    assert re.search(r"#define\s+AMPS_RECC_FLAG_CHANNEL_POWER\s+0x200u", hdr)
    assert re.search(r"#define\s+AMPS_RECC_POWER_STRIDE\s+256\b", hdr)
    assert re.search(r"#define\s+AMPS_RECC_ABI_VERSION\s+4\b", hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int\s+amps_recc_channel_power\(amps_recc_t \*h, uint64_t first_snap, size_t n, float \*out, size_t out_ld,\s*"
                     r"uint32_t \*rows, uint64_t \*produced_snaps\);", code)
    assert re.search(r"int\s+amps_recc_burst_power\(amps_recc_t \*h, const amps_recc_burst_t \*recs, size_t n, float \*mean_power, "
                     r"uint32_t \*n_snaps\);", code)
    assert re.search(r"uint32_t\s+amps_recc_power_ring_snaps\(const amps_recc_t \*h\);", code)
    assert capi.FLAG_CHANNEL_POWER == 0x200 and capi.POWER_STRIDE == powerref.STRIDE == 256
    for name in ("amps_recc_channel_power", "amps_recc_burst_power", "amps_recc_power_ring_snaps"):
        assert name in capi.EXPORTS


def test_entry_points_validate_without_a_device():
    L = capi.load()
    assert L.amps_recc_abi_version() == 4
    out, cnt = (C.c_float * 4)(), (C.c_uint32 * 4)()
    recs = np.zeros(4, capi.BURST_DTYPE)
    assert L.amps_recc_channel_power(None, 0, 0, None, 0, None, None) == -22          # -EINVAL: no handle, whatever the rest
    assert L.amps_recc_channel_power(None, 0, 4, out, 4, None, None) == -22
    assert L.amps_recc_burst_power(None, None, 0, None, None) == -22
    assert L.amps_recc_burst_power(None, recs.ctypes.data_as(C.c_void_p), 4, out, cnt) == -22
    assert L.amps_recc_power_ring_snaps(None) == 0


@pytest.fixture(scope="module")
def res():
    if not os.path.exists(build.hipcc()) or not shutil.which("c++filt"):
        if os.path.exists(build.RESOURCES):
            import json
            with open(build.RESOURCES) as f:
                return json.load(f)
        pytest.skip("hipcc / c++filt not installed and no cached kernel_resources.json")
    return build.kernel_resources()


def test_power_kernels_need_no_scratch_and_little_lds(res):
    snap = {k: v for k, v in res.items() if "amps::chz_power_kernel<" in k}
    assert len(snap) == 4, sorted(snap)                               # fc32 and sc16 blocks at either decimation
    gather = {k: v for k, v in res.items() if "amps::power_ring_gather_kernel(" in k}
    assert len(gather) == 1, sorted(gather)
    for name, r in {**snap, **gather}.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["lds_bytes"] <= 24 * 1024, (name, r)
    # the names do not collide with the prefixes other tests count instantiations by
    for name in list(snap) + list(gather):
        assert not re.search(r"amps::(chz12_kernel|recc_front_kernel|recc_resolve_kernel)<", name), name
    for name in gather:
        assert not re.search(r"amps::(chz_power_kernel<|stream_power_kernel\()", name), name


@pytest.mark.parametrize("D", [512, 768])
def test_model_snapshots_are_the_channelizer_frames(D):
    rng = np.random.default_rng(5)
    n = 600 * D + 77
    x = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    y = cz.channelize(x, P=8, D=D, first_bin=900, n_channels=300)     # wraps past bin 1023
    want = np.abs(y[:, ::256]) ** 2
    got = powerref.snapshots(x, D, 900, 300)
    assert got.shape == want.shape == (300, 3)
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12 * want.max())
    # an origin shifts which frames are snapshots: s = origin + m
    got = powerref.snapshots(x, D, 900, 300, origin=64 * 3)
    want = np.abs(y[:, 64::256]) ** 2
    assert powerref.first_snapshot(64 * 3) == 1 and got.shape == want.shape == (300, 3)
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12 * want.max())


@pytest.mark.parametrize("D", [512, 768])
def test_carrier_at_a_channel_centre_reads_its_amplitude_squared(D):
    n = 1100 * D
    x = 0.5 * np.exp(2j * np.pi * sw.bin_freq(100) * np.arange(n) / sw.FS_WIDE)
    P = powerref.snapshots(x, D, 0, 1024)
    assert P.shape == (1024, 5)
    assert np.all(np.abs(P[100, 1:] - 0.25) <= 1e-9 * 0.25), P[100]   # unit DC gain; snapshot 0 still sees the zeros before the stream
    assert P[100, 0] < 0.01 and np.delete(P[:, 1:], 100, axis=0).max() < 1e-6


@pytest.mark.parametrize("sps,counts", [(2, {26, 27}), (3, {39, 40})])
def test_burst_mean_counts(sps, counts):
    P = np.arange(64, dtype=np.float64)
    seen = set()
    for pos in range(256):
        mean, cnt = powerref.burst_mean(P, pos, sps)
        j0 = -(-pos // 256)
        assert cnt == (pos + 3374 * sps) // 256 - j0 + 1 and cnt in counts
        assert mean == np.mean(P[j0:j0 + cnt])
        seen.add(cnt)
    assert seen == counts
    # a capture that reaches past what is held: no count, no power
    assert powerref.burst_mean(P[:20], 0, sps) == (0.0, 0)
    assert powerref.burst_mean(P, 0, sps, first=1) == (0.0, 0)
    assert powerref.burst_mean(P[2:], 2 * 256, sps, first=2) == (float(np.mean(P[2:2 + max(counts)])), max(counts))
