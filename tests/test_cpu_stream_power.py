"""not gpu: received power of the IQ and translate seams (AMPS_RECC_FLAG_STREAM_POWER, include/amps_recc.h) as far as it can be
checked without a device -- the flag in the header and the binding, the resources of the block kernel and of the gather
kernel (the one both received-power flags share), and the float64 model
tests/streampowerref.py that the GPU tests compare against."""
import inspect
import os
import re
import shutil

import numpy as np
import pytest

import streampowerref as spr
from gr_amps_amd import build, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (3, 4, 5, 6, 8, 10, 12)                                      # the streaming kernel's samples per symbol (front_kernel_for)


def test_header_has_the_flag_and_the_abi_version_stands():
    hdr = open(os.path.join(ROOT, "include", "amps_recc.h")).read()
    assert re.search(r"#define\s+AMPS_RECC_FLAG_STREAM_POWER\s+0x400u", hdr)
    assert re.search(r"#define\s+AMPS_RECC_FLAG_CHANNEL_POWER\s+0x200u", hdr)
    assert re.search(r"#define\s+AMPS_RECC_ABI_VERSION\s+4\b", hdr)
    assert re.search(r"#define\s+AMPS_RECC_POWER_STRIDE\s+256\b", hdr)
    # no other flag has the bit
    flags = re.findall(r"#define\s+(AMPS_RECC_FLAG_\w+)\s+(0x[0-9a-fA-F]+)u", hdr)
    assert [n for n, v in flags if int(v, 16) & 0x400] == ["AMPS_RECC_FLAG_STREAM_POWER"]


def test_binding_has_the_flag_and_the_argument():
    assert capi.FLAG_STREAM_POWER == 0x400
    assert capi.POWER_STRIDE == spr.STRIDE == 256
    p = inspect.signature(capi.Recc.__init__).parameters
    assert "stream_power" in p and p["stream_power"].default is False
    assert capi.load().amps_recc_abi_version() == 4


@pytest.fixture(scope="module")
def res():
    if not os.path.exists(build.hipcc()) or not shutil.which("c++filt"):
        if os.path.exists(build.RESOURCES):
            import json
            with open(build.RESOURCES) as f:
                return json.load(f)
        pytest.skip("hipcc / c++filt not installed and no cached kernel_resources.json")
    return build.kernel_resources()


def test_stream_power_kernels_need_no_scratch_and_no_lds(res):
    block = {k: v for k, v in res.items() if "amps::stream_power_kernel(" in k}
    gather = {k: v for k, v in res.items() if "amps::power_ring_gather_kernel(" in k}
    assert len(block) == 1 and len(gather) == 1, (sorted(block), sorted(gather))
    for name, r in {**block, **gather}.items():
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
    assert list(block.values())[0]["lds_bytes"] == 0
    assert list(gather.values())[0]["lds_bytes"] <= 24 * 1024
    # the names do not collide with the prefixes other tests count instantiations by
    for name in list(block) + list(gather):
        assert not re.search(r"amps::(chz12_kernel<|recc_front_kernel<|recc_resolve_kernel<|chz_power_kernel<)", name), name
    for name in gather:
        assert "amps::stream_power_kernel(" not in name, name


def test_model_constant_amplitude_tone_reads_its_amplitude_squared():
    a = 0.37
    n = 256 * 9 + 100
    y = a * np.exp(2j * np.pi * 0.0123 * np.arange(n))
    P = spr.blocks(y)
    assert P.shape == (1, 9)
    assert np.all(np.abs(P - a * a) <= 1e-12 * a * a)
    # an origin moves the block edges: s = origin + m, and a block that would begin before the origin does not exist
    origin = 64 * 15
    y2 = np.arange(n) + 0j
    P2 = spr.blocks(y2, origin=origin)
    assert spr.first_block(origin) == 4 and P2.shape == (1, 9)       # n - 64 = 9 * 256 + 36
    m = np.arange(64, 64 + 256, dtype=np.float64)                    # block 4 = samples m = 1024 - 960 ... of the stream
    assert abs(P2[0, 0] - np.mean(m * m)) <= 1e-9 * P2[0, 0]
    assert spr.blocks(np.zeros(255, complex)).shape == (1, 0)
    assert spr.blocks(np.ones((3, 512), complex)).shape == (3, 2)


@pytest.mark.parametrize("sps,counts", [(3, {38, 39}), (4, {51, 52}), (5, {64, 65}), (6, {78, 79}), (8, {104, 105}), (10, {130, 131}),
                                        (12, {157, 158})])
def test_burst_mean_counts(sps, counts):
    """n_snaps = floor((pos + 3374 sps) / 256) - ceil(pos / 256) at every residue of the position: floor(3374 sps / 256) or one less"""
    assert sps in RATES and max(counts) == 3374 * sps // 256 and min(counts) == max(counts) - 1
    row = np.arange(200, dtype=np.float64) ** 2
    seen = set()
    for pos in range(256, 512):                                      # every residue mod 256
        mean, cnt = spr.burst_mean(row, pos, sps)
        j0 = -(-pos // 256)
        assert (j0, cnt) == spr.burst_window(pos, sps)
        assert cnt == (pos + 3374 * sps) // 256 - j0 and cnt in counts
        assert 256 * j0 >= pos and 256 * (j0 + cnt) <= pos + 3374 * sps < 256 * (j0 + cnt + 1)   # wholly inside, and no more fit
        assert mean == np.mean(row[j0:j0 + cnt])
        seen.add(cnt)
    assert seen == counts


def test_burst_mean_outside_the_held_window_is_nothing():
    row = np.arange(200, dtype=np.float64)
    for sps in RATES:
        _, cnt = spr.burst_window(0, sps)
        assert spr.burst_mean(row[:cnt - 1], 0, sps) == (0.0, 0)     # the last block is not produced yet
        assert spr.burst_mean(row, 0, sps, first=1) == (0.0, 0)      # the first block has left the window
        assert spr.burst_mean(row[2:], 2 * 256, sps, first=2) == (float(np.mean(row[2:2 + cnt])), cnt)
