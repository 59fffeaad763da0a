"""-m gpu: received power through the host block -- gr::amps::recc_wideband made with channel_power = true publishes every record's
{mean_power, n_snaps} on its "power" port, and `recctest wide ... power` prints them beside the records.  Without the option the
program's output is what it always was (tests/test_gpu_host_blocks.py reads that)."""
import re
import subprocess

import numpy as np
import pytest

from gr_amps_amd import capi, synth_wideband as sw
from gr_amps_amd.host import build_host

pytestmark = pytest.mark.gpu


def _lines(args):
    _, exe = build_host()
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return [l for l in out.stdout.splitlines() if l.startswith("MSG ")]


def test_recctest_wide_prints_burst_power_beside_each_record(gpu, tmp_path, decim):
    D = decim
    n = int(0.2 * sw.FS_WIDE) // 1536 * 1536
    a, _ = sw.make_wideband(n, [(96 + 7, 30000)], seed=51)
    b, _ = sw.make_wideband(n, [(96 + 500, 60000)], seed=52, snr_db=200.0)
    x = (a + np.float32(0.25) * b).astype(np.complex64)
    p = tmp_path / "band.fc32"
    x.tofile(p)
    with capi.Recc(n_channels=832, sps=1536 // D, max_samples=n // D + 72, max_bursts=64, channel_power=True,
                   wideband={"channels": 1024, "decim": D, "taps_per_branch": 8, "first_channel": 96}) as r:
        r.push_wideband(x)
        r.push_wideband(np.zeros(64 * D, np.complex64))
        recs = r.drain()
        mean, cnt = r.burst_power(recs)
    assert [int(g["channel"]) for g in recs] == [7, 500] and cnt.all()
    plain = _lines(["wide", str(p), "777777", "-1", str(D)])
    withp = _lines(["wide", str(p), "777777", "-1", str(D), "power"])
    assert plain and not [l for l in plain if l.startswith("MSG power")]
    assert [l for l in withp if not l.startswith("MSG power")] == plain          # the option only adds lines
    got = {}
    for l in withp:
        m = re.fullmatch(r"MSG power channel (\d+) (-?\d+\.\d\d) dB n=(\d+)", l)
        if m:
            got[int(m.group(1))] = (float(m.group(2)), int(m.group(3)))
    assert sorted(got) == [7, 500]
    # snapshots do not depend on how the stream was cut into pushes: the block's figures are the library's own
    for g, m_, c in zip(recs, mean, cnt):
        db, k = got[int(g["channel"])]
        assert k == int(c) and abs(db - 10.0 * np.log10(float(m_))) <= 0.005 + 1e-9, (g["channel"], db, m_)
    assert 6.0 < got[7][0] - got[500][0] < 18.0                                  # the second mobile is 12 dB down, give or take the envelope
