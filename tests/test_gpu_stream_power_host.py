"""-m gpu: received power of the translate and IQ seams through the host blocks -- gr::amps::recc_subband and gr::amps::recc_fused made
with channel_power = true publish every record's {mean_power, n_snaps} on their "power" port, and `recctest sub ... power` /
`recctest raw ... power` print them beside the records.  Without the option the program's output is what it always was
(tests/test_gpu_host_blocks.py and tests/test_gpu_xlate_shared.py read that)."""
import re
import subprocess

import numpy as np
import pytest

from gr_amps_amd import capi, synth
from gr_amps_amd.host import build_host

pytestmark = pytest.mark.gpu

FS = 400e3
CENTRES = [-100e3, 130e3]
AMPS = [1.0, 0.25]                                                   # the second mobile 12 dB down


def _lines(args):
    _, exe = build_host()
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return [l for l in out.stdout.splitlines() if l.startswith("MSG ")]


def _power_lines(lines):
    got = []
    for l in lines:
        m = re.fullmatch(r"MSG power channel (\d+) (-?\d+\.\d\d) dB n=(\d+)", l)
        if m:
            got.append((int(m.group(1)), float(m.group(2)), int(m.group(3))))
    return got


def _stream():
    """two mobiles in a quarter of a second of a 400 ksps stream, their bursts overlapping in time"""
    n = 100000
    k = np.arange(n)
    x = np.zeros(n, np.complex128)
    for c, (fc, a) in enumerate(zip(CENTRES, AMPS)):
        iq, truth = synth.make_channel_block(n, 1, seed=61 + c, sps=20, snr_db=40.0, first=4000 + 9000 * c)
        assert len(truth) == 1
        x += a * iq * np.exp(2j * np.pi * fc * k / FS)
    return x.astype(np.complex64)


def test_recctest_sub_prints_burst_power_beside_each_record(gpu, tmp_path):
    x = _stream()
    p = tmp_path / "two.raw"
    x.tofile(p)
    with capi.Recc(n_channels=2, sps=10, max_samples=x.size // 2, max_bursts=16, stream_power=True) as r:
        r.set_xlate_shared(FS, CENTRES, 2)
        r.push_raw_shared(x)
        recs = r.drain()
        mean, cnt = r.burst_power(recs)
    assert [int(g["channel"]) for g in recs] == [0, 1] and cnt.all()
    args = ["sub", str(p), "30011", "400000", "2", ",".join("%g" % c for c in CENTRES)]
    plain = _lines(args)
    withp = _lines(args + ["power"])
    assert plain and not _power_lines(plain)
    assert [l for l in withp if not l.startswith("MSG power")] == plain          # the option only adds lines
    got = _power_lines(withp)
    assert sorted(c for c, _, _ in got) == [0, 1]                                 # one line per burst
    # the block's "power" messages follow their records: each line stands behind its channel's lines and before the next channel's
    order = [("record", l.split()[2]) if l.startswith("MSG channel ") else ("power", l.split()[3])
             for l in withp if l.startswith("MSG channel ") or l.startswith("MSG power channel ")]
    assert [k for k, _ in order] == ["record", "power"] * 2 and order[0][1] == order[1][1] and order[2][1] == order[3][1]
    # blocks do not depend on how the stream was cut into pushes: the block's figures are the library's own
    by = {c: (db, k) for c, db, k in got}
    for g, m_, c in zip(recs, mean, cnt):
        db, k = by[int(g["channel"])]
        assert k == int(c) and k in (130, 131)
        assert abs(db - 10.0 * np.log10(float(m_))) <= 0.005 + 1e-9, (g["channel"], db, m_)
    assert 10.0 < by[0][0] - by[1][0] < 14.0                                      # the second mobile is 12 dB down


def test_recctest_raw_prints_burst_power_of_the_one_channel(gpu, tmp_path):
    """gr::amps::recc_fused with channel_power = true: the one-channel translate seam"""
    x = _stream()
    p = tmp_path / "two.raw"
    x.tofile(p)
    with capi.Recc(n_channels=1, sps=10, max_samples=x.size // 2, max_bursts=16, stream_power=True) as r:
        r.set_xlate(rate_hz=FS, center_hz=CENTRES[1], decim=2)
        r.push_raw(x[None, :])
        recs = r.drain()
        mean, cnt = r.burst_power(recs)
    assert len(recs) == 1 and cnt.all()
    args = ["raw", str(p), "30011", "%g" % CENTRES[1]]
    plain = _lines(args)
    withp = _lines(args + ["power"])
    assert plain and not _power_lines(plain)
    assert [l for l in withp if not l.startswith("MSG power")] == plain
    got = _power_lines(withp)
    assert len(got) == 1 and got[0][0] == 0 and got[0][2] == int(cnt[0])
    assert abs(got[0][1] - 10.0 * np.log10(float(mean[0]))) <= 0.005 + 1e-9
