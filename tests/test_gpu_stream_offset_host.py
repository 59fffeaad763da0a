"""-m gpu: the carrier offset of the translate seams through the host blocks -- gr::amps::recc_subband and gr::amps::recc_fused made with
channel_offset = true publish every record's {offset_hz, n_blocks} on their "offset" port, `recctest sub ... offset` / `recctest raw ...
power offset` print them beside the records, and examples/decode_subband.py --cfo reads the tuner's error off 21 mobiles.  Without the
option the program's output is what it always was (tests/test_gpu_host_blocks.py, tests/test_gpu_xlate_shared.py and
tests/test_gpu_stream_power_host.py read that).

The figures recctest prints are the library's own (amps_recc_burst_offset on the same stream), to the one decimal it prints.  The bound
of the example against what was SENT is the CPU measurement's worst error on the example's very stream, 232 Hz, times 1.5
(scripts/offset_estimator_cpu.py part 3, DESIGN.md 4.7g: 21 adjacent channels, bursts overlapping in time, cut-off 16 kHz)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from gr_amps_amd import capi, synth
from gr_amps_amd.host import build_host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS = 400e3
CENTRES = [-100e3, 130e3]
OFFSETS = [600.0, -900.0]
EXAMPLE_BOUND_HZ = 1.5 * 232.2


def _lines(args):
    _, exe = build_host()
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return [l for l in out.stdout.splitlines() if l.startswith("MSG ")]


def _offset_lines(lines):
    got = []
    for l in lines:
        m = re.fullmatch(r"MSG offset channel (\d+) (-?\d+\.\d) Hz n=(\d+)", l)
        if m:
            got.append((int(m.group(1)), float(m.group(2)), int(m.group(3))))
    return got


def _stream():
    """two mobiles in a quarter of a second of a 400 ksps stream, each off its centre by its own amount, their bursts overlapping in time"""
    n = 100000
    k = np.arange(n)
    x = np.zeros(n, np.complex128)
    for c, (fc, f) in enumerate(zip(CENTRES, OFFSETS)):
        iq, truth = synth.make_channel_block(n, 1, seed=61 + c, sps=20, snr_db=40.0, first=4000 + 9000 * c, cfo_hz=f)
        assert len(truth) == 1
        x += iq * np.exp(2j * np.pi * fc * k / FS)
    return x.astype(np.complex64)


def test_recctest_sub_prints_the_offset_beside_each_record(gpu, tmp_path):
    x = _stream()
    p = tmp_path / "two.raw"
    x.tofile(p)
    with capi.Recc(n_channels=2, sps=10, max_samples=x.size // 2, max_bursts=16, stream_offset=True) as r:
        r.set_xlate_shared(FS, CENTRES, 2)
        r.push_raw_shared(x)
        recs = r.drain()
        hz, cnt = r.burst_offset(recs)
    assert [int(g["channel"]) for g in recs] == [0, 1] and cnt.all()
    args = ["sub", str(p), "30011", "400000", "2", ",".join("%g" % c for c in CENTRES)]
    plain = _lines(args)
    witho = _lines(args + ["offset"])
    assert plain and not _offset_lines(plain)
    assert [l for l in witho if not l.startswith("MSG offset")] == plain          # the option only adds lines
    got = _offset_lines(witho)
    assert sorted(c for c, _, _ in got) == [0, 1]                                 # one line per burst
    # the block's "offset" messages follow their records: each line stands behind its channel's lines and before the next channel's
    order = [("record", l.split()[2]) if l.startswith("MSG channel ") else ("offset", l.split()[3])
             for l in witho if l.startswith("MSG channel ") or l.startswith("MSG offset channel ")]
    assert [k for k, _ in order] == ["record", "offset"] * 2 and order[0][1] == order[1][1] and order[2][1] == order[3][1]
    # blocks do not depend on how the stream was cut into pushes: the block's figures are the library's own
    by = {c: (f, k) for c, f, k in got}
    for g, f_, c in zip(recs, hz, cnt):
        f, k = by[int(g["channel"])]
        assert k == int(c) and k in (130, 131)
        assert abs(f - float(f_)) <= 0.05 + 1e-6, (g["channel"], f, f_)
    # both options, in either order: the power lines of `... power` and the offset lines above, nothing else new
    withp = _lines(args + ["power"])
    for both in (_lines(args + ["power", "offset"]), _lines(args + ["offset", "power"])):
        assert [l for l in both if not l.startswith("MSG offset")] == withp
        assert [l for l in both if not l.startswith("MSG power")] == witho


def test_recctest_raw_prints_power_and_offset_of_the_one_channel(gpu, tmp_path):
    """gr::amps::recc_fused with channel_power and channel_offset, the channel filter opened to 16 kHz: the one-channel translate seam"""
    x = _stream()
    p = tmp_path / "two.raw"
    x.tofile(p)
    with capi.Recc(n_channels=1, sps=10, max_samples=x.size // 2, max_bursts=16, stream_power=True, stream_offset=True) as r:
        r.set_xlate(rate_hz=FS, center_hz=CENTRES[1], decim=2, cutoff_hz=16e3)
        r.push_raw(x[None, :])
        recs = r.drain()
        mean, pcnt = r.burst_power(recs)
        hz, cnt = r.burst_offset(recs)
    assert len(recs) == 1 and cnt.all() and pcnt.all()
    args = ["raw", str(p), "30011", "%g" % CENTRES[1], "16000"]
    plain = _lines(args)
    both = _lines(args + ["power", "offset"])
    assert plain and not _offset_lines(plain)
    assert [l for l in both if not l.startswith("MSG power") and not l.startswith("MSG offset")] == plain
    got = _offset_lines(both)
    assert len(got) == 1 and got[0][0] == 0 and got[0][2] == int(cnt[0])
    assert abs(got[0][1] - float(hz[0])) <= 0.05 + 1e-6
    m = [re.fullmatch(r"MSG power channel 0 (-?\d+\.\d\d) dB n=(\d+)", l) for l in both if l.startswith("MSG power")]
    assert len(m) == 1 and m[0] and abs(float(m[0].group(1)) - 10.0 * np.log10(float(mean[0]))) <= 0.005 + 1e-9
    assert _lines(args + ["offset", "power"]) == both                             # either order


def test_the_example_reads_every_mobiles_offset_and_the_tuner_error(gpu):
    """examples/decode_subband.py --cfo: the tuner +1200 Hz off, every mobile up to 300 Hz on its own, the channel filter at 16 kHz"""
    script = os.path.join(ROOT, "examples", "decode_subband.py")
    p = subprocess.run([sys.executable, script, "--cfo"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "21 bursts sent, 21 decoded" in p.stdout and "MISMATCH" not in p.stdout
    rows = re.findall(r"channel +(\d+)  MIN \d+  sent +([+-]\d+\.\d) Hz  read +([+-]\d+\.\d) Hz  over (\d+) blocks", p.stdout)
    assert sorted(int(c) for c, _, _, _ in rows) == list(range(21))
    for c, sent, read, nb in rows:
        assert float(sent) == 1200.0 + 150.0 * (int(c) % 5 - 2) and int(nb) in (130, 131)
        assert abs(float(read) - float(sent)) <= EXAMPLE_BOUND_HZ, (c, sent, read)
    m = re.search(r"tuner error \(median of 21\): ([+-]\d+\.\d) Hz", p.stdout)
    assert m and abs(float(m.group(1)) - 1200.0) <= EXAMPLE_BOUND_HZ
