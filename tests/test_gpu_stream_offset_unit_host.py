"""-m gpu: the unit-amplitude carrier offset and the retune through the host blocks and the example -- gr::amps::recc_subband and
gr::amps::recc_fused made with channel_offset = true, offset_unit = true publish the unit statistic's {offset_hz, n_blocks} on their
"offset" port (`recctest sub ... offset unit` / `raw ... offset unit`), their retune() moves the centres in mid-stream (`recctest ...
retune=<sample>:<hz>`), and examples/decode_subband.py --cfo-unit / --afc measure and steer behind the DEFAULT channel filter.

The figures recctest prints are the library's own (amps_recc_burst_offset on the same stream), to the one decimal it prints.  The
bounds of the example against what was SENT are the CPU measurement's worst errors on the example's very stream times 1.5
(scripts/offset_unit_estimator_cpu.py part 4, profiles/stream_offset_unit/estimator_cpu.txt): 11.5 Hz in the first half, 3.5 Hz in the
second, where the centres have been moved and only the mobiles' own offsets are left."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from gr_amps_amd import capi
from gr_amps_amd.host import build_host
from test_gpu_stream_offset_host import CENTRES, FS, _lines, _offset_lines, _stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST_HALF_BOUND_HZ = 1.5 * 11.5
SECOND_HALF_BOUND_HZ = 1.5 * 3.5
CHUNK = 30011


def _library(x, centres, mode, retune=None):
    """records and offsets of the library itself on the stream cut as recctest cuts it; retune = (input sample, Hz)"""
    with capi.Recc(n_channels=len(centres), sps=10, max_samples=x.size // 2, max_bursts=16, stream_offset=mode) as r:
        r.set_xlate_shared(FS, centres, 2)
        for off in range(0, x.size, CHUNK):
            if retune and off >= retune[0]:
                r.retune_xlate([c + retune[1] for c in centres])
                retune = None
            r.push_raw_shared(x[off:off + CHUNK])
        recs = r.drain()
        hz, cnt = r.burst_offset(recs)
    return recs, hz, cnt


def test_recctest_sub_offset_unit_prints_the_unit_statistic(gpu, tmp_path):
    x = _stream()
    p = tmp_path / "two.raw"
    x.tofile(p)
    recs, hz, cnt = _library(x, CENTRES, "unit")
    _, hz_amp, _ = _library(x, CENTRES, True)
    assert [int(g["channel"]) for g in recs] == [0, 1] and cnt.all()
    args = ["sub", str(p), str(CHUNK), "400000", "2", ",".join("%g" % c for c in CENTRES)]
    plain = _lines(args)
    unit = _lines(args + ["offset", "unit"])
    assert plain and [l for l in unit if not l.startswith("MSG offset")] == plain          # the option only adds lines
    got = {c: (f, k) for c, f, k in _offset_lines(unit)}
    assert sorted(got) == [0, 1]
    for g, f_, c in zip(recs, hz, cnt):
        f, k = got[int(g["channel"])]
        assert k == int(c) and abs(f - float(f_)) <= 0.05 + 1e-6, (g["channel"], f, f_)
    # and it is the other statistic: `offset` alone prints the amplitude-weighted figures, which differ
    amp = {c: f for c, f, _ in _offset_lines(_lines(args + ["offset"]))}
    for g, f_ in zip(recs, hz_amp):
        assert abs(amp[int(g["channel"])] - float(f_)) <= 0.05 + 1e-6
    assert all(abs(amp[c] - got[c][0]) > 1.0 for c in got)
    assert _lines(args + ["power", "offset", "unit"]) == _lines(args + ["offset", "unit", "power"])      # with power, in either order


def test_recctest_sub_retune_is_the_librarys_retune(gpu, tmp_path):
    """gr::amps::recc_subband::retune in mid-stream: the records and offsets are those of the library retuned before the same push"""
    x = _stream()
    p = tmp_path / "two.raw"
    x.tofile(p)
    at, move = 2 * CHUNK, 400.0                                      # both bursts are under way: what they read changes
    recs, hz, cnt = _library(x, CENTRES, "unit", retune=(at, move))
    recs0, hz0, _ = _library(x, CENTRES, "unit")
    args = ["sub", str(p), str(CHUNK), "400000", "2", ",".join("%g" % c for c in CENTRES), "offset", "unit"]
    moved = _lines(args + ["retune=%d:%g" % (at, move)])
    got = {c: (f, k) for c, f, k in _offset_lines(moved)}
    assert sorted(got) == sorted(int(g["channel"]) for g in recs)
    for g, f_, c in zip(recs, hz, cnt):
        f, k = got[int(g["channel"])]
        assert k == int(c) and abs(f - float(f_)) <= 0.05 + 1e-6
    still = {c: f for c, f, _ in _offset_lines(_lines(args))}
    for g, f_ in zip(recs0, hz0):
        assert abs(still[int(g["channel"])] - float(f_)) <= 0.05 + 1e-6
    assert any(abs(got[c][0] - still[c]) > 10.0 for c in got if c in still)               # the retune reached the stage
    # a refused retune ends the program with the library's message: the block throws
    _, exe = build_host()
    bad = subprocess.run([exe] + args + ["retune=0:1e9"], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 3 and "retune" in bad.stderr


def test_recctest_raw_offset_unit_and_retune(gpu, tmp_path):
    """gr::amps::recc_fused with offset_unit behind the DEFAULT filter, and its retune(double)"""
    x = _stream()
    p = tmp_path / "two.raw"
    x.tofile(p)

    def library(retune=None):
        with capi.Recc(n_channels=1, sps=10, max_samples=x.size // 2, max_bursts=16, stream_offset="unit") as r:
            r.set_xlate(rate_hz=FS, center_hz=CENTRES[1], decim=2)
            for off in range(0, x.size, CHUNK):
                if retune and off >= retune[0]:
                    r.retune_xlate([CENTRES[1] + retune[1]])
                    retune = None
                r.push_raw(x[None, off:off + CHUNK])
            recs = r.drain()
            return recs, r.burst_offset(recs)

    args = ["raw", str(p), str(CHUNK), "%g" % CENTRES[1], "0", "offset", "unit"]
    seen = []
    for retune in (None, (CHUNK, -300.0)):
        recs, (hz, cnt) = library(retune)
        assert len(recs) == 1 and cnt.all()
        got = _offset_lines(_lines(args + (["retune=%d:%g" % retune] if retune else [])))
        assert len(got) == 1 and got[0][0] == 0 and got[0][2] == int(cnt[0])
        assert abs(got[0][1] - float(hz[0])) <= 0.05 + 1e-6
        seen.append(got[0][1])
    assert abs(seen[0] - seen[1]) > 10.0                             # the retune reached the stage


def _example(flag):
    script = os.path.join(ROOT, "examples", "decode_subband.py")
    p = subprocess.run([sys.executable, script, flag], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "MISMATCH" not in p.stdout
    return p.stdout


def _first_half(out):
    rows = re.findall(r"channel +(\d+)  MIN \d+  sent +([+-]\d+\.\d) Hz  read +([+-]\d+\.\d) Hz  over (\d+) blocks", out)
    assert rows and len({c for c, _, _, _ in rows}) == len(rows)
    for c, sent, read, nb in rows:
        assert float(sent) == 1200.0 + 150.0 * (int(c) % 5 - 2) and int(nb) in (130, 131)
        assert abs(float(read) - float(sent)) <= FIRST_HALF_BOUND_HZ, (c, sent, read)
    m = re.search(r"tuner error \(median of (\d+)\): ([+-]\d+\.\d) Hz", out)
    assert m and int(m.group(1)) == len(rows)
    return rows, float(m.group(2))


def test_the_example_reads_the_offsets_behind_the_default_filter(gpu):
    """examples/decode_subband.py --cfo-unit: every burst that survives the 10 kHz filter reads within the CPU-derived bound of what was
    sent -- with the right sign, where --cfo had to open the filter to 16 kHz"""
    out = _example("--cfo-unit")
    rows, tuner = _first_half(out)
    m = re.search(r"21 bursts sent, (\d+) decoded", out)
    assert m and int(m.group(1)) == len(rows)
    print("\n%d of 21 decoded behind the default filter; tuner error read as %+.1f Hz" % (len(rows), tuner))
    assert len(rows) >= 11                                           # a median of most channels
    if len(rows) == 21:                                              # the median of the 21 sent offsets is the tuner's 1200 Hz
        assert abs(tuner - 1200.0) <= FIRST_HALF_BOUND_HZ


def test_the_example_steers_by_the_measurement(gpu):
    """examples/decode_subband.py --afc: measure, retune every centre by the median, go on: every burst of the second half decodes and
    reads what is left of its offset"""
    out = _example("--afc")
    rows, tuner = _first_half(out)
    m = re.search(r"retuned every centre by ([+-]\d+\.\d) Hz; second half: 21 bursts sent, 21 decoded", out)
    assert m and float(m.group(1)) == tuner
    second = re.findall(r"channel +(\d+)  MIN \d+  left +([+-]\d+\.\d) Hz  read +([+-]\d+\.\d) Hz  over (\d+) blocks of 256 samples  ok", out)
    assert sorted(int(c) for c, _, _, _ in second) == list(range(21))
    for c, left, read, nb in second:
        assert abs(float(left) - (1200.0 + 150.0 * (int(c) % 5 - 2) - tuner)) <= 0.1 and int(nb) in (130, 131)
        assert abs(float(read) - float(left)) <= SECOND_HALF_BOUND_HZ + 0.1, (c, left, read)
    m = re.search(r"residual \(median of 21\): ([+-]\d+\.\d) Hz", out)
    left_median = float(np.median([float(l) for _, l, _, _ in second]))
    assert m and abs(float(m.group(1)) - left_median) <= SECOND_HALF_BOUND_HZ + 0.1
    print("\nretuned by %+.1f Hz; residual %s Hz (the mobiles' own offsets leave %+.1f)" % (tuner, m.group(1), left_median))
