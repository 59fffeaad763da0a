"""-m gpu: the "seizures" port of the host blocks through `recctest sub ... seizures` (gr::amps::recc_subband made with
seizure_events = true): for a one-burst file the event's line comes in front of the record's lines, with the record's channel and
position, and is what the binding drains for the same pushes; without the argument the output is what it was."""
import re
import subprocess

import numpy as np
import pytest

from gr_amps_amd import capi, synth
from gr_amps_amd.host import build_host

pytestmark = pytest.mark.gpu
FS, CENTRES, CHUNK = 400e3, (-60e3, 90e3), 16384


def _one_burst_file():
    n = 120000
    iq, _ = synth.make_channel_block(n, 1, seed=8100, sps=20, first=9000)
    x = (iq * np.exp(2j * np.pi * CENTRES[1] * np.arange(n) / FS)).astype(np.complex64)
    return x


def test_recctest_sub_prints_the_event_in_front_of_its_record(gpu, tmp_path):
    x = _one_burst_file()
    p = tmp_path / "one.raw"
    x.tofile(p)
    with capi.Recc(n_channels=2, sps=10, max_samples=x.size // 2, max_bursts=16, seizure_events=True) as r:
        r.set_xlate_shared(FS, CENTRES, 2)
        ev, recs = [], []
        for o in range(0, x.size, CHUNK):
            r.push_raw_shared(x[o:o + CHUNK])
            ev.append(r.drain_seizures())
            recs.append(r.drain())
    ev, recs = np.concatenate(ev), np.concatenate(recs)
    assert len(ev) == 1 and len(recs) == 1 and int(recs[0]["channel"]) == 1
    assert (int(ev[0]["channel"]), int(ev[0]["position"])) == (1, int(recs[0]["position"]))
    _, exe = build_host()
    args = [exe, "sub", str(p), str(CHUNK), "%g" % FS, "2", ",".join("%g" % c for c in CENTRES)]
    out = subprocess.run(args + ["seizures"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [l for l in out.stdout.splitlines() if l.startswith("MSG ")]
    e = ev[0]
    dcc = "".join(str(int(b)) for b in e["dcc"]) if int(e["flags"]) & capi.SEIZURE_FLAG_DCC_COMPLETE else "-"
    want = "MSG seizure channel 1 position %d found_at %d dcc %s bad %d" % (int(e["position"]), int(e["found_at"]), dcc, int(e["dcc_bad"]))
    assert [l for l in lines if l.startswith("MSG seizure")] == [want]
    assert lines.index(want) < lines.index("MSG channel 1")                              # the event in front of the record's lines
    m = re.fullmatch(r"MSG seizure channel (\d+) position (\d+) found_at (\d+) dcc ([01]{7}|-) bad (\d+)", want)
    assert m and (int(m.group(1)), int(m.group(2))) == (int(recs[0]["channel"]), int(recs[0]["position"]))
    plain = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0, plain.stderr
    assert [l for l in plain.stdout.splitlines() if l.startswith("MSG ")] == [l for l in lines if l != want]
