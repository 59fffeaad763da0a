"""-m gpu: the wideband seam's L / M resampler through the tools -- gr::amps::recc_wideband::make(..., rate_hz, interp, decim_in) behind
recctest's `resample=`, and examples/decode_wideband.py --rate: a 4 Msps stream x 5/4 into the 500 bank, the MINs and lines those of
the binding."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gr_amps_amd import capi

import wbresampleref as wr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SC8 = capi.SAMPLES_SC8


def test_recctest_wide_with_resample(gpu, tmp_path):
    """a 4 Msps sc8 capture file through `recctest wide block.sc8 <chunk> channels=500 resample=4000000:5/4`: the block is made with a
    resampler and pushes of up to 2^22 items, 5/4 as many samples at the bank (its enlarged max_samples_per_push).  The lines of the six
    bursts are those of the binding's records of the same samples"""
    from gr_amps_amd.host import build_host
    from test_gpu_host_blocks import _expected_lines
    b = wr.TOOL_BURSTS["4M@0"]
    x, truth = wr.burst_block("4M@0")
    scale = 100.0 / max(np.abs(x.real).max(), np.abs(x.imag).max())
    q = np.stack([np.rint(x.real * scale), np.rint(x.imag * scale)], axis=1).astype(np.int8)
    p = tmp_path / "block.sc8"
    q.tofile(p)
    tail = np.zeros((64 * 768, 2), np.int8)                       # recctest's own tail of silence, in items of the file
    frames = wr.nout(len(q) + len(tail), b.L, b.M) // b.decim + 72
    with capi.Recc(n_channels=b.C, max_samples=frames, max_bursts=64,
                   wideband={"channels": b.channels, "decim": b.decim, "first_channel": 0, "resample": (b.rate, b.L, b.M)}) as r:
        r.push_wideband_as(q, SC8)
        r.push_wideband_as(tail, SC8)
        recs = r.drain()
    assert sorted(int(c) for c in recs["channel"]) == sorted(b.rows)
    assert sorted(g["min"].decode() for g in recs) == sorted(truth[row][1] for row in b.rows)
    want = []
    for g in recs:
        want.append("MSG channel %d" % int(g["channel"]))
        want += _expected_lines(recs[recs["channel"] == g["channel"]])
    _, exe = build_host()
    out = subprocess.run([exe, "wide", str(p), "777777", "channels=500", "resample=4000000:5/4"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = [l for l in out.stdout.splitlines() if l.startswith("MSG ")]
    assert sorted(got) == sorted(want) and len([l for l in got if l.startswith("MSG channel")]) == 6
    # a ratio the library refuses ends the tool with an error, not with a plain bank
    bad = subprocess.run([exe, "wide", str(p), "777777", "channels=500", "resample=4000000:5/3"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 3 and "resample" in bad.stderr and "MSG " not in bad.stdout


@pytest.mark.parametrize("args,entry", [(["--rate", "4e6", "--channels", "500"], "4e+06 sps x 5/4 into the bank of 500 branches at decimation 125"),
                                        (["--rate", "8e6", "--sc8"], "8e+06 sps x 5/2 into the bank of 2000 branches at decimation 500")],
                         ids=["4M_into_500", "8M_sc8"])
def test_example_decodes_a_resampled_stream(gpu, args, entry):
    """examples/decode_wideband.py --rate: the first plan entry (into the bank asked for, where one is) that keeps the whole band is
    printed and set, twelve mobiles across the band the resampler keeps flat, every burst back with the MIN that was sent and nothing
    else -- no image of a mobile from a bin beyond the delivered band (the script's own exit code)"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "decode_wideband.py")] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith(entry)
    assert "12 bursts sent, 12 decoded" in out.stdout and "MISMATCH" not in out.stdout
