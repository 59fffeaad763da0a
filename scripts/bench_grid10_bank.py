"""What the filter banks of 10 kHz bins cost: the wideband seam at M = 2500, 2000, 1000, 500 branches (25, 20, 10, 5 Msps), D = M / 4, on
fc32, sc16 and sc8 blocks (the same noise in each format), every admissible channel active (M / 3 of them), beside the narrow bank of
512 branches at D = 384 as the yardstick per input sample -- all in ONE process, because boxes differ by up to 12 %.

Per size one second of stream (M x 10 000 samples, rounded up to whole pushes) is pushed from a device-resident block of 2^22 samples
of noise, spec D.  Times come from amps_recc_get_timing in timing mode "all": ms_channelizer is the filter-bank kernel, the step is the
sum of every kernel the push launches (filter bank, streaming kernel, resolve, carry, decode).  The legs alternate: yardstick, then per
size fc32, sc16, sc8, yardstick again, `rounds` times; the table holds each leg's median over the rounds.

The one condition: every size's step runs faster than its own sample rate (x real time > 1); exit status 1 otherwise.  Everything else
is reported, not gated.

usage (GPU box):  python scripts/bench_grid10_bank.py [rounds = 3] [out = profiles/grid10_bank/bench.txt]
prints the table and writes it to `out`; numbers from different jobs do not compare."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from gr_amps_amd import capi

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "grid10_bank", "bench.txt")
PUSH = 1 << 22
dev = torch.device("cuda:0")
STEP_KEYS = ("ms_channelizer", "ms_front", "ms_resolve", "ms_carry", "ms_decode")

g = torch.Generator(device=dev)
g.manual_seed(5)
block_f = torch.view_as_complex(torch.randn((PUSH, 2), generator=g, device=dev, dtype=torch.float32).contiguous())
block_s = torch.round(torch.view_as_real(block_f) * 4000.0).clamp(-32000, 32000).to(torch.int16).contiguous()
block_b = torch.round(torch.view_as_real(block_f) * 30.0).clamp(-127, 127).to(torch.int8).contiguous()
torch.cuda.synchronize()
FORMATS = {"fc32": (capi.SAMPLES_FC32, block_f), "sc16": (capi.SAMPLES_SC16, block_s), "sc8": (capi.SAMPLES_SC8, block_b)}


def geometry(M):
    """(input samples per frame, channels, sample rate) of the bank of M branches"""
    return (M // 4, M // 3, M * 10e3) if M in capi.GRID10_CHANNELS else (3 * M // 4, M, M * 30e3)


def handle(M):
    D, C, _ = geometry(M)
    r = capi.Recc(n_channels=C, max_samples=PUSH // D + 72, max_bursts=4096, time_kernels=True, slicer="exact", sync_torch=False,
                  wideband={"channels": M, "decim": D, "first_channel": 0})
    r.set_timing("all")
    return r


def leg(r, fmt, npush):
    """(ms_channelizer per push, step ms per push) over npush pushes behind two of warm-up"""
    format, block = FORMATS[fmt]
    for _ in range(2):
        r.push_wideband_as(block, format)
    r.drain(copy=False)
    r.timing(reset=True)
    for _ in range(npush):
        r.push_wideband_as(block, format)
    r.drain(copy=False)
    t = r.timing()
    return t["ms_channelizer"] / npush, sum(t[k] for k in STEP_KEYS) / npush


legs = [(512, "fc32", "first")] + [(M, fmt, "") for M in capi.GRID10_CHANNELS for fmt in ("fc32", "sc16", "sc8")] + [(512, "fc32", "last")]
handles = {M: handle(M) for M, fmt, tag in legs}
results = {}
for rnd in range(rounds):
    for M, fmt, tag in legs:
        npush = -(-int(geometry(M)[2]) // PUSH)
        results.setdefault((M, fmt, tag), []).append(leg(handles[M], fmt, npush))
for h in handles.values():
    h.close()

lines = ["rounds %d, pushes of 2^22 samples, every admissible channel active, spec D; medians" % rounds,
         "%-30s %7s %10s %10s %9s %9s %11s %11s" % ("leg", "pushes", "chz ms", "step ms", "chz Msps", "step Msps", "x real time", "ns/sample")]
slow = []
for key in legs:
    M, fmt, tag = key
    D, C, fs = geometry(M)
    chz, step = (float(np.median([v[i] for v in results[key]])) for i in (0, 1))
    name = "M=%d D=%d C=%d %s%s" % (M, D, C, fmt, " yardstick (%s)" % tag if tag else "")
    real = PUSH / step * 1e3 / fs
    lines.append("%-30s %7d %10.4f %10.4f %9.0f %9.0f %11.1f %11.4f" % (name, -(-int(fs) // PUSH), chz, step, PUSH / chz / 1e3, PUSH / step / 1e3, real, chz * 1e6 / PUSH))
    if not tag and real <= 1.0:
        slow.append(name)
lines.append("slower than their own sample rate: %s" % (", ".join(slow) if slow else "none"))
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
sys.exit(1 if slow else 0)
