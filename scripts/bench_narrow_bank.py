"""What the narrow filter banks cost: the wideband seam at M = 512, 256, 128 branches (15.36, 7.68, 3.84 Msps), D = M / 2 and 3 M / 4,
on fc32, sc16 and sc8 blocks (the same noise in each format), beside the two-kernel form of the 1024 bank (AMPS_RECC_FLAG_UNFUSED_WIDEBAND, all 1024 bins) as the
yardstick per input sample -- all in ONE process, because boxes differ by up to 12 %.

Per geometry one second of stream (M x 30 000 samples, rounded up to whole pushes) is pushed from a device-resident block of 2^22
samples of noise, every bin a channel, spec D.  Times come from amps_recc_get_timing in timing mode "all": ms_channelizer is the
filter-bank kernel, the step is the sum of every kernel the push launches (filter bank, streaming kernel, resolve, carry, decode).
The legs alternate: yardstick, then per geometry fc32, sc16, sc8 and the same three again (legs A and B: what two legs of one format
differ by is the noise a difference between formats has to exceed), yardstick again, `rounds` times; the table holds each leg's median
over the rounds.

usage (GPU box):  python scripts/bench_narrow_bank.py [rounds = 3]
prints a table; numbers from different jobs do not compare."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gr_amps_amd import capi

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
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


def handle(M, D, unfused=False):
    r = capi.Recc(n_channels=M, max_samples=PUSH // D + 72, max_bursts=4096, time_kernels=True, slicer="exact", sync_torch=False,
                  unfused_wideband=unfused, wideband={"channels": M, "decim": D, "first_channel": 0})
    r.set_timing("all")
    return r


def leg(r, fmt, npush):
    """(ms_channelizer per push, step ms per push) over npush pushes behind two of warm-up"""
    format, block = FORMATS[fmt]
    push = lambda b: r.push_wideband_as(b, format)
    for _ in range(2):
        push(block)
    r.drain(copy=False)
    r.timing(reset=True)
    for _ in range(npush):
        push(block)
    r.drain(copy=False)
    t = r.timing()
    return t["ms_channelizer"] / npush, sum(t[k] for k in STEP_KEYS) / npush


yardstick = [(1024, 768, "fc32", "A"), (1024, 512, "fc32", "A")]
legs = yardstick + [(M, D, fmt, ab) for M in (512, 256, 128) for D in (3 * M // 4, M // 2) for ab in "AB" for fmt in ("fc32", "sc16", "sc8")]
legs += [(M, D, fmt, "B") for M, D, fmt, _ in yardstick]     # the yardstick first and last
handles = {(M, D): handle(M, D, M == 1024) for M, D, fmt, ab in legs}
results = {}
for rnd in range(rounds):
    for M, D, fmt, ab in legs:
        npush = -(-M * 30000 // PUSH)
        results.setdefault((M, D, fmt, ab), []).append(leg(handles[(M, D)], fmt, npush))
for h in handles.values():
    h.close()

print("rounds %d, pushes of 2^22 samples, every bin a channel, spec D; medians" % rounds)
print("%-28s %7s %10s %10s %9s %9s %11s %11s" % ("leg", "pushes", "chz ms", "step ms", "chz Msps", "step Msps", "x real time", "ns/sample"))
yard = {}
for key in sorted(results, key=lambda k: (-k[0], -k[1], k[2], k[3])):
    M, D, fmt, ab = key
    chz, step = (float(np.median([v[i] for v in results[key]])) for i in (0, 1))
    name = "M=%d D=%d %s %s" % (M, D, fmt, ("unfused (%s)" % ab) if M == 1024 else "(%s)" % ab)
    fs = M * 30e3
    print("%-28s %7d %10.4f %10.4f %9.0f %9.0f %11.0f %11.4f" % (name, -(-M * 30000 // PUSH), chz, step, PUSH / chz / 1e3, PUSH / step / 1e3,
                                                                 PUSH / step * 1e3 / fs, chz * 1e6 / PUSH))
    if M == 1024:
        yard.setdefault(D, []).append(chz * 1e6 / PUSH)
print("yardstick, filter-bank kernel ns per input sample (legs A, B): " + ", ".join("D=%d: %s" % (D, " ".join("%.4f" % v for v in vs)) for D, vs in sorted(yard.items())))
