"""What the tuner correction inside the filter bank costs (amps_recc_set_wideband_shift: a sincospif and a complex multiply per staged
sample in the mixing twins of the narrow and the 10 kHz-grid kernels): M = 128 and 512 at D = 3 M / 4, M = 500 and 2500 at D = M / 4, on
fc32 and sc8 blocks (the same noise in both), every admissible channel active -- all in ONE process, because boxes differ by up to 12 %.

Per size and format the legs alternate on one handle: shift off, shift on (+6543.21 Hz), shift off again, `rounds` times; one second of
stream per leg (rounded up to whole pushes of 2^22 samples, 32 pushes at least) from a device-resident block, spec D.  Times come from
amps_recc_get_timing in timing mode "all": ms_channelizer is the filter-bank kernel, the step is the sum of every kernel the push
launches.  The table holds each leg's median over the rounds; the off legs run the unmixed kernels (instruction for instruction the
parent's: profiles/wideband_shift/isa_identity.txt) and their spread, |first - last| / mean, says what a difference in this job means.

The one condition: every size's whole step with the shift on runs faster than its own sample rate (x real time > 1); exit status 1
otherwise.  Everything else is reported, not gated.

usage (GPU box):  python scripts/bench_wideband_shift.py [rounds = 3] [out = profiles/wideband_shift/bench.txt]
prints the table and writes it to `out`; numbers from different jobs do not compare."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from gr_amps_amd import capi

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "wideband_shift", "bench.txt")
PUSH = 1 << 22
SHIFT_HZ = 6543.21
SIZES = (128, 512, 500, 2500)
MIN_PUSHES = 32                                   # one second of stream is one push at M = 128: too short a window to compare legs by
dev = torch.device("cuda:0")
STEP_KEYS = ("ms_channelizer", "ms_front", "ms_resolve", "ms_carry", "ms_decode")

g = torch.Generator(device=dev)
g.manual_seed(5)
block_f = torch.view_as_complex(torch.randn((PUSH, 2), generator=g, device=dev, dtype=torch.float32).contiguous())
block_b = torch.round(torch.view_as_real(block_f) * 30.0).clamp(-127, 127).to(torch.int8).contiguous()
torch.cuda.synchronize()
FORMATS = {"fc32": (capi.SAMPLES_FC32, block_f), "sc8": (capi.SAMPLES_SC8, block_b)}


def geometry(M):
    """(input samples per frame, channels, sample rate) of the bank of M branches"""
    return (M // 4, M // 3, M * 10e3) if M in capi.GRID10_CHANNELS else (3 * M // 4, M, M * 30e3)


def handle(M):
    D, C, _ = geometry(M)
    r = capi.Recc(n_channels=C, max_samples=PUSH // D + 72, max_bursts=4096, time_kernels=True, slicer="exact", sync_torch=False,
                  wideband={"channels": M, "decim": D, "first_channel": 0})
    r.set_timing("all")
    return r


def leg(r, fmt, shift_hz, npush):
    """(ms_channelizer per push, step ms per push) over npush pushes behind two of warm-up, with the shift set first"""
    format, block = FORMATS[fmt]
    r.set_wideband_shift(shift_hz)
    for _ in range(2):
        r.push_wideband_as(block, format)
    r.drain(copy=False)
    r.timing(reset=True)
    for _ in range(npush):
        r.push_wideband_as(block, format)
    r.drain(copy=False)
    t = r.timing()
    return t["ms_channelizer"] / npush, sum(t[k] for k in STEP_KEYS) / npush


LEGS = (("off", 0.0), ("on", SHIFT_HZ), ("off again", 0.0))
handles = {M: handle(M) for M in SIZES}
results = {}
for rnd in range(rounds):
    for M in SIZES:
        npush = max(MIN_PUSHES, -(-int(geometry(M)[2]) // PUSH))
        for fmt in FORMATS:
            for tag, hz in LEGS:
                results.setdefault((M, fmt, tag), []).append(leg(handles[M], fmt, hz, npush))
for h in handles.values():
    h.close()

lines = ["rounds %d, pushes of 2^22 samples, every admissible channel active, spec D, shift %+.2f Hz on the `on` legs; medians" % (rounds, SHIFT_HZ),
         "%-24s %-9s %7s %10s %10s %9s %11s %11s" % ("size", "shift", "pushes", "chz ms", "step ms", "chz Msps", "x real time", "ns/sample")]
slow = []
for M in SIZES:
    D, C, fs = geometry(M)
    for fmt in FORMATS:
        med = {tag: tuple(float(np.median([v[i] for v in results[(M, fmt, tag)]])) for i in (0, 1)) for tag, _ in LEGS}
        name = "M=%d D=%d C=%d %s" % (M, D, C, fmt)
        for tag, _ in LEGS:
            chz, step = med[tag]
            real = PUSH / step * 1e3 / fs
            lines.append("%-24s %-9s %7d %10.4f %10.4f %9.0f %11.1f %11.4f" % (name, tag, max(MIN_PUSHES, -(-int(fs) // PUSH)), chz, step, PUSH / chz / 1e3, real, chz * 1e6 / PUSH))
            if tag == "on" and real <= 1.0:
                slow.append(name)
        off = 0.5 * (med["off"][0] + med["off again"][0])
        off_step = 0.5 * (med["off"][1] + med["off again"][1])
        lines.append("%-24s on / off: filter bank x %.3f, step x %.3f; spread of the off legs %.1f %%" % (
            "", med["on"][0] / off, med["on"][1] / off_step, 100.0 * abs(med["off"][0] - med["off again"][0]) / off))
lines.append("slower than their own sample rate with the shift on: %s" % (", ".join(slow) if slow else "none"))
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
sys.exit(1 if slow else 0)
