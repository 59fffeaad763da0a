#!/usr/bin/env python
"""The shared translate seam against what there was before it, in ONE process and one job (machines differ by up to 12 %): a system's 21
control channels out of one 800 ksps stream, a device-resident block of 800 000 samples (1 s of signal) per step, decimation 4.
  leg (a): one 21-channel handle, set_xlate_shared + push_raw_shared of the block, one drain;
  leg (b): 21 one-channel handles, each set_xlate(centre) + push_raw of the same block, then the 21 drains.
The legs alternate, three rounds each; a step is timed on the host clock around work that ends in the drain's synchronise.  Behind them
the kernels' own time by the library's events (ms_xlate: the channel filter alone) for both forms.
usage (GPU box): python scripts/bench_xlate_shared.py [--steps 20] [--out profiles/xlate_shared/bench_xlate_shared.json]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gr_amps_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xlate_shared", "bench_xlate_shared.json"))
args = ap.parse_args()

RATE, DECIM, N = 800e3, 4, 800_000
centres = [-300e3 + 30e3 * i for i in range(21)]
dev = torch.device("cuda", 0)
torch.manual_seed(1)
x = torch.view_as_complex(torch.randn(N, 2, device=dev).mul_(0.5)).contiguous()
torch.cuda.synchronize()

shared = capi.Recc(n_channels=21, sps=10, max_samples=N // DECIM, max_bursts=256, sync_torch=False)
shared.set_xlate_shared(RATE, centres, DECIM)
singles = []
for fc in centres:
    r = capi.Recc(n_channels=1, sps=10, max_samples=N // DECIM, max_bursts=16, sync_torch=False)
    r.set_xlate(rate_hz=RATE, center_hz=fc, decim=DECIM)
    singles.append(r)
x1 = x.reshape(1, N)


def step_shared():
    shared.push_raw_shared(x)
    shared.drain(copy=False)


def step_singles():
    for r in singles:
        r.push_raw(x1)
    for r in singles:
        r.drain(copy=False)


def leg(step, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    return (time.perf_counter() - t0) * 1e3 / steps


for _ in range(3):                                   # warm-up: code objects, staging, the handles' first pushes
    step_shared()
    step_singles()
rounds = []
for _ in range(args.rounds):
    a = leg(step_shared, args.steps)
    b = leg(step_singles, args.steps)
    rounds.append({"shared_ms_per_block": a, "singles_ms_per_block": b})
    print("round: shared %.3f ms/block, 21 one-channel handles %.3f ms/block (x%.2f)" % (a, b, b / a), flush=True)

# kernel time by the library's events, in legs of their own (the event records perturb the host-clock legs above)
shared.set_timing("all")
shared.timing(reset=True)
for _ in range(args.steps):
    step_shared()
ta = shared.timing()
for r in singles:
    r.set_timing("all")
    r.timing(reset=True)
for _ in range(args.steps):
    step_singles()
tb = [r.timing() for r in singles]
keys = ("ms_xlate", "ms_front", "ms_resolve", "ms_carry")
res = {
    "setup": {"centres": 21, "rate_hz": RATE, "decim": DECIM, "block_samples": N, "block": "device-resident fc32 noise", "steps_per_leg": args.steps,
              "rounds": args.rounds, "device": torch.cuda.get_device_name(0)},
    "rounds": rounds,
    "shared_ms_per_block": min(r["shared_ms_per_block"] for r in rounds),
    "singles_ms_per_block": min(r["singles_ms_per_block"] for r in rounds),
    "shared_kernel_ms_per_block": {k: ta[k] / args.steps for k in keys},
    "singles_kernel_ms_per_block_sum_of_21": {k: sum(t[k] for t in tb) / args.steps for k in keys},
}
res["speedup"] = res["singles_ms_per_block"] / res["shared_ms_per_block"]
# the FIR's arithmetic: 597 real taps x complex samples, 2 flop per fma per component, for 21 x 200 000 outputs
res["shared_xlate_tflops"] = 21 * (N // DECIM) * 597 * 4 / (res["shared_kernel_ms_per_block"]["ms_xlate"] * 1e-3) / 1e12
shared.close()
for r in singles:
    r.close()
print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write("\n")
