#!/usr/bin/env python
"""The shared translate seam at the rates SDRs deliver (xlate_shared_wide_kernel: decimations 12, 10, 16, 5) against the staged kernel
at 1.6 Msps / 8 (xlate_shared_kernel<8>), in ONE process and one job (machines differ by up to 12 %), in the shape of
scripts/bench_xlate_shared.py: 21 centres 30 kHz apart out of one stream, one device-resident fc32 block of 1 s of signal per step, the
default channel filter of each rate, 10 samples per symbol behind it.  A step is a push plus a drain; legs alternate, three rounds of
20 steps.  Per leg: ms per block on the host clock; in a pass of its own ms_xlate by the library's events (the channel filter alone);
real-tap MACs per second = centres x outputs x ntaps / ms_xlate; and how many times real time the 1 s block is decoded.
usage (GPU box): python scripts/bench_xlate_shared_rates.py [--steps 20] [--out profiles/xlate_shared/rates.json]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xlate_shared", "rates.json"))
args = ap.parse_args()

# (name, rate, decimation): the yardstick first
LEGS = [("1600k_d8", 1.6e6, 8), ("2400k_d12", 2.4e6, 12), ("2000k_d10", 2.0e6, 10), ("3200k_d16", 3.2e6, 16), ("1000k_d5", 1.0e6, 5)]
centres = [-300e3 + 30e3 * i for i in range(21)]
dev = torch.device("cuda", 0)
torch.manual_seed(1)

legs = {}
for name, rate, decim in LEGS:
    n = int(rate)                                                   # 1 s of signal
    ntaps = dict((d, t) for d, _, t in capi.subband_plan(rate))[decim]
    block = torch.view_as_complex(torch.randn(n, 2, device=dev).mul_(0.5)).contiguous()
    rx = capi.Recc(n_channels=21, sps=10, max_samples=n // decim, max_bursts=256, sync_torch=False)
    rx.set_xlate_shared(rate, centres, decim)
    legs[name] = {"rx": rx, "block": block, "n": n, "decim": decim, "ntaps": ntaps}
torch.cuda.synchronize()


def step(leg):
    leg["rx"].push_raw_shared(leg["block"])
    leg["rx"].drain(copy=False)


def host_leg(leg, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        step(leg)
    return (time.perf_counter() - t0) * 1e3 / steps


def kernel_leg(leg, steps):
    leg["rx"].timing(reset=True)
    for _ in range(steps):
        step(leg)
    return leg["rx"].timing()["ms_xlate"] / steps


for _ in range(3):                                   # warm-up: code objects, the handles' first pushes
    for leg in legs.values():
        step(leg)
rounds = []
for _ in range(args.rounds):
    rounds.append({name: host_leg(leg, args.steps) for name, leg in legs.items()})
    print("round, ms per block: " + ", ".join("%s %.3f" % kv for kv in rounds[-1].items()), flush=True)
# kernel time by the library's events, in a pass of its own (the event records perturb the host-clock legs above)
for leg in legs.values():
    leg["rx"].set_timing("all")
krounds = []
for _ in range(args.rounds):
    krounds.append({name: kernel_leg(leg, args.steps) for name, leg in legs.items()})
    print("round, ms_xlate per block: " + ", ".join("%s %.4f" % kv for kv in krounds[-1].items()), flush=True)
for leg in legs.values():
    leg["rx"].close()

res = {
    "setup": {"centres": 21, "block": "1 s of noise, sigma 0.5 per component, fc32, device-resident", "samples_per_symbol": 10,
              "legs": {name: {"rate_hz": rate, "decim": decim, "ntaps": legs[name]["ntaps"], "block_samples": legs[name]["n"]} for name, rate, decim in LEGS},
              "steps_per_leg": args.steps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)},
    "rounds_ms_per_block": rounds,
    "rounds_ms_xlate": krounds,
    "ms_per_block": {name: min(r[name] for r in rounds) for name in legs},
    "ms_xlate": {name: min(r[name] for r in krounds) for name in legs},
}
res["gmacs_per_s"] = {name: 21 * (leg["n"] // leg["decim"]) * leg["ntaps"] / (res["ms_xlate"][name] * 1e-3) / 1e9 for name, leg in legs.items()}
res["mac_rate_over_the_d8_leg"] = {name: res["gmacs_per_s"][name] / res["gmacs_per_s"]["1600k_d8"] for name in legs}
res["times_real_time"] = {name: 1e3 / res["ms_per_block"][name] for name in legs}
print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write("\n")
