#!/usr/bin/env python
"""The shared translate seam behind the rational resampler (xlate_shared_rational_kernel: 2.048 Msps x 5/64 and 2.5 Msps x 2/25) against
the wide kernel at 2.4 Msps / 12 (xlate_shared_wide_kernel), in ONE process and one job (machines differ by up to 12 %), in the shape
of scripts/bench_xlate_shared_rates.py: 21 centres 30 kHz apart out of one stream, one device-resident fc32 block of 1 s of signal per
step, the default channel filter of each rate.  A step is a push plus a drain; legs alternate, three rounds of 20 steps.  Per leg: ms
per block on the host clock; in a pass of its own ms_xlate by the library's events (the channel filter alone); real-tap MACs per
second = centres x outputs x padded taps (per phase) / ms_xlate; and how many times real time the 1 s block is decoded.
usage (GPU box): python scripts/bench_xlate_shared_resample.py [--steps 20] [--out profiles/xlate_shared/resample.json]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xlate_shared", "resample.json"))
args = ap.parse_args()

# (name, rate, interp, decim, samples per symbol): the yardstick first
YARD = "2400k_d12"
LEGS = [(YARD, 2.4e6, 1, 12, 10), ("2048k_5_64", 2.048e6, 5, 64, 8), ("2500k_2_25", 2.5e6, 2, 25, 10)]
centres = [-300e3 + 30e3 * i for i in range(21)]
dev = torch.device("cuda", 0)
torch.manual_seed(1)


def pad8(n):
    return (n + 7) // 8 * 8


legs = {}
for name, rate, interp, decim, sps in LEGS:
    n = int(rate)                                                   # 1 s of signal
    nout = -(-n * interp // decim) if interp > 1 else n // decim
    block = torch.view_as_complex(torch.randn(n, 2, device=dev).mul_(0.5)).contiguous()
    rx = capi.Recc(n_channels=21, sps=sps, max_samples=nout, max_bursts=256, sync_torch=False)
    if interp > 1:
        ntaps = dict(((L, M), t) for L, M, _, t in capi.resample_plan(rate))[(interp, decim)]   # per phase
        rx.set_xlate_resampled(rate, centres, interp, decim)
    else:
        ntaps = dict((d, t) for d, _, t in capi.subband_plan(rate))[decim]
        rx.set_xlate_shared(rate, centres, decim)
    legs[name] = {"rx": rx, "block": block, "n": n, "nout": nout, "ntaps": ntaps, "ntp": pad8(ntaps)}
torch.cuda.synchronize()


def step(leg):
    leg["rx"].push_raw_shared(leg["block"])           # a whole second: rate x interp / decim outputs every push, no remainder
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
    "setup": {"centres": 21, "block": "1 s of noise, sigma 0.5 per component, fc32, device-resident",
              "legs": {name: {"rate_hz": rate, "interp": interp, "decim": decim, "samples_per_symbol": sps, "ntaps": legs[name]["ntaps"],
                              "padded_taps": legs[name]["ntp"], "block_samples": legs[name]["n"], "outputs": legs[name]["nout"]}
                       for name, rate, interp, decim, sps in LEGS},
              "steps_per_leg": args.steps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)},
    "rounds_ms_per_block": rounds,
    "rounds_ms_xlate": krounds,
    "ms_per_block": {name: min(r[name] for r in rounds) for name in legs},
    "ms_xlate": {name: min(r[name] for r in krounds) for name in legs},
}
res["gmacs_per_s"] = {name: 21 * leg["nout"] * leg["ntp"] / (res["ms_xlate"][name] * 1e-3) / 1e9 for name, leg in legs.items()}
res["mac_rate_over_the_yardstick"] = {name: res["gmacs_per_s"][name] / res["gmacs_per_s"][YARD] for name in legs}
res["times_real_time"] = {name: 1e3 / res["ms_per_block"][name] for name in legs}
print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write("\n")
