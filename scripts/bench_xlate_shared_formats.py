#!/usr/bin/env python
"""The shared translate seam on an SDR's integer samples against the fc32 path, in ONE process and one job (machines differ by up to
12 %), in the shape of scripts/bench_xlate_shared.py: a system's 21 control channels out of one 800 ksps stream, one block of 800 000
samples (1 s of signal) per step, decimation 4.  A step is a push plus a drain; legs alternate, three rounds of 20 steps.
  device-resident legs: fc32 (push_raw_shared), sc16 and cu8 (push_raw_shared_as, the block read in place): ms per block on the host
      clock, and in a pass of their own ms_xlate by the library's events (the channel filter alone);
  host-resident legs:   fc32; sc16 pushed as it is; sc16 converted by capi.convert_samples INSIDE the timed region and pushed as
      fc32 -- what a caller had to do before the _as entry points.  The ratio of the third to the second is the feature's worth.
  --ab-lib OTHER.so:    did the fc32 path move?  The device-resident fc32 leg alone, in fresh child processes that load this tree's
      library and OTHER (an A/B build of the parent revision, through AMPS_RECC_LIB) in turn, three of each, alternating in the same
      job.  Reported: the difference between the two libraries and what two legs of the SAME library differ by.
usage (GPU box): python scripts/bench_xlate_shared_formats.py [--steps 20] [--ab-lib parent/libamps_recc.so] [--out profiles/xlate_shared/formats.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gr_amps_amd import capi  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--ab-lib", default=None, help="another build of libamps_recc.so to compare the fc32 leg against")
ap.add_argument("--fc32-leg-only", action="store_true", help="(the --ab-lib child) one device-resident fc32 leg of whatever library AMPS_RECC_LIB names")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xlate_shared", "formats.json"))
args = ap.parse_args()

RATE, DECIM, N = 800e3, 4, 800_000
centres = [-300e3 + 30e3 * i for i in range(21)]
dev = torch.device("cuda", 0)
torch.manual_seed(1)
noise = torch.randn(N, 2, device=dev).mul_(0.5)                       # the block of scripts/bench_xlate_shared.py
d_fc32 = torch.view_as_complex(noise).contiguous()
torch.cuda.synchronize()

rx = capi.Recc(n_channels=21, sps=10, max_samples=N // DECIM, max_bursts=256, sync_torch=False)
rx.set_xlate_shared(RATE, centres, DECIM)


def leg(step, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    return (time.perf_counter() - t0) * 1e3 / steps


def kernel_leg(step, steps):
    rx.timing(reset=True)
    for _ in range(steps):
        step()
    return rx.timing()["ms_xlate"] / steps


def step_d_fc32():
    rx.push_raw_shared(d_fc32)
    rx.drain(copy=False)


if args.fc32_leg_only:
    for _ in range(3):
        step_d_fc32()
    ms = leg(step_d_fc32, args.steps)
    rx.set_timing("all")
    k = kernel_leg(step_d_fc32, args.steps)
    rx.close()
    print(json.dumps({"lib": os.path.relpath(capi.LIB_PATH, ROOT), "ms_per_block": ms, "ms_xlate": k}))
    sys.exit(0)

# the same noise as a converter would deliver it: 2048 per unit for sc16 (4 sigma = 4096 of 32 767), 32 per unit for cu8, clipped
d_sc16 = noise.mul(2048.0).round_().clamp_(-32768, 32767).to(torch.int16).contiguous()
d_cu8 = noise.mul(32.0).add_(128.0).floor_().clamp_(0, 255).to(torch.uint8).contiguous()
torch.cuda.synchronize()
h_fc32 = d_fc32.cpu().numpy()
h_sc16 = d_sc16.cpu().numpy()


def step_d_sc16():
    rx.push_raw_shared_as(d_sc16, capi.SAMPLES_SC16)
    rx.drain(copy=False)


def step_d_cu8():
    rx.push_raw_shared_as(d_cu8, capi.SAMPLES_CU8)
    rx.drain(copy=False)


def step_h_fc32():
    rx.push_raw_shared(h_fc32)
    rx.drain(copy=False)


def step_h_sc16():
    rx.push_raw_shared_as(h_sc16, capi.SAMPLES_SC16)
    rx.drain(copy=False)


def step_h_sc16_converted():
    rx.push_raw_shared(capi.convert_samples(h_sc16, capi.SAMPLES_SC16))
    rx.drain(copy=False)


LEGS = [("device_fc32", step_d_fc32), ("device_sc16", step_d_sc16), ("device_cu8", step_d_cu8),
        ("host_fc32", step_h_fc32), ("host_sc16", step_h_sc16), ("host_sc16_converted_then_fc32", step_h_sc16_converted)]
for _ in range(3):                                   # warm-up: code objects, the staging buffer, the handle's first pushes
    for _, step in LEGS:
        step()
rounds = []
for _ in range(args.rounds):
    rounds.append({name: leg(step, args.steps) for name, step in LEGS})
    print("round, ms per block: " + ", ".join("%s %.3f" % kv for kv in rounds[-1].items()), flush=True)
# kernel time by the library's events, in a pass of its own (the event records perturb the host-clock legs above)
rx.set_timing("all")
krounds = []
for _ in range(args.rounds):
    krounds.append({name: kernel_leg(step, args.steps) for name, step in LEGS[:3]})
    print("round, ms_xlate per block: " + ", ".join("%s %.4f" % kv for kv in krounds[-1].items()), flush=True)
rx.close()

res = {
    "setup": {"centres": 21, "rate_hz": RATE, "decim": DECIM, "block_samples": N, "block": "noise, sigma 0.5 per component; sc16 at 2048 per unit, cu8 at 32 per unit",
              "steps_per_leg": args.steps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)},
    "rounds_ms_per_block": rounds,
    "rounds_ms_xlate": krounds,
    "ms_per_block": {name: min(r[name] for r in rounds) for name, _ in LEGS},
    "ms_xlate": {name: min(r[name] for r in krounds) for name, _ in LEGS[:3]},
}
res["host_convert_then_fc32_over_sc16_in_place"] = res["ms_per_block"]["host_sc16_converted_then_fc32"] / res["ms_per_block"]["host_sc16"]
res["host_fc32_over_sc16_in_place"] = res["ms_per_block"]["host_fc32"] / res["ms_per_block"]["host_sc16"]

if args.ab_lib:
    runs = {"this": [], "other": []}
    for i in range(2 * args.rounds):                 # fresh processes, one at a time, alternating: this, other, this, other, ...
        which = "this" if i % 2 == 0 else "other"
        env = dict(os.environ)
        if which == "other":
            env["AMPS_RECC_LIB"] = os.path.abspath(args.ab_lib)
        else:
            env.pop("AMPS_RECC_LIB", None)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--fc32-leg-only", "--steps", str(args.steps)], env=env,
                             capture_output=True, text=True, timeout=300)
        if out.returncode != 0:
            sys.exit("the %s library's fc32 leg failed (%d): %s" % (which, out.returncode, out.stderr[-2000:]))
        runs[which].append(json.loads(out.stdout.strip().splitlines()[-1]))
        print("fc32 leg, %s library: %.3f ms per block, ms_xlate %.4f" % (which, runs[which][-1]["ms_per_block"], runs[which][-1]["ms_xlate"]), flush=True)
    ab = {"other_lib": args.ab_lib, "runs": runs}
    for key in ("ms_per_block", "ms_xlate"):
        a, b = [r[key] for r in runs["this"]], [r[key] for r in runs["other"]]
        ab[key] = {"this_median": float(np.median(a)), "other_median": float(np.median(b)),
                   "difference_of_medians": float(np.median(a) - np.median(b)),
                   "same_library_spread": float(max(max(a) - min(a), max(b) - min(b)))}
        ab[key]["inside_the_spread"] = abs(ab[key]["difference_of_medians"]) <= ab[key]["same_library_spread"]
    res["fc32_path_this_library_against_other"] = ab

print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write("\n")
