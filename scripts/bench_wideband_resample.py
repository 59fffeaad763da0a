#!/usr/bin/env python
"""The wideband seam behind its L / M resampler (wb_resample_kernel) against the plain bank it feeds, in ONE process and one job, in the
shape of scripts/bench_xlate_shared_resample.py: one second of a 4 Msps sc8 stream x 5/4 into the 500 bank against one second of a
5 Msps sc8 stream into a plain 500 handle, and 12.5 Msps x 2/1 into the 2500 bank against 25 Msps into a plain 2500 handle; every
channel of the band decoded, device-resident blocks.  A step is a push plus a drain; legs alternate, three rounds of `--steps` steps,
best of the rounds.  Per leg: ms per block on the host clock and the multiple of real time; in a pass of its own ms_channelizer by the
library's events.  That span is all that is MEASURED: it covers everything up to and including the bank kernel, the resampler's two
kernels (wb_resample_kernel and its carry kernel) too where there are any.  Behind the resampler the bank runs its fc32 instantiation on
the resampler's output, not the sc8 one of the plain leg, so each bank has a third leg: the plain handle fed a device fc32 block of the
same length, whose span is the time of the very bank kernel the resampling leg runs (ms_bank_kernel).  ms_resample_kernels is the
resampling leg's span minus that one: a DIFFERENCE of two measured spans, both kernels of the resampler together.
usage (GPU box): python scripts/bench_wideband_resample.py [--steps 10] [--out profiles/wideband_resample/resample.json]"""
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
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wideband_resample", "resample.json"))
args = ap.parse_args()

# (name, delivered rate, interp, decim, bank, bank decimation, format of the block, the plain fc32 leg whose bank kernel it runs)
LEGS = [("5M_plain_500", 5e6, 1, 1, 500, 125, "sc8", None), ("5M_plain_500_fc32", 5e6, 1, 1, 500, 125, "fc32", None),
        ("4M_5_4_500", 4e6, 5, 4, 500, 125, "sc8", "5M_plain_500_fc32"),
        ("25M_plain_2500", 25e6, 1, 1, 2500, 625, "sc8", None), ("25M_plain_2500_fc32", 25e6, 1, 1, 2500, 625, "fc32", None),
        ("12.5M_2_1_2500", 12.5e6, 2, 1, 2500, 625, "sc8", "25M_plain_2500_fc32")]
dev = torch.device("cuda", 0)
torch.manual_seed(1)

legs = {}
for name, rate, interp, decim, channels, D, fmt, _ in LEGS:
    n = int(rate)                                                   # 1 s of signal
    nout = -(-n * interp // decim)
    block = torch.randint(-100, 101, (n, 2), device=dev, dtype=torch.int8)
    if fmt == "fc32":                                               # the same kind of samples as the bank behind a resampler reads them
        block = torch.view_as_complex(block.to(torch.float32).contiguous())
    wb = {"channels": channels, "decim": D}
    if interp != decim:
        wb["resample"] = (rate, interp, decim)
    rx = capi.Recc(n_channels=channels // 3, max_samples=nout // D + 8, max_bursts=256, wideband=wb, sync_torch=False)
    legs[name] = {"rx": rx, "block": block, "n": n, "nout": nout, "frames": nout // D, "fmt": fmt}
torch.cuda.synchronize()


def step(leg):
    if leg["fmt"] == "fc32":
        leg["rx"].push_wideband(leg["block"])
    else:
        leg["rx"].push_wideband_as(leg["block"], capi.SAMPLES_SC8)
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
    t = leg["rx"].timing()
    return {"ms_channelizer": t["ms_channelizer"] / steps, "ms_front": t["ms_front"] / steps}


for _ in range(3):                                   # warm-up: code objects, the handles' first pushes, the output buffers' growth
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
    print("round, ms_channelizer per block: " + ", ".join("%s %.4f" % (k, v["ms_channelizer"]) for k, v in krounds[-1].items()), flush=True)
for leg in legs.values():
    leg["rx"].close()

res = {
    "setup": {"block": "1 s of uniform noise in -100 ... 100, sc8 (the _fc32 legs: the same as fc32), device-resident; every channel of the band decoded",
              "legs": {name: {"rate_hz": rate, "interp": interp, "decim": decim, "channels": channels, "bank_decim": D, "format": fmt, "block_samples": legs[name]["n"],
                              "bank_samples": legs[name]["nout"], "frames": legs[name]["frames"]} for name, rate, interp, decim, channels, D, fmt, _ in LEGS},
              "steps_per_leg": args.steps, "rounds": args.rounds, "device": torch.cuda.get_device_name(0)},
    "rounds_ms_per_block": rounds,
    "rounds_kernels": krounds,
    "ms_per_block": {name: min(r[name] for r in rounds) for name in legs},
    "ms_channelizer_span": {name: min(r[name]["ms_channelizer"] for r in krounds) for name in legs},
    "ms_front": {name: min(r[name]["ms_front"] for r in krounds) for name in legs},
}
res["what_is_measured"] = ("ms_per_block (host clock) and ms_channelizer_span (the library's events) are measured; ms_bank_kernel of a plain leg is its span, of a "
                           "resampling leg the span of the plain fc32 leg that runs the same bank kernel on as many samples; ms_resample_kernels is the "
                           "difference of the resampling leg's span and that one (wb_resample_kernel and its carry kernel together), no measurement of its own")
res["ms_bank_kernel"] = {name: res["ms_channelizer_span"][plain or name] for name, *_, plain in LEGS}
res["ms_resample_kernels"] = {name: res["ms_channelizer_span"][name] - res["ms_channelizer_span"][plain] for name, *_, plain in LEGS if plain}
res["times_real_time"] = {name: 1e3 / res["ms_per_block"][name] for name in legs}
print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1, sort_keys=True)
    f.write("\n")
