"""What AMPS_RECC_FLAG_CHANNEL_POWER costs the wideband seam, measured in ONE process: the bench's own step (bench.py: 138 412 032
samples at D = 768, 2^27 at D = 512; spec D, 832 channels from bin 96, device-resident fc32 block, records drained every step with the
split drain) with the flag off and on.  Per decimation the legs run in ROUNDS, each round `reps` steps of every leg back to back:
  off_a, on, off_b    -- the off leg runs twice per round, first and last, so that its own spread inside the job is on record beside
                         every difference (two handles of the same build, the same block).
Per leg: step ms (host clock over the leg's steps, stream synchronised at both ends), the filter-bank kernel's ms from the library's own
events (amps_recc_get_timing: ms_channelizer, timing mode "dominant" -- the span ends behind chz12_kernel, IN FRONT of the power
kernel, so it shows whether the unchanged kernel is disturbed by what runs behind it), package power and shader clock as bench.py
samples them (its SmiSampler).  The on leg also reads the power ring once per round, outside the timed region, and checks that the
snapshots of two consecutive steps of the same block are there.

usage (GPU box):  python scripts/bench_channel_power.py [reps per round = 1500] [rounds = 3] [warm-up = 60] [--off-only]
  --off-only   only the two off legs: for a library of an earlier revision, which does not know the flag (AMPS_RECC_LIB=... built by
               scripts/ab_build.sh) -- run it in the same job as the working tree's library to compare the flag-off step of the two.
prints one JSON object; numbers from different jobs do not compare (boxes differ by up to 12 %)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from gr_amps_amd import capi

args = [a for a in sys.argv[1:] if not a.startswith("--")]
off_only = "--off-only" in sys.argv[1:]
reps = int(args[0]) if len(args) > 0 else 1500
rounds = int(args[1]) if len(args) > 1 else 3
warm = int(args[2]) if len(args) > 2 else 60
dev = torch.device("cuda:0")


def handle(decim, nw, on):
    wb = {"channels": 1024, "decim": decim, "taps_per_branch": 8, "first_channel": 96}
    kw = {"channel_power": True} if on else {}
    r = capi.Recc(n_channels=832, sps=1536 // decim, max_samples=nw // decim + 72, max_bursts=8192, time_kernels=True, slicer="exact",
                  sync_torch=False, wideband=wb, **kw)
    r.set_timing("dominant")
    return r


def timed(r, block, n):
    """n steps as bench.py's timed region runs them: the records of step i are collected while step i + 1 runs"""
    r.timing(reset=True)
    smi = bench.SmiSampler(0, period=0.1)
    smi.start()
    torch.cuda.synchronize()
    nrec = 0
    t0 = time.perf_counter()
    for i in range(n):
        r.push_wideband(block)
        if i:
            nrec += len(r.drain_end(copy=False))
        r.drain_begin()
    nrec += len(r.drain_end(copy=False))
    el = time.perf_counter() - t0
    t = r.timing()
    smi.stop()
    return el / n * 1e3, t["ms_channelizer"] / max(1, t["launches_channelizer"]), nrec, smi.samples


out = {"library": os.path.relpath(capi.LIB_PATH, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "reps_per_round": reps, "rounds": rounds, "warmup": warm, "device": torch.cuda.get_device_name(0), "steps": {}}
for decim in (768, 512):
    nw = (1 << 27) if decim == 512 else 11 * 256 * 64 * 768
    x, planted = bench.make_wideband_batch(torch, dev, nw, 96, 832, 2, seed=1)
    bench._WIDEBAND_CACHE.clear()
    torch.cuda.synchronize()
    legs = {"off_a": handle(decim, nw, False)}
    if not off_only:
        legs["on"] = handle(decim, nw, True)
    legs["off_b"] = handle(decim, nw, False)
    step_ms = {k: [] for k in legs}
    chz_ms = {k: [] for k in legs}
    recs = {k: 0 for k in legs}
    power = {k: [] for k in legs}
    for r in legs.values():
        for _ in range(warm):
            r.push_wideband(x)
            r.drain(copy=False)
    ring = None
    for rd in range(rounds):
        for k, r in legs.items():
            s, c, n, p = timed(r, x, reps)
            step_ms[k].append(s)
            chz_ms[k].append(c)
            recs[k] += n
            power[k] += p
        if "on" in legs:
            # outside the timed region: the block repeats and a step is a whole number of snapshot strides, so consecutive steps leave
            # the same snapshots
            P, first = legs["on"].channel_power()
            per_step = nw // decim // capi.POWER_STRIDE
            k = min(per_step, P.shape[1] - per_step)                     # the ring holds one step and (part of) the one before it
            assert P.shape[0] == 832 and k > 0 and np.isfinite(P).all() and P.max() > 0.0
            ring = {"snapshots_held": int(P.shape[1]), "snapshots_per_step": int(per_step), "ring_snaps": legs["on"].power_ring_snaps,
                    "mean_power": float(P.mean()), "compared": int(k),
                    "consecutive_steps_equal": bool(np.array_equal(P[:, -k:], P[:, -per_step - k:-per_step]))}
    for r in legs.values():
        r.close()
    step = {"samples": nw, "frames_per_step": nw // decim, "bursts_planted": len(planted),
            "records_per_step": {k: v / (reps * rounds) for k, v in recs.items()}}
    for k in legs:
        step[k] = {"step_ms": round(float(np.mean(step_ms[k])), 4), "step_ms_per_round": [round(v, 4) for v in step_ms[k]],
                   "filter_bank_kernel_ms": round(float(np.mean(chz_ms[k])), 4), "filter_bank_kernel_ms_per_round": [round(v, 4) for v in chz_ms[k]],
                   "package_w": round(float(np.mean([p[0] for p in power[k]])), 1) if power[k] else None,
                   "sclk_mhz": round(float(np.mean([p[1] for p in power[k]])), 1) if power[k] else None}
    for key in ("step_ms", "filter_bank_kernel_ms"):
        ref = 0.5 * (step["off_a"][key] + step["off_b"][key])
        spread = abs(step["off_a"][key] - step["off_b"][key])
        step[key + "_off_mean"] = round(ref, 4)
        step[key + "_off_spread"] = round(spread, 4)
        step[key + "_off_spread_rel"] = round(spread / ref, 4)
        per_round = step["off_a"][key + "_per_round"] + step["off_b"][key + "_per_round"]
        step[key + "_off_range"] = [min(per_round), max(per_round)]         # every round of either off leg
        if "on" in legs:
            step[key + "_on_minus_off"] = round(step["on"][key] - ref, 4)
            step[key + "_on_vs_off"] = round(step["on"][key] / ref - 1.0, 4)
            step[key + "_on_inside_off_spread"] = bool(min(per_round) <= step["on"][key] <= max(per_round))
    if ring:
        step["ring"] = ring
    out["steps"]["D%d" % decim] = step
    del x, legs
    torch.cuda.empty_cache()
print(json.dumps(out, indent=1))
