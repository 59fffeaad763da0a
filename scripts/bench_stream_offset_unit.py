"""What AMPS_RECC_FLAG_STREAM_OFFSET_UNIT costs the IQ and translate seams beside AMPS_RECC_FLAG_STREAM_OFFSET, measured in ONE process,
in the shape of scripts/bench_stream_offset.py.  Two workloads, each a push plus a drain per step on a device-resident block:
  (a) subband21   one second of 21 centres 30 kHz apart out of a 2.4 Msps cu8 stream at / 12: 200 000 channel-rate samples x 21 rows
                  per step
  (b) direct832   bench.py's direct832 step: 832 channels x 2^18 samples at 200 ksps through amps_recc_push_iq
Per workload the legs run in ROUNDS (default two), each round `reps` steps of every leg back to back:
  off_a, amp, unit, off_b  -- amp: the shipped statistic (stream_offset=True), unit: the unit-amplitude one (stream_offset="unit"); the
                         off leg runs twice per round, first and last, so that its own spread inside the job is on record beside
                         every difference (two handles of the same build, the same block).
Per leg: step ms on the host clock over the leg's steps, stream synchronised at both ends.  The yardstick on paper: the flag adds one
read of 8 B per channel-rate sample and one float2 per 256 samples -- (a) 33.6 MB, which the translate stage has just written and
which fits the L2 / MALL, (b) 1.74 GB from HBM: what AMPS_RECC_FLAG_STREAM_POWER adds.  The on leg reads the ring once
per round, outside the timed region.  The unit kernel reads the same bytes as its sibling and adds per sample one frexp, two ldexp, a
multiply, an fma, one reciprocal square root and two multiplies.

usage (GPU box):  python scripts/bench_stream_offset_unit.py [reps per round = 300] [rounds = 2] [warm-up = 20] [--off-only]
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
reps = int(args[0]) if len(args) > 0 else 300
rounds = int(args[1]) if len(args) > 1 else 2
warm = int(args[2]) if len(args) > 2 else 20
dev = torch.device("cuda:0")
torch.manual_seed(1)


def subband21():
    rate, decim = 2.4e6, 12
    n = int(rate)
    centres = [-300e3 + 30e3 * i for i in range(21)]
    block = torch.randint(0, 256, (n, 2), dtype=torch.uint8, device=dev)

    def handle(on):
        r = capi.Recc(n_channels=21, sps=10, max_samples=n // decim, max_bursts=256, sync_torch=False, **({"stream_offset": on} if on else {}))
        r.set_xlate_shared(rate, centres, decim)
        return r
    return handle, (lambda r: r.push_raw_shared_as(block, capi.SAMPLES_CU8)), 21, n // decim


def direct832():
    C, N = 832, 1 << 18
    batch, _, expected = bench.make_batch(torch, dev, C, N, 10, seed=1)

    def handle(on):
        return capi.Recc(n_channels=C, sps=10, max_samples=N, max_bursts=max(4096, 2 * expected), slicer="exact", sync_torch=False,
                         **({"stream_offset": on} if on else {}))
    return handle, (lambda r: r.push_iq(batch)), C, N


def timed(r, push, n):
    torch.cuda.synchronize()
    nrec = 0
    t0 = time.perf_counter()
    for _ in range(n):
        push(r)
        nrec += len(r.drain(copy=False))
    return (time.perf_counter() - t0) / n * 1e3, nrec


out = {"library": os.path.relpath(capi.LIB_PATH, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "reps_per_round": reps, "rounds": rounds,
       "warmup": warm, "device": torch.cuda.get_device_name(0), "steps": {}}
for name, make in (("subband21", subband21), ("direct832", direct832)):
    handle, push, C, per_step = make()
    torch.cuda.synchronize()
    legs = {"off_a": handle(False)}
    if not off_only:
        legs["amp"] = handle(True)
        legs["unit"] = handle("unit")
    legs["off_b"] = handle(False)
    step_ms = {k: [] for k in legs}
    recs = {k: 0 for k in legs}
    for r in legs.values():
        for _ in range(warm):
            push(r)
            r.drain(copy=False)
    ring = None
    for rd in range(rounds):
        for k, r in legs.items():
            s, n = timed(r, push, reps)
            step_ms[k].append(s)
            recs[k] += n
        if "unit" in legs:                                            # outside the timed region
            A, first = legs["unit"].channel_autocorr()
            assert A.shape[0] == C and A.shape[1] > 0 and np.isfinite(A.view(np.float32)).all() and 0.0 < np.abs(A).max() <= 1.0 + 2e-5
            ring = {"blocks_held": int(A.shape[1]), "first_block": int(first), "ring_blocks": legs["unit"].autocorr_ring_blocks,
                    "mean_abs": float(np.abs(A).mean())}
    for r in legs.values():
        r.close()
    step = {"rows": C, "channel_rate_samples_per_step": per_step, "extra_read_bytes_per_step": 8 * C * per_step,
            "records_per_step": {k: v / (reps * rounds) for k, v in recs.items()}}
    for k in legs:
        step[k] = {"step_ms": round(float(np.mean(step_ms[k])), 4), "step_ms_per_round": [round(v, 4) for v in step_ms[k]]}
    ref = 0.5 * (step["off_a"]["step_ms"] + step["off_b"]["step_ms"])
    spread = abs(step["off_a"]["step_ms"] - step["off_b"]["step_ms"])
    per_round = step["off_a"]["step_ms_per_round"] + step["off_b"]["step_ms_per_round"]
    step["step_ms_off_mean"] = round(ref, 4)
    step["step_ms_off_spread"] = round(spread, 4)
    step["step_ms_off_spread_rel"] = round(spread / ref, 4)
    step["step_ms_off_range"] = [min(per_round), max(per_round)]      # every round of either off leg
    for k in ("amp", "unit"):
        if k in legs:
            d = step[k]["step_ms"] - ref
            step["step_ms_%s_minus_off" % k] = round(d, 4)
            step["step_ms_%s_vs_off" % k] = round(d / ref, 4)
            step["extra_read_gb_per_s_%s" % k] = round(8 * C * per_step / (d * 1e-3) / 1e9, 1) if d > 0 else None
    if "unit" in legs:
        step["ring"] = ring
    out["steps"][name] = step
    del legs, handle, push
    torch.cuda.empty_cache()
print(json.dumps(out, indent=1))
