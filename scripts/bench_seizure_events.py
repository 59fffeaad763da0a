"""What AMPS_RECC_FLAG_SEIZURE_EVENTS costs and what it buys, measured in ONE process.

cost     The flag adds one small launch (recc_seizure_kernel, one workgroup) behind every resolve.  Legs off_a, on, off_b -- three
         handles of the same build on the same block, `reps` steps of each leg back to back per round, the off leg first and last so
         that its own spread inside the job stands beside every difference -- on
           wideband D768 / D512   the bench's wideband step (bench.py: 138 412 032 samples at D = 768, 2^27 at D = 512, 832 channels)
           direct832              the bench's IQ-seam step (832 channels x 2^18 samples)
           block20ms D768 / D512  a device-resident 20 ms block of the full band (614 400 samples): the step a real-time caller runs,
                                  where one launch weighs the most
         Steps are timed as bench.py times them: records collected one step behind with the split drain, host clock over the leg.
latency  Host-resident 2 ms blocks, as an SDR delivers them: the 21 control channels of system A from one 2.4 Msps cu8 stream
         decimated by 12.  Per block, host clock from the push call to the return of drain_seizures() on a handle with the flag, and
         from the push call to the return of drain() on a handle without it, on the same 500 blocks; and for every event the
         stream-side delay found_at - position in milliseconds.

usage (GPU box):  python scripts/bench_seizure_events.py cost [reps = 40] [rounds = 3] [warm-up = 10]
                  python scripts/bench_seizure_events.py latency [blocks = 500]
prints one JSON object; numbers from different jobs do not compare (boxes differ by up to 12 %)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
from gr_amps_amd import capi, synth

what = sys.argv[1] if len(sys.argv) > 1 else "cost"
args = sys.argv[2:]
dev = torch.device("cuda:0")
out = {"library": os.path.relpath(capi.LIB_PATH, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "device": torch.cuda.get_device_name(0)}


def timed(r, push, n):
    """n steps as bench.py's timed region runs them: the records of step i are collected while step i + 1 runs"""
    torch.cuda.synchronize()
    nrec = 0
    t0 = time.perf_counter()
    for i in range(n):
        push()
        if i:
            nrec += len(r.drain_end(copy=False))
        r.drain_begin()
    nrec += len(r.drain_end(copy=False))
    return (time.perf_counter() - t0) / n * 1e3, nrec


def legs_of(make, push_of, reps, rounds, warm):
    legs = {"off_a": make(False), "on": make(True), "off_b": make(False)}
    ms = {k: [] for k in legs}
    recs = {k: 0 for k in legs}
    events = 0
    for r in legs.values():
        for _ in range(warm):
            push_of(r)()
            r.drain(copy=False)
    legs["on"].drain_seizures()
    for _ in range(rounds):
        for k, r in legs.items():
            s, n = timed(r, push_of(r), reps)
            ms[k].append(s)
            recs[k] += n
        try:                                                   # outside the timed region; a full list only drops events, the kernel runs all the same
            events += len(legs["on"].drain_seizures())
        except capi.AmpsError as e:
            events += len(e.seizures)
    for r in legs.values():
        r.close()
    res = {k: {"step_ms": round(float(np.mean(v)), 5), "step_ms_per_round": [round(x, 5) for x in v]} for k, v in ms.items()}
    ref = 0.5 * (res["off_a"]["step_ms"] + res["off_b"]["step_ms"])
    per_round = ms["off_a"] + ms["off_b"]
    res.update(reps_per_round=reps, rounds=rounds, records_per_step={k: v / (reps * rounds) for k, v in recs.items()}, events_drained=events,
               off_mean_ms=round(ref, 5), off_spread_ms=round(abs(res["off_a"]["step_ms"] - res["off_b"]["step_ms"]), 5),
               off_range_ms=[round(min(per_round), 5), round(max(per_round), 5)],
               on_minus_off_us=round((res["on"]["step_ms"] - ref) * 1e3, 3), on_vs_off=round(res["on"]["step_ms"] / ref - 1.0, 5),
               on_inside_off_range=bool(min(per_round) <= res["on"]["step_ms"] <= max(per_round)))
    return res


if what == "cost":
    reps = int(args[0]) if len(args) > 0 else 40
    rounds = int(args[1]) if len(args) > 1 else 3
    warm = int(args[2]) if len(args) > 2 else 10
    out["cost"] = {}
    for decim in (768, 512):
        wb = {"channels": 1024, "decim": decim, "taps_per_branch": 8, "first_channel": 96}
        nw = (1 << 27) if decim == 512 else 11 * 256 * 64 * 768
        x, planted = bench.make_wideband_batch(torch, dev, nw, 96, 832, 2, seed=1)
        bench._WIDEBAND_CACHE.clear()
        torch.cuda.synchronize()
        make = lambda on, n=nw: capi.Recc(n_channels=832, sps=1536 // decim, max_samples=n // decim + 72, max_bursts=8192, slicer="exact",
                                          sync_torch=False, wideband=wb, seizure_events=on)
        step = legs_of(make, lambda r: (lambda: r.push_wideband(x)), reps, rounds, warm)
        step.update(samples=nw, bursts_planted=len(planted))
        out["cost"]["wideband_D%d" % decim] = step
        blk = x[:614400].clone()                               # 20 ms of the same band
        torch.cuda.synchronize()
        step = legs_of(lambda on: make(on, 614400), lambda r: (lambda: r.push_wideband(blk)), reps * 50, rounds, warm * 10)
        step.update(samples=614400)
        out["cost"]["block20ms_D%d" % decim] = step
        del x, blk
        torch.cuda.empty_cache()
    batch, _, expected = bench.make_batch(torch, dev, 832, 1 << 18, 10, seed=1)
    torch.cuda.synchronize()
    make = lambda on: capi.Recc(n_channels=832, sps=10, max_samples=1 << 18, max_bursts=max(4096, 2 * expected), slicer="exact", sync_torch=False,
                                seizure_events=on)
    step = legs_of(make, lambda r: (lambda: r.push_iq(batch)), reps * 10, rounds, warm)
    step.update(samples_per_channel=1 << 18, bursts_planted=expected)
    out["cost"]["direct832"] = step
else:
    blocks = int(args[0]) if len(args) > 0 else 500
    RATE, DECIM, BLOCK = 2.4e6, 12, 4800                       # 2 ms blocks; 200 ksps per channel
    tuned = capi.reverse_channel_hz(323) + 15e3                # between two channels: none on the tuner's DC
    centres = capi.control_channel_centers("A", tuned)
    n = BLOCK * 250                                            # 0.5 s of stream, pushed twice over
    k = np.arange(n)
    x = np.zeros(n, np.complex128)
    for c, fc in enumerate(centres):                           # one seizure per channel, 15 ms apart
        iq, _ = synth.make_channel_block(n, 1, seed=9000 + c, sps=120, snr_db=40.0, first=12000 + 36000 * c)
        x += iq * np.exp(2j * np.pi * fc * k / RATE)
    q = np.clip(np.floor(np.stack([x.real, x.imag], -1) * 4.0 + 128.0), 0, 255).astype(np.uint8)
    parts = [np.ascontiguousarray(q[o:o + BLOCK]) for o in range(0, n, BLOCK)]
    res = {}
    for on in (True, False, True, False):                      # the two handles alternate, each measured twice
        with capi.Recc(n_channels=len(centres), sps=10, max_samples=BLOCK // DECIM + 8, max_bursts=256, seizure_events=on) as r:
            r.set_xlate_shared(RATE, centres, DECIM)
            lat, delay, got = [], [], 0
            for i in range(blocks + 20):
                blk = parts[i % len(parts)]
                t0 = time.perf_counter()
                r.push_raw_shared_as(blk, capi.SAMPLES_CU8)
                ev = r.drain_seizures() if on else r.drain(copy=False)
                lat.append(time.perf_counter() - t0)
                got += len(ev)
                if on:
                    delay += [(int(e["found_at"]) - int(e["position"])) / 200.0 for e in ev]     # ms at 200 ksps
                    r.drain(copy=False)                        # outside the timed region: the records still leave the handle
            lat = np.array(lat[20:]) * 1e6
            key = "push_to_drain_seizures_us" if on else "push_to_drain_us_flag_off"
            res.setdefault(key, []).append({"median": round(float(np.median(lat)), 1), "p99": round(float(np.percentile(lat, 99)), 1),
                                            "events" if on else "records": got})
            if on:
                res["stream_side_delay_ms"] = {"events": len(delay), "median": round(float(np.median(delay)), 3), "max": round(float(np.max(delay)), 3),
                                               "bound_ms": round((BLOCK // DECIM + 64 + 128) / 200.0, 3)}   # a push of 400 samples processes 384 or 448
    res.update(blocks_timed=blocks, block_ms=2.0, block_samples=BLOCK, channels=len(centres), input="host memory (numpy cu8), staged by the library inside the push")
    out["latency"] = res
print(json.dumps(out, indent=1))
