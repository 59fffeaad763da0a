"""What AMPS_RECC_FLAG_EARLY_MESSAGES costs and what it buys, measured in ONE process.

cost   The flag adds two small launches behind every resolve (recc_early_wave_kernel, one wave per channel, and recc_early_scan_kernel,
       one workgroup).  Legs off_a, on, off_b -- three handles of the same build on the same block, `reps` steps of each leg back to
       back per round, the off leg first and last so that its own spread inside the job stands beside every difference -- on
         wideband D768 / D512   the bench's wideband step (bench.py: 138 412 032 samples at D = 768, 2^27 at D = 512, 832 channels)
         direct832              the bench's IQ-seam step (832 channels x 2^18 samples)
         block20ms D768 / D512  a device-resident 20 ms block of the full band (614 400 samples) with the block's bursts in flight: the
                                step a real-time caller runs, where a launch weighs the most
       Steps are timed as bench.py times them: records collected one step behind with the split drain, host clock over the leg.  The
       off legs run the parent's kernels (profiles/early_messages/isa_identity.txt).
gain   Host-resident blocks of 2 ms and of 20 ms, as an SDR delivers them: the 21 control channels of system A from one 2.4 Msps cu8
       stream decimated by 12, one mobile per channel sending a page response (2 words), a registration (3) or an origination with
       seven digits (4) whose carrier ends behind its last word.  After every push the early messages and the records are drained;
       per message length: stream time from the trigger (position) to the drained early message and to the drained record, in
       milliseconds of stream, beside the rule's 24 ms per word + 0.93 ms and 169 ms + at most one block; and the host clock from the
       push call to the return of drain_early().

usage (GPU box):  python scripts/bench_early_messages.py [out = profiles/early_messages/early_messages.txt] [reps = 40] [rounds = 3] [warm-up = 10]
writes one JSON object to `out` and prints it; numbers from different jobs do not compare (boxes differ by up to 12 %)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from gr_amps_amd import capi, synth

args = sys.argv[1:]
path = args[0] if len(args) > 0 else os.path.join(ROOT, "profiles", "early_messages", "early_messages.txt")
reps = int(args[1]) if len(args) > 1 else 40
rounds = int(args[2]) if len(args) > 2 else 3
warm = int(args[3]) if len(args) > 3 else 10
dev = torch.device("cuda:0")
out = {"library": os.path.relpath(capi.LIB_PATH, ROOT), "device": torch.cuda.get_device_name(0)}


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


def drained(r):
    try:                                                       # a full list only drops events, the kernels run all the same
        return len(r.drain_early())
    except capi.AmpsError as e:
        return len(e.early)


def legs_of(make, push_of, reps, rounds, warm):
    legs = {"off_a": make(False), "on": make(True), "off_b": make(False)}
    ms = {k: [] for k in legs}
    recs = {k: 0 for k in legs}
    for r in legs.values():
        for _ in range(warm):
            push_of(r)()
            r.drain(copy=False)
    events = drained(legs["on"])
    for _ in range(rounds):
        for k, r in legs.items():
            s, n = timed(r, push_of(r), reps)
            ms[k].append(s)
            recs[k] += n
        events += drained(legs["on"])                          # outside the timed region
    for r in legs.values():
        r.close()
    res = {k: {"step_ms": round(float(np.mean(v)), 5), "step_ms_per_round": [round(x, 5) for x in v]} for k, v in ms.items()}
    ref = 0.5 * (res["off_a"]["step_ms"] + res["off_b"]["step_ms"])
    per_round = ms["off_a"] + ms["off_b"]
    res.update(reps_per_round=reps, rounds=rounds, records_per_step={k: v / (reps * rounds) for k, v in recs.items()}, early_messages_drained=events,
               off_mean_ms=round(ref, 5), off_spread_ms=round(abs(res["off_a"]["step_ms"] - res["off_b"]["step_ms"]), 5),
               off_range_ms=[round(min(per_round), 5), round(max(per_round), 5)],
               on_minus_off_us=round((res["on"]["step_ms"] - ref) * 1e3, 3), on_vs_off=round(res["on"]["step_ms"] / ref - 1.0, 5),
               on_inside_off_range=bool(min(per_round) <= res["on"]["step_ms"] <= max(per_round)))
    return res


# ------------------------------------------------------------------------------------------------------------------------------ cost
out["cost"] = {}
for decim in (768, 512):
    wb = {"channels": 1024, "decim": decim, "taps_per_branch": 8, "first_channel": 96}
    nw = (1 << 27) if decim == 512 else 11 * 256 * 64 * 768
    x, planted = bench.make_wideband_batch(torch, dev, nw, 96, 832, 2, seed=1)
    bench._WIDEBAND_CACHE.clear()
    torch.cuda.synchronize()
    make = lambda on, n=nw: capi.Recc(n_channels=832, sps=1536 // decim, max_samples=n // decim + 72, max_bursts=8192, slicer="exact",
                                      sync_torch=False, wideband=wb, early_messages=on)
    step = legs_of(make, lambda r: (lambda: r.push_wideband(x)), reps, rounds, warm)
    step.update(samples=nw, bursts_planted=len(planted))
    out["cost"]["wideband_D%d" % decim] = step
    blk = x[:614400].clone()                                   # 20 ms of the same band: its bursts begin and never end, captures stay in flight
    torch.cuda.synchronize()
    step = legs_of(lambda on: make(on, 614400), lambda r: (lambda: r.push_wideband(blk)), reps * 50, rounds, warm * 10)
    step.update(samples=614400)
    out["cost"]["block20ms_D%d" % decim] = step
    del x, blk
    torch.cuda.empty_cache()
batch, _, expected = bench.make_batch(torch, dev, 832, 1 << 18, 10, seed=1)
torch.cuda.synchronize()
make = lambda on: capi.Recc(n_channels=832, sps=10, max_samples=1 << 18, max_bursts=max(4096, 2 * expected), slicer="exact", sync_torch=False,
                            early_messages=on)
step = legs_of(make, lambda r: (lambda: r.push_iq(batch)), reps * 10, rounds, warm)
step.update(samples_per_channel=1 << 18, bursts_planted=expected)
out["cost"]["direct832"] = step
del batch
torch.cuda.empty_cache()

# ------------------------------------------------------------------------------------------------------------------------------ gain
RATE, DECIM, SPS_IN = 2.4e6, 12, 120                           # 200 ksps per channel, ten samples per symbol
tuned = capi.reverse_channel_hz(323) + 15e3                    # between two channels: none on the tuner's DC
centres = capi.control_channel_centers("A", tuned)
n = 4800 * 250                                                 # 0.5 s of stream
k = np.arange(n)
x = np.zeros(n, np.complex128)
rng = np.random.default_rng(9100)
KINDS = (("page_response", ""), ("registration", ""), ("origination", "5551234"))
for c, fc in enumerate(centres):                               # one seizure per channel, 15 ms apart
    kind, dialed = KINDS[c % 3]
    words = synth.make_message(kind, "".join(str(int(d)) for d in rng.integers(0, 10, 10)), int(rng.integers(0, 2 ** 32)), dialed)
    bits = synth.burst_bits(words, dcc=int(rng.integers(0, 4)), pad_words=False)
    iq = synth.fsk_modulate(n, [(12000 + 36000 * c, bits)], sps=SPS_IN, fs=20e3 * SPS_IN, snr_db=40.0, rng=rng)
    x += iq * np.exp(2j * np.pi * fc * k / RATE)
q = np.clip(np.floor(np.stack([x.real, x.imag], -1) * 4.0 + 128.0), 0, 255).astype(np.uint8)
out["gain"] = {"channels": len(centres), "input": "host memory (numpy cu8), staged by the library inside the push", "rule_ms": {
    str(w): round((10 * (15 + 480 * w) + 36) / 200.0, 3) for w in (2, 3, 4)}, "rule_record_ms": round((10 * 3375 + 36) / 200.0, 3)}
for block_ms in (2, 20):
    BLOCK = int(RATE * block_ms * 1e-3)
    parts = [np.ascontiguousarray(q[o:o + BLOCK]) for o in range(0, n, BLOCK)]
    with capi.Recc(n_channels=len(centres), sps=10, max_samples=BLOCK // DECIM + 8, max_bursts=256, early_messages=True) as r:
        r.set_xlate_shared(RATE, centres, DECIM)
        msg, rec, words_of, lat = {}, {}, {}, []
        for blk in parts:
            t0 = time.perf_counter()
            r.push_raw_shared_as(blk, capi.SAMPLES_CU8)
            ev = r.drain_early()
            lat.append(time.perf_counter() - t0)
            recs = r.drain()
            produced = r.debug_slicer_bits(0, 0)[1]
            for e in ev:
                key = (int(e["rec"]["channel"]), int(e["rec"]["position"]))
                assert int(e["found_at"]) == produced
                msg[key], words_of[key] = (produced - key[1]) / 200.0, int(e["n_words"])
            for R in recs:
                rec[(int(R["channel"]), int(R["position"]))] = (produced - int(R["position"])) / 200.0
    res = {"block_samples": BLOCK, "block_channel_samples": BLOCK // DECIM, "blocks": len(parts), "records": len(rec), "early_messages": len(msg),
           "push_to_drain_early_us": {"median": round(float(np.median(lat[5:]) * 1e6), 1), "p99": round(float(np.percentile(lat[5:], 99) * 1e6), 1)}}
    for w in (2, 3, 4):
        keys = [key for key in msg if words_of[key] == w and key in rec]
        m, d = [msg[key] for key in keys], [rec[key] for key in keys]
        res["words_%d" % w] = {"mobiles": len(keys),
                               "trigger_to_early_ms": {"min": round(min(m), 3), "median": round(float(np.median(m)), 3), "max": round(max(m), 3)} if m else None,
                               "trigger_to_record_ms": {"min": round(min(d), 3), "median": round(float(np.median(d)), 3), "max": round(max(d), 3)} if d else None}
    out["gain"]["blocks_%dms" % block_ms] = res

text = json.dumps(out, indent=1)
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
with open(path, "w") as f:
    f.write(text + "\n")
print(text)
