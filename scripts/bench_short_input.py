"""A/B of the wideband seam's two block formats in ONE process: fc32 (amps_recc_push_wideband) against 16-bit I/Q
(amps_recc_push_wideband_short), the latter both ways the library can consume it -- read in place by chz12_short_kernel, and through
the conversion pre-pass in front of the fc32 kernel (AMPS_RECC_SHORT_PREPASS=1, read when a handle is created).

Per decimation the bench's own step (bench.py: 138 412 032 samples at D = 768, 2^27 at D = 512; spec D, device-resident block, the
bench's own signal quantised to int16 and its exact fc32 twin) is pushed in ROUNDS: every round times `reps` launches of each form,
back to back, from amps_recc_get_timing (ms_channelizer, timing mode "dominant").  The fc32 form is the reference and runs twice per
round (legs A and B, first and last), so its own spread inside the job is on record beside every difference.  Package power and shader
clock are sampled as bench.py samples them (its SmiSampler) while each form runs.  Then host-resident 20 ms blocks (614 400 samples,
full band, D = 512 as in bench.py's realtime_latency): us per block, push + drain, both forms.

usage (GPU box):  python scripts/bench_short_input.py [reps per round = 400] [rounds = 3] [warm-up = 40]
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

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 400
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 40
HBM_PEAK = 8.0e12
dev = torch.device("cuda:0")


def quantise(x):
    """torch complex64 [n] -> (int16 [n, 2], complex64 twin, scale): the largest power-of-two scale that keeps every component below 30 000"""
    v = torch.view_as_real(x)
    peak = float(v.abs().max())
    s = 2.0 ** np.floor(np.log2(30000.0 / peak))
    q = torch.round(v * s).to(torch.int16)
    return q, torch.view_as_complex(q.to(torch.float32).contiguous()), s


def handle(decim, nw, prepass):
    os.environ["AMPS_RECC_SHORT_PREPASS"] = "1" if prepass else "0"          # read by amps_recc_create
    wb = {"channels": 1024, "decim": decim, "taps_per_branch": 8, "first_channel": 96}
    r = capi.Recc(n_channels=832, sps=1536 // decim, max_samples=nw // decim + 72, max_bursts=8192, time_kernels=True, slicer="exact",
                  sync_torch=False, wideband=wb)
    r.set_timing("dominant")
    return r


def timed(r, push, block, n):
    r.timing(reset=True)
    smi = bench.SmiSampler(0, period=0.1)
    smi.start()
    nrec = 0
    for _ in range(n):
        push(block)
        nrec += len(r.drain(copy=False))
    t = r.timing()
    smi.stop()
    p = smi.samples                                                          # (power W, sclk MHz) pairs taken while this form ran
    return t["ms_channelizer"] / max(1, t["launches_channelizer"]), nrec, p


out = {"reps_per_round": reps, "rounds": rounds, "warmup": warm, "device": torch.cuda.get_device_name(0), "steps": {}}
for decim in (768, 512):
    nw = (1 << 27) if decim == 512 else 11 * 256 * 64 * 768
    x, planted = bench.make_wideband_batch(torch, dev, nw, 96, 832, 2, seed=1)
    q, xf, scale = quantise(x)
    del x
    bench._WIDEBAND_CACHE.clear()
    torch.cuda.synchronize()
    forms = {"fc32_a": (handle(decim, nw, False), "push_wideband", xf),
             "sc16_direct": (handle(decim, nw, False), "push_wideband_short", q),
             "sc16_prepass": (handle(decim, nw, True), "push_wideband_short", q),
             "fc32_b": (handle(decim, nw, False), "push_wideband", xf)}
    os.environ["AMPS_RECC_SHORT_PREPASS"] = "0"
    ms = {k: [] for k in forms}
    recs = {k: 0 for k in forms}
    power = {k: [] for k in forms}
    for k, (r, push, blk) in forms.items():
        for _ in range(warm):
            getattr(r, push)(blk)
            r.drain(copy=False)
    for rd in range(rounds):
        for k, (r, push, blk) in forms.items():
            m, n, p = timed(r, getattr(r, push), blk, reps)
            ms[k].append(m)
            recs[k] += n
            power[k] += p
    for r, _, _ in forms.values():
        r.close()
    step = {"samples": nw, "scale": scale, "bursts_planted": len(planted), "records_per_step": {k: v / (reps * rounds) for k, v in recs.items()}}
    for k in forms:
        bps = 8 if k.startswith("fc32") else 4
        mean = float(np.mean(ms[k]))
        step[k] = {"ms_per_step": round(mean, 4), "ms_per_round": [round(v, 4) for v in ms[k]], "bytes_per_sample": bps,
                   "gb_per_s": round(nw * bps / mean / 1e6, 1), "fraction_of_8_tb_per_s": round(nw * bps / (mean * 1e-3) / HBM_PEAK, 4),
                   "package_w": round(float(np.mean([p[0] for p in power[k]])), 1) if power[k] else None,
                   "sclk_mhz": round(float(np.mean([p[1] for p in power[k]])), 1) if power[k] else None}
    ref = 0.5 * (step["fc32_a"]["ms_per_step"] + step["fc32_b"]["ms_per_step"])
    step["fc32_spread_ms"] = round(abs(step["fc32_a"]["ms_per_step"] - step["fc32_b"]["ms_per_step"]), 4)
    step["fc32_spread_rel"] = round(step["fc32_spread_ms"] / ref, 4)
    step["sc16_direct_vs_fc32"] = round(step["sc16_direct"]["ms_per_step"] / ref - 1.0, 4)
    step["sc16_prepass_vs_fc32"] = round(step["sc16_prepass"]["ms_per_step"] / ref - 1.0, 4)
    step["sc16_direct_vs_prepass"] = round(step["sc16_direct"]["ms_per_step"] / step["sc16_prepass"]["ms_per_step"] - 1.0, 4)
    out["steps"]["D%d" % decim] = step
    del q, xf, forms
    torch.cuda.empty_cache()

# host-resident 20 ms blocks, as bench.py's realtime_latency pushes them
nw, blocks = 614400, 200
rng = np.random.default_rng(3)
base = rng.standard_normal((8, nw, 2)).astype(np.float32) * 0.05
wq = np.rint(base * 8192.0).astype(np.int16)                                 # |component| < 30 000 at 0.05 sigma x 8192 (checked below)
assert np.abs(base).max() * 8192.0 < 30000
wf = np.ascontiguousarray(wq.astype(np.float32)).view(np.complex64)[..., 0]
lat = {}
for name, push, data in (("fc32", "push_wideband", wf), ("sc16", "push_wideband_short", wq), ("fc32_again", "push_wideband", wf)):
    wb = {"channels": 1024, "decim": 512, "taps_per_branch": 8, "first_channel": 96}
    with capi.Recc(n_channels=832, sps=3, max_samples=nw // 512 + 72, max_bursts=4096, slicer="exact", wideband=wb) as r:
        t = []
        for k in range(blocks + 10):
            t0 = time.perf_counter()
            getattr(r, push)(data[k % 8])
            r.drain(copy=False)
            t.append(time.perf_counter() - t0)
    t = np.array(t[10:]) * 1e6
    lat[name] = {"median_us": round(float(np.median(t)), 1), "p99_us": round(float(np.percentile(t, 99)), 1), "bytes_per_block": int(data[0].nbytes)}
out["host_blocks_20ms"] = lat
print(json.dumps(out, indent=1))
