#!/usr/bin/env python
"""bench.py -- AMPS RECC receive path on MI355X: Manchester symbols demodulated AND decoded per second.

A "step" is one pass of the hot path over one resident batch of synthetic IQ:
    amps_recc_push_wideband / amps_recc_push_iq (device pointer) + amps_recc_drain (records to host).
Inputs are in HBM before the timed region starts.

N > 1: one process per GPU.  `python bench.py --gpus N` with no WORLD_SIZE in the environment starts the N ranks itself
(re-exec under torch.distributed.run on 127.0.0.1); under an external torchrun it uses the ranks it is given.
  --dist bands (default)      every rank owns its own 832-channel band (independent 30 kHz channels / whole bands are the
                              data-parallel axis): no data-path collective, weak scaling, value = all ranks' symbols / max time
  --dist broadcast            ONE band: rank 0 owns the step's wideband block and RCCL broadcasts it (flat ncclBroadcast) to
                              every rank inside the timed region; rank r decodes channel group r of the band
  --dist scatter_allgather    the same distribution as scatter (B/N per peer) + all-gather (every xGMI
                              link carries B/N per phase instead of B)
  --dist broadcast_abi / scatter_allgather_abi
                              the same two distributions issued by the LIBRARY (amps_recc_push_wideband_dist: RCCL inside the C ABI, with
                              its status word and bounded waits); torch.distributed only carries the 128-byte communicator id
  In the two one-band modes the filter bank does not shard (every rank runs the whole fold + FFT):
  value = the band's symbols / max time, "scaling": "strong".

Prints ONE JSON line (rank 0).  See DESIGN.md section 6 for the definitions of roofline / roofline_compute / cpu_baseline.
A plain run measures the headline only (setup, prewarm + warmup, the --steps timed steps, the line); --full adds the other slicer specs,
the other decimation, the secondary workload with its latency record, the CPU baseline, power / clock sampling and, with N > 1, the
one-band passes.  --dump-outputs DIR writes the records of the last timed step as .npy files (inputs are seeded: the same arguments give
the same records).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

ALG_BYTES_PER_SYMBOL_DIRECT = 80.0   # 8 B/sample x 10 samples/symbol, IQ read once
HBM_PEAK_GBPS = 8000.0               # MI355X_MICROARCH.md: 8 TB/s spec (6290 GB/s measured copy ceiling)
FP32_PEAK_TFLOPS = 157.3             # MI355X_MICROARCH.md: peak FP32 vector rate (packed)
SLICERS = {"atan": "A", "product": "B", "sine": "C", "exact": "D"}
# C/N (30 kHz channel) at 1 % seizure-burst loss, scripts/slicer_sensitivity.py on one MI355X (profiles/r04/slicer_sensitivity.txt)
SLICER_SENSITIVITY = {"unit": "dB C/N in 30 kHz at 1 % burst loss", "source": "profiles/r04/slicer_sensitivity.txt (1000 / 1248 bursts per point)",
                      "wideband_seam": {"A": 9.64, "B": 11.68, "C": 13.30, "D": 9.64, "restated_reference_chain": 24.3},
                      "iq_seam_behind_the_flow_graphs_channel_filter": {"A": 10.23, "B": 10.10, "C": 11.20, "D": 10.23, "restated_reference_chain": 24.8},
                      "penalty_vs_A_wideband_dB": {"B": 2.0, "C": 3.7, "D": 0.0}}


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=12000,
                    help="timed steps (default: ~5.5 s of sustained stream, long enough for a power-capped clock to settle and for an external GPU-activity sampler to see it)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", default="wideband832", choices=["wideband832", "direct832", "direct1"],
                    help="wideband832 = BASELINE configs[3] (headline): full band through the channelizer; direct832/direct1 = configs[1] style")
    ap.add_argument("--secondary", default="direct832", choices=["none", "direct832", "direct1", "wideband832"],
                    help="a second workload reported under 'secondary' (N=1 only)")
    ap.add_argument("--slicer", default="default", choices=["default"] + list(SLICERS),
                    help="numeric spec of the slicer (include/amps_recc_numerics.h).  default = whatever a handle created with no slicer flag "
                         "uses (amps_recc_default_slicer(): spec D, the sign of the arctangent discriminator's boxcar sum computed exactly from sign "
                         "bits and the winding number) -- the headline is the product's default path; atan = spec A (the arctangent itself, default of "
                         "rounds 1-3), sine = spec C, product = spec B: opt-in variants, their kernel times are reported under 'other_slicer_specs'")
    ap.add_argument("--dist", default="bands", choices=["bands", "broadcast", "scatter_allgather", "broadcast_abi", "scatter_allgather_abi"],
                    help="bands (default): one 832-channel band per GPU, no data-path collective.  broadcast / scatter_allgather: ONE band, rank 0's block "
                         "distributed every step through torch.distributed (RCCL), channel groups per rank.  broadcast_abi / scatter_allgather_abi: the same "
                         "distributions issued by the library itself (amps_recc_push_wideband_dist: the collectives on the library's own stream behind a status "
                         "word, bounded waits; torch.distributed only carries the 128-byte communicator id)")
    ap.add_argument("--optional-pass-timeout", type=float, default=240.0,
                    help="N > 1: seconds the optional one-band passes behind the headline may take before the line is printed without them")
    ap.add_argument("--groups", type=int, default=0, choices=[0, 2, 4, 8],
                    help="N = 1 only: run wideband832 as ONE rank of the one-band split over that many GPUs (cfg.wideband_groups: the rank decodes one "
                         "interleaved channel group and skips the last FFT pass and the slicer for the others' bins) -- the per-rank kernel time of --dist broadcast")
    ap.add_argument("--decim", default="default", choices=["default", "512", "768"],
                    help="wideband832: input samples per filter-bank frame -- 512 (2x oversampled, 3 samples per symbol) or 768 (4/3 x oversampled, 2 samples "
                         "per symbol; DESIGN.md 4.2b); default = what the library uses when the caller does not say (amps_recc_default_wideband_decim)")
    ap.add_argument("--no-other-decim", action="store_true", help="skip the pass of the same workload at the other decimation")
    ap.add_argument("--samples", type=int, default=0, help="per-channel samples per step (0 = workload default)")
    ap.add_argument("--taps", type=int, default=8, choices=[8], help="wideband832: prototype taps per polyphase branch")
    ap.add_argument("--prewarm-ms", type=float, default=400.0, help="untimed clock-settling run of the same step before the warmup steps")
    ap.add_argument("--no-pipeline", action="store_true", help="drain synchronously after every push instead of one step behind")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-power-sample", action="store_true", help="do not sample package power / shader clock with rocm-smi during the timed region")
    ap.add_argument("--no-other-specs", action="store_true", help="skip the short runs of the other slicer specs")
    ap.add_argument("--no-latency", action="store_true", help="skip the 20 ms-block real-time latency run (scripts/profile_round.sh: its small launches would dilute the per-kernel profile means)")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure: the other slicer specs, the other decimation, the secondary workload and its "
                         "real-time latency record, the CPU baseline, package power / clocks around the timed region and, with N > 1, the one-band "
                         "passes behind the headline (the --no-* options above select among them).  Without it a run sets up, warms up, times "
                         "--steps steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the records the last timed step drained, one float64 array per field, as DIR/records_<field>.npy "
                         "(position as records_position_in_step: samples from the first sample of that step's push)")
    return ap.parse_args(argv)


# ----------------------------------------------------------------------------------------------------- ranks
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def spawn_command(n, argv):
    """the torchrun command line `python bench.py --gpus n ...` re-executes itself under (one rank per GPU, 127.0.0.1)"""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % n,
            "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.join(ROOT, "bench.py")] + list(argv)


def ensure_world(a, argv):
    """`--gpus N` without a launcher: start the N ranks ourselves and relay their exit code."""
    if a.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "1")
    sys.stdout.flush()
    raise SystemExit(subprocess.call(spawn_command(a.gpus, argv), env=env))


def plumbing_only(a):
    """AMPS_BENCH_CPU_PLUMBING=1: the rank plumbing of this file on a box without GPUs (gloo): rendezvous, barrier, max-over-
    ranks reduction and the rank-0 JSON line -- what tests/test_cpu_bench.py checks for `--gpus 2`."""
    import torch
    import torch.distributed as dist
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    t = torch.tensor([float(rank + 1)], dtype=torch.float64)
    if world > 1:
        dist.barrier()
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"plumbing_only": True, "n_gpus": world, "max_over_ranks": float(t.item()), "dist": a.dist}), flush=True)


# ----------------------------------------------------------------------------------------------------- inputs
def make_batch(torch, dev, C, N, sps, seed):
    """C channels x N samples of config-1 style IQ (CPFSK seizure bursts in AWGN) resident on `dev`.
    A base set of distinct channels is synthesised on the CPU and tiled across the band."""
    from gr_amps_amd import synth
    base = min(C, 16)
    nb = max(1, N // 90000)
    iq, per_base = [], []
    for c in range(base):
        x, t = synth.make_channel_block(N, nb, seed=seed * 1000 + c, sps=sps)
        iq.append(x)
        per_base.append(len(t))
    iq = np.stack(iq)
    d = torch.from_numpy(iq).to(dev)
    reps = (C + base - 1) // base
    d = d.repeat(reps, 1)[:C].contiguous()
    expected = sum(per_base[c % base] for c in range(C))   # records per step
    return d, iq, expected


_WIDEBAND_CACHE = {}


def make_wideband_batch(torch, dev, nsamp, first_bin, n_channels, every, seed, build=True):
    """One wideband block (fs = 30.72 Msps, 1024 x 30 kHz) on `dev`: one random seizure burst in every
    `every`-th active channel at a random offset, AWGN at 30 dB SNR in a channel's 60 kHz.  Built on the GPU
    (torch is plumbing here): phase = cumsum(f_dev(t)) + 2 pi f_c t.  Returns (complex64 [nsamp], {channel: (MIN, words36)}).
    build = False: only what was planted (the same random draws) and an UNINITIALISED block of the right shape -- the ranks of a one-band
    run that never read their own copy (rank 0's travels to them) skip the synthesis.  The loop makes no host synchronisation (all
    symbols go up in one copy, sizes are passed explicitly): N ranks sharing one GPU in the rehearsals would otherwise pay a context
    switch per burst.  The last block is kept: the one-band passes behind the headline reuse it."""
    from gr_amps_amd import synth, synth_wideband as sw
    key = (str(dev), nsamp, first_bin, n_channels, every, seed, build)
    if key in _WIDEBAND_CACHE:
        return _WIDEBAND_CACHE[key]
    rng = np.random.default_rng(seed)
    fs = sw.FS_WIDE
    sps_w = 1536
    blen = 3456 * sps_w
    planted, plan, syms = {}, [], []
    for c in range(0, n_channels, every):
        k = (first_bin + c) % 1024
        _, min10, _, _, words = synth.random_message(rng)
        sym = synth.manchester(synth.burst_bits(words, dcc=int(rng.integers(0, 4)), rng=rng)).astype(np.float32) * 2 - 1
        off = int(rng.integers(1000, nsamp - blen - 1000))
        plan.append((k, off, float(rng.uniform(0, 2 * np.pi))))
        syms.append(sym)
        planted[c] = (min10, words)
    if not build:
        out = (torch.empty(nsamp, dtype=torch.complex64, device=dev), planted)
    else:
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        sigma = 10.0 ** (-30.0 / 20.0) / np.sqrt(2.0) * np.sqrt(fs / 60e3)
        x = torch.randn(nsamp, 2, device=dev, generator=g, dtype=torch.float32) * float(sigma)
        x = torch.view_as_complex(x)
        if syms:
            sd = torch.from_numpy(np.stack(syms)).to(dev) * (2 * np.pi * 8e3 / fs)      # [bursts][3456], one copy
            for i, (k, off, ph0) in enumerate(plan):
                f = sd[i].repeat_interleave(sps_w, output_size=blen)
                fc = 2 * np.pi * sw.bin_freq(k) / fs
                ph = torch.cumsum(f.double() + fc, 0) + ph0 + fc * off
                x[off:off + blen] += torch.polar(torch.ones_like(ph, dtype=torch.float32), ph.remainder(2 * np.pi).float())
        out = (x.contiguous(), planted)
    _WIDEBAND_CACHE.clear()
    _WIDEBAND_CACHE[key] = out
    return out


# ----------------------------------------------------------------------------------------------------- --dump-outputs
DUMP_LIMIT_BYTES = 64 << 20


def record_arrays(recs, position_origin=0):
    """The records of one drain (amps_recc_burst_t, sorted by channel and position) as {name: float64 array}, one per field, padding left
    out: a field of shape S holds [n_records, *S]; the text fields (min, dialed) are their bytes; position becomes position_in_step, the
    sample index counted from `position_origin`.  More than DUMP_LIMIT_BYTES in all: a fixed, seeded sample of the records, in their
    order, whose indices are under `rows`."""
    n = len(recs)
    names = [f for f in recs.dtype.names if not f.startswith("_")]
    per_record = sum(8 * max(1, int(np.prod(recs.dtype[f].shape)) * (recs.dtype[f].itemsize if recs.dtype[f].kind == "S" else 1)) for f in names)
    out = {}
    if n * per_record > DUMP_LIMIT_BYTES:
        rows = np.sort(np.random.default_rng(0).choice(n, DUMP_LIMIT_BYTES // per_record - 1, replace=False))
        recs = recs[rows]
        out["rows"] = rows.astype(np.float64)
    for f in names:
        v = recs[f]
        if v.dtype.kind == "S":
            v = np.ascontiguousarray(v).view(np.uint8).reshape(len(recs), -1)
        if f == "position":
            out["position_in_step"] = v.astype(np.int64).astype(np.float64) - float(position_origin)
        else:
            out[f] = v.astype(np.float64)
    return out


def dump_records(d, recs, position_origin):
    os.makedirs(d, exist_ok=True)
    for k, v in record_arrays(recs, position_origin).items():
        np.save(os.path.join(d, "records_%s.npy" % k), v)


# ----------------------------------------------------------------------------------------------------- CPU baseline
def cpu_baseline(iq_base, sps, budget_s):
    """Reference CPU chain (oracle restatement: quadrature demod -> M&M clock recovery -> slicer ->
    recc trigger search/capture -> Manchester -> BCH -> parse), single thread, on a bounded sample of
    the same workload; then all host cores with one channel per thread."""
    import oracle
    from concurrent.futures import ThreadPoolExecutor
    n = iq_base.shape[1]
    t0 = time.perf_counter()
    done = 0
    k = 0
    while True:
        oracle.chain_iq200(iq_base[k % iq_base.shape[0]], channel=k)
        done += n
        k += 1
        el = time.perf_counter() - t0
        if el > budget_s * 0.5 or k >= 4 * iq_base.shape[0]:
            break
    single = done / sps / el
    cores = os.cpu_count() or 1
    reps = max(1, int(budget_s * 0.5 * single * sps / n))  # channels each worker can do in the remaining budget
    jobs = cores * reps
    t1 = time.perf_counter()
    with ThreadPoolExecutor(cores) as ex:
        list(ex.map(lambda j: len(oracle.chain_iq200(iq_base[j % iq_base.shape[0]], channel=j)), range(jobs)))
    el2 = time.perf_counter() - t1
    allc = jobs * n / sps / el2
    # the same chain from the flow graph's 400 ksps capture rate, i.e. including the per-channel 299-tap channel filter
    # (G1) that the wideband workload's channelizer replaces -- the reference's full per-channel cost
    from gr_amps_amd import synth
    n4 = 1 << 19
    iq400, _ = synth.make_channel_block(n4, 1, seed=77, sps=20)
    iq400 = (iq400 * np.exp(2j * np.pi * 0.4 * np.arange(n4))).astype(np.complex64)
    t2 = time.perf_counter()
    oracle.chain_iq400(iq400, 160e3, chunk=4096)
    el3 = time.perf_counter() - t2
    with_g1 = n4 / 20 / el3
    return {
        "with_channel_filter": {"value": round(with_g1 / 1e6, 4), "unit": "Msym/s", "cores": 1,
                                "sample": "1 block of %d samples @400 ksps through G1 (299-tap xlating FIR, decim 2) + the chain above" % n4},
        "value": round(single / 1e6, 4), "unit": "Msym/s", "cores": 1, "kind": "port",
        "sample": "%d channel-blocks of %d samples @200 ksps through the restated reference chain "
                  "(quad demod, M&M, slicer, recc, recc_decode), 1 thread" % (k, n),
        "all_cores_value": round(allc / 1e6, 4), "all_cores": cores,
    }


# what the 4/3 x oversampled bank (D = 768, the library default since round 6) costs in sensitivity against the 2x oversampled one, on the
# same blocks: scripts/decim_sensitivity.py on one MI355X, 1248 bursts per point (profiles/r06/decim768_sensitivity.txt)
DECIM_SENSITIVITY = {"unit": "dB C/N in 30 kHz at 1 % burst loss, wideband seam, slicer spec D, tracked capture",
                     "source": "profiles/r06/decim768_sensitivity.txt (1248 bursts per point, the same blocks through both decimations)",
                     "no_offset": {"D512": 9.07, "D768": 9.23}, "clock_100ppm": {"D512": 9.18, "D768": 9.40},
                     "clock_100ppm_carrier_2kHz": {"D512": 11.57, "D768": 12.29}, "clock_500ppm": {"D512": 9.06, "D768": 9.42},
                     "penalty_of_D768_dB": {"no_offset": 0.16, "clock_100ppm": 0.22, "clock_100ppm_carrier_2kHz": 0.72, "clock_500ppm": 0.36}}


# ----------------------------------------------------------------------------------------------------- flop / byte models
def chz_flops_per_frame(taps, slicer, n_channels):
    """Algorithmic flops of the filter-bank kernel per frame (512 new wideband samples), as the kernel computes them:
    fold 1024 branches x taps x (complex x real = 2 FMA); FFT-1024 = 4 x 16 x 16: 10240 complex adds, 2816 general complex
    multiplies (twiddles between the passes + inside the radix-16 butterflies); slicer per active bin."""
    fold = 1024 * taps * 2 * 2
    fft = 10240 * 2 + 2816 * 6
    # conj-product (+ arctangent) + boxcar adds; spec D: two imaginary parts of conj-products (its sign logic is integer work, not flops)
    per_bin = {"atan": 8 + 27 + 2, "sine": 3 + 2, "product": 3, "exact": 6}[slicer]
    return fold + fft + per_bin * n_channels


def front_flops_per_sample(slicer, sps):
    return {"atan": 8 + 27, "sine": 3, "product": 3, "exact": 6}[slicer] + (0 if slicer in ("product", "exact") else (sps - 1))


def profile_traffic(key):
    """HBM bytes per launch of this workload's dominant kernel from the newest committed PMC profile (profiles/rNN/traffic.json,
    separate rocprofv3 --pmc passes) -- a profile figure, reported beside the in-run numbers, never as one of them."""
    pdir = os.path.join(ROOT, "profiles")
    if not os.path.isdir(pdir):
        return None
    for tag in sorted(os.listdir(pdir), reverse=True):
        tj = os.path.join(pdir, tag, "traffic.json")
        if os.path.exists(tj):
            t = json.load(open(tj))
            for e in (t if isinstance(t, list) else [t]):
                if e.get("key") == key:
                    e = dict(e)
                    e["source"] = "profiles/%s/traffic.json" % tag
                    return e
    return None


# ----------------------------------------------------------------------------------------------------- power / clock sampler
class SmiSampler:
    """Samples package power and shader clock with rocm-smi (a subprocess per sample, on the host only) while the timed region
    runs, so that the bench line says in what state the number was measured (the wideband stream sits on the
    package power limit).  Absent or failing rocm-smi -> no field."""

    def __init__(self, device, period=0.7):
        import shutil
        import threading
        self.exe = shutil.which("rocm-smi")
        self.device, self.period = device, period
        self.samples, self._stop, self.other_clocks = [], threading.Event(), {}
        self._t = threading.Thread(target=self._run, daemon=True) if self.exe else None

    def _one(self):
        import subprocess
        try:
            out = subprocess.run([self.exe, "-d", str(self.device), "--showpower", "--showclocks", "--json"], stdout=subprocess.PIPE,
                                 stderr=subprocess.DEVNULL, timeout=5, text=True).stdout
            card = next(iter(json.loads(out).values()))
            power = next((float(v) for k, v in card.items() if "Power" in k and "(W)" in k), None)

            def clock(name):
                v = next((v for k, v in card.items() if k.startswith(name)), None)
                digits = "".join(ch for ch in str(v) if ch.isdigit() or ch == ".") if v else ""
                return float(digits) if digits else None
            mhz = clock("sclk")
            if power is not None and mhz is not None:
                self.samples.append((power, mhz))
                # memory and fabric clocks beside the shader clock: what an HBM-bound kernel's box-to-box spread has to be read against
                self.other_clocks = {k: clock(k) for k in ("mclk", "fclk", "socclk") if clock(k) is not None}
        except Exception:
            pass

    def _run(self):
        while not self._stop.wait(self.period):
            self._one()

    def one_shot(self):
        """one sample, synchronously (short timed regions: taken immediately before and after, while the GPU still runs the same step)"""
        n = len(self.samples)
        if self.exe:
            self._one()
        return self.samples[-1] if len(self.samples) > n else None

    def start(self):
        if self._t:
            self._t.start()

    def stop(self):
        if not self._t:
            return None
        self._stop.set()
        self._t.join(timeout=6)
        if len(self.samples) < 2:
            return None
        p = [x[0] for x in self.samples]
        f = [x[1] for x in self.samples]
        return {"package_w_mean": round(sum(p) / len(p), 1), "package_w_max": round(max(p), 1), "sclk_mhz_mean": round(sum(f) / len(f), 1),
                "other_clocks_mhz": self.other_clocks, "samples": len(p), "source": "rocm-smi --showpower --showclocks every %.1f s during the timed region" % self.period}


# ----------------------------------------------------------------------------------------------------- one workload
def run_workload(name, a, torch, dev, dist, rank, world, local, slicer, steps, warmup, light=False, dist_mode=None, decim=None):
    """Build the resident batch, warm up, time exactly `steps` steps (barrier + synchronize on both sides,
    max over ranks) and return the result fields for this workload.  light = kernel time only (other slicer specs)."""
    from gr_amps_amd import capi
    wide = name == "wideband832"
    dist_mode = dist_mode or a.dist
    one_band = wide and dist is not None and dist_mode != "bands"
    planted = None
    # test knob (tests/test_gpu_bench_ranks.py): N ranks on ONE device.  Their batch syntheses -- thousands of small torch kernels each --
    # then run one rank after the other: eight processes with deep queues on one GPU are time-sliced per PROCESS by the kernel driver
    # and did not finish in seven minutes (all eight sat in the first synchronising HIP call of amps_recc_create behind their own
    # queues; AMPS_RECC_TRACE_CREATE).  On a node every rank has its own device and nothing is serialised.
    stagger = dist is not None and world > 1 and os.environ.get("AMPS_BENCH_SHARE_GPU") == "1"

    def build_in_turn(fn):
        if not stagger:
            return fn()
        out = None
        for turn in range(world):
            if turn == rank:
                out = fn()
                torch.cuda.synchronize()
            dist.barrier()
        return out
    if wide:
        # config 3: the whole 832-channel band from one 30.72 Msps stream through the polyphase channelizer
        decim = int(decim or a.decim)
        sps, C, first_bin = 1536 // decim, 832, 96
        # wideband samples per step: ~1 GiB = 4.4 s of signal, and a whole number of 64-frame groups per CU either way (the filter bank's
        # workgroups take whole groups of 64 frames: 2^27 samples are 16 groups per CU at D = 512 but 10.67 at D = 768, where eleven
        # groups per CU are 138 412 032 samples = 1.03 GiB -- a caller who cares picks its push size like that, and so does this step)
        NW = a.samples or ((1 << 27) if decim == 512 else 11 * 256 * 64 * 768)
        N = NW // decim                                   # samples per channel after the channelizer
        wb = {"channels": 1024, "decim": decim, "taps_per_branch": a.taps, "first_channel": first_bin}
        n_band = C
        groups, group = (world, rank) if one_band else ((a.groups, a.groups - 1) if (a.groups and dist is None) else (0, 0))
        if groups in (2, 4, 8):
            # one band, interleaved channel groups (cfg.wideband_groups): rank r decodes the channels whose FFT bin k has (k mod 64)
            # in its window, and its filter-bank kernel skips pass 3 and the slicer for everybody else's bins
            mine = [c for c in range(832) if (((96 + c) % 1024) % 64) // (64 // groups) == group]
            wb.update(groups=groups, group=group)
            batch, planted = build_in_turn(lambda: make_wideband_batch(torch, dev, NW, 96, 832, 2, seed=1, build=(rank == 0)))   # (only rank 0's copy is ever read)
            planted = {c: m for c, m in planted.items() if c in set(mine)}
            C = len(mine)
        elif one_band:                                    # world sizes without a group split: contiguous channel ranges, whole filter bank per rank
            C = 832 // world
            first_bin = 96 + rank * C
            wb["first_channel"] = first_bin
            n_band = C
            batch, planted = build_in_turn(lambda: make_wideband_batch(torch, dev, NW, 96, 832, 2, seed=1, build=(rank == 0)))
            planted = {c - rank * C: m for c, m in planted.items() if rank * C <= c < (rank + 1) * C}
        else:
            batch, planted = build_in_turn(lambda: make_wideband_batch(torch, dev, NW, first_bin, C, 2, seed=rank + 1))
        abi_mode = {"broadcast_abi": "broadcast", "scatter_allgather_abi": "scatter_allgather"}.get(dist_mode) if one_band else None
        if one_band and not abi_mode:
            recv = [torch.empty_like(batch), torch.empty_like(batch)]
        coll_ev = []                                      # torch.distributed modes: (start, end) events around the last steps' collectives
        expected = len(planted)
        iq_base = None
        r = capi.Recc(n_channels=n_band, sps=sps, max_samples=N + 72, max_bursts=max(4096, 2 * expected), device=local, time_kernels=True,
                      slicer=slicer, sync_torch=False, wideband=wb)                # (+ 72: at D = 768 a 2^27-sample block is no whole number of 64-frame groups, the rest waits in the carry)
        if abi_mode:                                      # the communicator lives in the handle; the id travels over the control plane
            ids = [capi.Recc.rccl_unique_id() if rank == 0 else None]
            dist.broadcast_object_list(ids, src=0)
            r.rccl_init(ids[0], world, rank)
        step_no = [0]
        busy = [None, None]                               # per receive buffer: event behind the kernels that last read it

        def push():
            if abi_mode:
                r.push_wideband_dist(batch if rank == 0 else None, NW if rank == 0 else None, 0, abi_mode)
            elif one_band:
                # the step's block travels rank 0 -> everybody over xGMI inside the timed region; two receive buffers, so the
                # collective of step i overlaps the kernels of step i - 1 and only waits for those of step i - 2
                slot = step_no[0] & 1
                buf = recv[slot]
                step_no[0] += 1
                if busy[slot] is not None:
                    torch.cuda.current_stream().wait_event(busy[slot])
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
                if dist_mode == "broadcast":
                    if rank == 0:
                        buf.copy_(batch, non_blocking=True)
                    dist.broadcast(torch.view_as_real(buf), src=0)
                else:
                    flat = torch.view_as_real(buf).view(-1)
                    chunk = flat.numel() // world
                    mine = flat[rank * chunk:(rank + 1) * chunk]
                    src = list(torch.view_as_real(batch).view(-1).split(chunk)) if rank == 0 else None
                    dist.scatter(mine, scatter_list=src, src=0)
                    dist.all_gather_into_tensor(flat, mine)
                ev[1].record()
                coll_ev.append(ev)
                del coll_ev[:-8]
                r.wait_torch()                            # the handle's stream waits for the collective (no host sync)
                r.push_wideband(buf)
                busy[slot] = r.record_torch_event()
            else:
                r.push_wideband(batch)
    else:
        sps = 10
        C, N = (1, a.samples or (1 << 26)) if name == "direct1" else (832, a.samples or (1 << 18))
        NW = 0
        batch, iq_base, expected = make_batch(torch, dev, C, N, sps, seed=rank + 1)
        r = capi.Recc(n_channels=C, sps=sps, max_samples=N, max_bursts=max(4096, 2 * expected), device=local, time_kernels=True,
                      slicer=slicer, sync_torch=False)

        def push():
            r.push_iq(batch)
    torch.cuda.synchronize()                               # the batch is complete before the library's stream reads it

    def step():
        push()
        return r.drain(copy=False)

    # the metric is SUSTAINED throughput: the GPU's clocks take a few hundred ms of load to settle (kernel time falls
    # ~7 % over the first dozen launches), so the same step runs untimed for --prewarm-ms before the W warmup steps
    short_poll = a.full and not light and steps < 4000 and not a.no_power_sample and not one_band
    short_smi = SmiSampler(local, period=0.02) if (short_poll and rank == 0) else None
    if short_smi:
        short_smi.start()
    tp = time.perf_counter()
    lockstep = dist is not None and one_band                # a step holds a collective: every rank must run the SAME number of them
    go = torch.ones(1, device=dev, dtype=torch.int32) if lockstep else None
    n_prewarm = 0
    while True:
        more = (time.perf_counter() - tp) * 1e3 < (100.0 if light else a.prewarm_ms)
        if lockstep:
            # rank 0's clock decides for everybody (round 5: the loop used to end on every rank's own clock -- ranks that fit one step
            # more into the window than their peers left an unmatched collective behind them and the run hung; found by the 4-rank
            # rehearsal on one GPU, tests/test_gpu_bench_ranks.py)
            go.fill_(1 if more else 0)
            dist.broadcast(go, src=0)
            more = bool(int(go.item()))
        if not more:
            break
        step()
        n_prewarm += 1
    recs = None
    r.timing(reset=True)
    for _ in range(warmup):             # the per-kernel breakdown comes from these (all launches bracketed by HIP events)
        recs = step()
    tm_all = r.timing()
    n_all = max(warmup, 1)
    # in the timed region only the dominant kernel is bracketed: ten event records per step cost ~3 % of the step
    # ... and two event records per step still cost a wideband step 6.5 us = 1.9 % (profiles/r06/event_cost.txt): a long region brackets
    # the dominant kernel of every eighth push (>= 100 launches timed), a short one (the driver's --steps 20) every push
    r.set_timing(os.environ.get("AMPS_BENCH_TIMING", "sampled" if steps >= 800 else "dominant"))
    checked = None
    if recs is not None:   # sanity: the decode path really ran -- the planted bursts came back with the transmitted MIN
        if wide:           # a burst cut by the edge of the repeated block may be lost; nearly all must decode
            ok = sum(1 for g in recs if planted.get(int(g["channel"]), (None,))[0] == g["min"].decode() and g["valid"][0])
            assert ok >= 0.97 * expected, (ok, len(recs), expected)
            checked = {"planted": expected, "decoded_with_transmitted_MIN": ok}
        else:
            assert len(recs) == expected and recs["valid"].all(), (len(recs), expected)
            checked = {"planted": expected, "decoded_valid": int(len(recs))}
    r.timing(reset=True)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    barrier()
    sustained = steps >= 4000                             # a region of a couple of seconds: sampled while it runs
    smi = SmiSampler(local) if (a.full and rank == 0 and not light and sustained and not a.no_power_sample) else None
    if smi:
        smi.start()
    # A short region (the driver's --steps 20 is 9 ms) ends before one rocm-smi call returns.  The poller (`short_smi`, started in front
    # of the prewarm) then runs back to back THROUGH prewarm, warmup, the timed region and a burst of untimed steps of the same workload
    # behind it, so the clock and the power this very process ran at are on the record ("power: null in the run the judge
    # sees"); `sustained: false` says these are samples around a region too short to hold one.  (Measured, profiles/r05/power_modes.txt:
    # an extra second of load + polling in FRONT of the region slowed its kernels by 8-17 %; polling through it costs <= 2 %.)  Every rank
    # runs the same number of untimed steps (whole-band modes only: no collective in them); rank 0 samples.
    t0 = time.perf_counter()
    nrec = 0
    last = None
    if a.no_pipeline:
        for _ in range(steps):
            last = step()
            nrec += len(last)
    else:
        # streaming form of the same K steps: the records of step i are collected (split drain) while step i+1 runs, so the
        # GPU does not idle for the ~60 us of host work between steps; every step's records are still drained inside the
        # timed region
        for i in range(steps):
            push()
            if i:
                nrec += len(r.drain_end(copy=False))
            r.drain_begin()
        last = r.drain_end(copy=False)
        nrec += len(last)
    torch.cuda.synchronize()
    barrier()
    el = time.perf_counter() - t0
    el_own = el
    # the last timed step's records, copied before any later drain reuses the handle's buffer; position made relative to the first
    # sample (channel rate) of that step's push, which a clock-bounded prewarm would otherwise move from run to run
    last_records = None
    if a.dump_outputs and not light and last is not None:
        pushes_before = n_prewarm + warmup + steps - 1
        last_records = (np.array(last), pushes_before * NW // decim if wide else pushes_before * N)
    power = None
    tm_keep = None
    if smi:
        power = smi.stop()
        if power:
            power["sustained"] = True
    elif short_poll:
        tm_keep = r.timing()                              # the timed region's events, before the burst behind it adds to them
        for i in range(1100):                             # ~0.5 s more of the same step for the poller to catch
            push()
            if i:
                r.drain_end(copy=False)
            r.drain_begin()
        r.drain_end(copy=False)
        torch.cuda.synchronize()
        if short_smi and short_smi._t:                    # (no rocm-smi on the box: no poller thread, no `power`)
            short_smi._stop.set()
            short_smi._t.join(timeout=6)
            sm = short_smi.samples
            if sm:
                def mean(k):
                    return round(sum(x[k] for x in sm) / len(sm), 1)
                power = {"sustained": False, "package_w_mean": mean(0), "package_w_max": round(max(x[0] for x in sm), 1), "sclk_mhz_mean": mean(1),
                         "sclk_mhz_min": round(min(x[1] for x in sm), 1), "other_clocks_mhz": short_smi.other_clocks, "samples": len(sm),
                         "source": "rocm-smi --showpower --showclocks polled back to back from the prewarm, through the warmup and the timed region (shorter "
                                   "than one rocm-smi call), to the end of ~0.5 s of untimed steps of the same workload behind it"}
    if dist is not None:
        t = torch.tensor([el], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
    tm = tm_keep if tm_keep is not None else r.timing()
    gathered = None
    coll = None
    if wide and one_band:
        # the collective itself, by events on the stream it ran on: the library's (ABI modes, amps_recc_rccl_info) or torch's
        if abi_mode:
            i = r.rccl_info()
            coll = {"op": abi_mode, "issued_by": "libamps_recc.so (amps_recc_push_wideband_dist)", "timed": int(i["collectives_timed"]),
                    "ms": round(i["collective_ms"] / max(1, i["collectives_timed"]), 4), "gbps": None if i["collective_gbps"] is None else round(i["collective_gbps"], 2)}
        elif coll_ev:
            ms = [e[0].elapsed_time(e[1]) for e in coll_ev]
            coll = {"op": dist_mode, "issued_by": "torch.distributed (%s)" % dist.get_backend(), "timed": len(ms), "ms": round(sum(ms) / len(ms), 4),
                    "gbps": round(8.0 * NW / (sum(ms) / len(ms) * 1e-3) / 1e9, 2) if sum(ms) > 0 else None}
        if coll:
            coll["bytes_per_step"] = 8 * NW
            coll["note"] = "block bytes / duration of the collective on this rank's stream (root -> all); overlaps the kernels of the previous step"
    identity = None
    if dist is not None:
        # who this rank is, as the library's own view of the device (and of the communicator, where it owns one) reports it
        try:
            i = r.rccl_info()
            identity = {"rank": rank, "device": i["device"], "device_uuid": i["device_uuid"], "pci": "%04x:%02x:%02x" % (i["pci_domain"], i["pci_bus"], i["pci_device"]),
                        "rccl_nranks": i["comm_nranks"] if i["nranks"] else None, "rccl_rank": i["comm_rank"] if i["nranks"] else None,
                        "rccl_library": i["library"] if i["nranks"] else None, "ms_per_step": round(el_own / steps * 1e3, 4), "kernel_ms": None}
        except capi.AmpsError:
            identity = {"rank": rank, "error": "amps_recc_rccl_info"}
    if wide and abi_mode and a.full:
        # outside the timed region: one more step whose records come back through the ABI's collective drain (amps_recc_drain_gather:
        # every rank's list merged at rank 0) -- the whole band's bursts in one place, counted on the record
        push()
        gathered = int(len(r.drain_gather(root=0)))
    r.close()
    del batch
    torch.cuda.empty_cache()
    syms_per_step_rank = C * (NW / 1536.0) if wide else C * N / sps
    # whole-job symbols: every rank its own band (bands), or the ONE band the ranks split between them (one-band modes)
    if one_band:           # the ONE band the ranks split between them: count the channels the ranks really decode (832 // world * world
        tc = torch.tensor([float(C)], device=dev, dtype=torch.float64)      # for a world size without a group split)
        dist.all_reduce(tc, op=dist.ReduceOp.SUM)
        value = float(tc.item()) * (NW / 1536.0) * steps / el
    else:                  # every rank its own band
        value = syms_per_step_rank * world * steps / el
    if wide:   # dominant kernel = the channelizer; algorithmic bytes = the wideband block read once (14.77 B/symbol at 832 channels)
        kms = tm["ms_channelizer"] / max(1, tm["launches_channelizer"])
        alg_bytes = 8.0 * NW
        kname = "chz12_kernel<%d, slicer %s, D = %d>" % (a.taps, SLICERS[slicer], decim)
        flops = chz_flops_per_frame(a.taps, slicer, C) * (NW / float(decim))
        note = ("filter bank (fold + FFT-1024 = 4 x 16 x 16) + slicer spec %s in one kernel, %.1f flop per input byte: bound by VALU issue "
                "and LDS exchange, not by HBM bandwidth (both rooflines are reported; the HBM fraction is what the metric asks for); in the sustained "
                "stream the package sits on its 1.4 kW limit, and the ~180 W of reading the input from HBM cost the kernel 10 %% of its time in shader "
                "clock, late loads another 5 %% (profiles/r06/chz_l2_touch.txt).  Only slicer bits (1/64 of the input) reach HBM; the trigger search "
                "and the decode kernel follow" % (SLICERS[slicer], flops / alg_bytes))
    else:
        kms = tm["ms_front"] / max(1, tm["launches_front"])
        alg_bytes = ALG_BYTES_PER_SYMBOL_DIRECT * syms_per_step_rank
        kname = "recc_front_kernel<10,1, slicer %s>" % SLICERS[slicer]
        flops = front_flops_per_sample(slicer, sps) * float(C) * N
        note = ("streaming kernel: one pass over the IQ block, %.1f flop per input byte; bound by HBM latency / bandwidth together with VALU issue "
                "(profiles/r04/pmc_kernels.txt)" % (flops / alg_bytes))
    if identity is not None and "error" not in identity:
        identity["kernel_ms"] = round(kms, 4)
    if light:
        return {"kernel": kname, "kernel_ms": round(kms, 4), "value": round(value / 1e6, 3), "checked": checked}, iq_base
    ach = alg_bytes / (kms * 1e-3) / 1e9 if kms > 0 else 0.0
    tfl = flops / (kms * 1e-3) / 1e12 if kms > 0 else 0.0
    drain_note = "" if a.no_pipeline else " (split drain: collected while the next step runs)"
    prof = profile_traffic(name + ":" + slicer + (":768" if wide and decim == 768 else ""))
    if wide and groups in (2, 4, 8):
        par = ("one band, %d interleaved channel groups (cfg.wideband_groups), this line = group %d: %d channels; every rank folds the whole stream, "
               "pass 3 of the FFT and the slicer run for the rank's own bins only%s"
               % (groups, group, C, ("; rank 0's block by RCCL %s every step" % ({"broadcast": "broadcast", "broadcast_abi": "broadcast issued inside the C ABI", "scatter_allgather_abi": "scatter + all-gather issued inside the C ABI"}.get(dist_mode, "scatter + all-gather"))) if one_band else
                  " (single-GPU measurement of one rank's share, --groups)"))
    elif one_band:
        par = ("%s: rank 0's block by RCCL %s every step, rank r decodes channels [%d r, %d (r+1)); the whole filter bank runs on every rank"
               % (dist_mode, "broadcast" if dist_mode == "broadcast" else "scatter + all-gather", C, C))
    else:
        par = "bands sharded x%d (one 832-channel band per GPU), no data-path collective" % world
    res = {
        "value": round(value / 1e6, 3), "ms_per_step": round(el / steps * 1e3, 4),
        "config": {"workload": ("wideband832 (BASELINE configs[3]): one fc32 stream @30.72 Msps, %d samples per step per GPU -> 1024-branch "
                                "polyphase channelizer (D = %d) -> 832 RECC channels @%d ksps -> fused slicer (numeric spec %s) + sync + BCH(63,51) decode, "
                                "records drained every step%s" % (NW, decim, 30720 // decim, SLICERS[slicer], drain_note)) if wide else
                               ("%s (BASELINE configs[1] batched): %d RECC channels x %d fc32 IQ samples @200 ksps per step per GPU, channel-major, "
                                "fused slicer (numeric spec %s) + sync + BCH(63,51) decode, records drained every step%s"
                                % (name, C, N, SLICERS[slicer], drain_note)),
                   "channels_per_gpu": C, "samples_per_channel": N, "samples_per_symbol": sps, "slicer_spec": SLICERS[slicer],
                   **({"wideband_decim": decim, "wideband_samples_per_step": NW} if wide else {}),
                   "algorithmic_bytes_per_symbol": round(alg_bytes / syms_per_step_rank, 2),
                   "realtime_channels_per_gpu": round(value / world / 20e3, 1),
                   **({"records_gathered_at_rank0_in_one_step": gathered} if gathered is not None else {}),
                   "bursts_decoded_per_step_per_gpu": nrec // max(1, steps), "checked": checked, "parallelism": par},
        "roofline": {"bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                     "frac": round(ach / HBM_PEAK_GBPS, 4),
                     # what actually limits the kernel (PMC, profiles/): the filter bank issues VALU instructions 0.6 of the time at 18 flop/B and
                     # moves 1.08x its algorithmic bytes -- it is NOT held back by HBM; the HBM fraction above stays the headline figure because
                     # that is what the metric asks for.  The streaming kernel of the IQ seam is the HBM-side one (latency / bandwidth + issue).
                     "binding_resource": "valu_issue" if wide else "hbm_latency_and_valu_issue",
                     # the same algorithmic bytes over the whole step (all kernels + launch gaps), per rank
                     "frac_end_to_end": round(alg_bytes / (el_own / steps) / 1e9 / HBM_PEAK_GBPS, 4),
                     "traffic": None,
                     "traffic_note": "HBM counters need separate rocprofv3 --pmc passes; the committed profile of this command is under 'traffic_profile'",
                     "traffic_profile": prof,
                     "kernel": kname, "kernel_ms": round(kms, 4), "launches_timed": int(tm["launches_channelizer"] if wide else tm["launches_front"]),
                     "algorithmic_bytes_per_launch": alg_bytes, "note": note,
                     "frac_of_measured_copy_ceiling_6290": round(ach / 6290.0, 4),
                     "other_kernels_ms_per_step": {k: round(tm_all[k] / n_all, 4) for k in ("ms_front", "ms_resolve", "ms_decode", "ms_carry", "ms_channelizer")},
                     "other_kernels_from": "the %d warmup steps (all kernels bracketed); kernel_ms is from the timed steps" % n_all},
        "roofline_compute": {"bound": "valu_fp32", "flop_per_launch": flops, "achieved": round(tfl, 2), "peak": FP32_PEAK_TFLOPS, "unit": "TFLOP/s",
                             "frac": round(tfl / FP32_PEAK_TFLOPS, 4), "flop_per_byte": round(flops / alg_bytes, 2),
                             "kernel": kname, "kernel_ms": round(kms, 4),
                             "note": "algorithmic flops of the same kernel (model in bench.py: chz_flops_per_frame / front_flops_per_sample) over the same in-run HIP-event duration"},
    }
    # self-check of the in-run event timing against the host clock: the dominant kernel's events + the other kernels of a step (from the
    # warmup steps) cannot exceed the step.  (Seen once in round 6: a sustained run right behind five rocprofv3 passes on the same box
    # whose sampled events read 0.3185 ms inside a 0.3360 ms step with a 0.035 ms tail -- the step is the host clock's and stands.)
    dom = "ms_channelizer" if wide else "ms_front"
    tail_ms = sum(tm_all[k] / n_all for k in ("ms_front", "ms_resolve", "ms_decode", "ms_carry", "ms_channelizer") if k != dom)
    step_ms = el_own / steps * 1e3
    res["roofline"]["events_vs_step"] = {"kernel_ms_plus_other_kernels": round(kms + tail_ms, 4), "ms_per_step": round(step_ms, 4),
                                         "consistent": bool(kms + tail_ms <= 1.02 * step_ms),
                                         "kernel_ms_bound_from_step": round(step_ms - tail_ms, 4)}
    if power:
        res["power"] = power
    if identity is not None:
        res["identity"] = identity
    if coll is not None:
        res["collective"] = coll
    if last_records is not None:
        res["last_records"] = last_records
    return res, iq_base


def realtime_latency(torch, slicer, local, blocks=60):
    """'also report a real-time-latency run'.  HOST-resident IQ arrives in 20 ms blocks, as a receiver delivers it;
    latency = amps_recc_push_* (H2D staging + kernels) + amps_recc_drain, per block, host clock.  Three cases: one channel and 832
    channels at 200 ksps on the IQ seam (4000 samples per channel and block), and the full band on the wideband seam (614 400 samples
    at 30.72 Msps per block)."""
    from gr_amps_amd import capi, synth
    out = {"block_ms": 20.0, "blocks_timed": blocks, "input": "host memory (pageable numpy), staged by the library inside the push",
           "unit": "us per block: push + drain"}

    def stats(lat):
        lat = np.array(lat) * 1e6
        return {"median_us": round(float(np.median(lat)), 1), "p99_us": round(float(np.percentile(lat, 99)), 1),
                "fraction_of_real_time": round(float(np.median(lat)) / 20000.0, 5)}
    n = 4000
    for C in (1, 832):
        base = np.stack([synth.make_channel_block(25 * n, 2, seed=c)[0] for c in range(min(C, 8))])
        iq = np.tile(base, ((C + 7) // 8, 1))[:C]
        with capi.Recc(n_channels=C, sps=10, max_samples=n, max_bursts=max(64, 4 * C), device=local, slicer=slicer) as r:
            lat = []
            for k in range(blocks + 10):
                blk = np.ascontiguousarray(iq[:, (k % 25) * n:(k % 25 + 1) * n])
                t0 = time.perf_counter()
                r.push_iq(blk)
                r.drain(copy=False)
                lat.append(time.perf_counter() - t0)
        out["iq_seam_%d_channels" % C] = stats(lat[10:])
    nw = 614400
    rng = np.random.default_rng(3)
    wbase = (rng.standard_normal((8, nw, 2)).astype(np.float32) * 0.05).view(np.complex64)[..., 0]
    wb = {"channels": 1024, "decim": 512, "taps_per_branch": 8, "first_channel": 96}
    with capi.Recc(n_channels=832, sps=3, max_samples=nw // 512 + 72, max_bursts=4096, device=local, slicer=slicer, wideband=wb) as r:
        lat = []
        for k in range(blocks + 10):
            t0 = time.perf_counter()
            r.push_wideband(wbase[k % 8])
            r.drain(copy=False)
            lat.append(time.perf_counter() - t0)
    out["wideband_seam_832_channels"] = stats(lat[10:])
    return out


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    a = parse(argv)
    ensure_world(a, argv)
    if os.environ.get("AMPS_BENCH_CPU_PLUMBING") == "1":
        return plumbing_only(a)
    import torch

    if os.environ.get("AMPS_BENCH_FAULTHANDLER"):            # debugging aid: every thread's Python stack to stderr if the run is still going after that many seconds
        import faulthandler
        faulthandler.dump_traceback_later(float(os.environ["AMPS_BENCH_FAULTHANDLER"]), repeat=False, file=sys.stderr, exit=False)
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != a.gpus and world > 1:
        raise SystemExit("--gpus must equal WORLD_SIZE")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the RECC path has no CPU fallback")
    share = os.environ.get("AMPS_BENCH_SHARE_GPU") == "1"    # test knob: every rank on device 0, collectives over gloo (RCCL refuses two ranks on one
    if share:                                                # device) -- tests/test_gpu_bench_ranks.py runs the N > 1 code on the one GPU a box has
        local = 0
    if local >= torch.cuda.device_count():
        raise SystemExit("rank %d: only %d GPU(s) visible on this node" % (rank, torch.cuda.device_count()))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    if world > 1 or os.environ.get("AMPS_BENCH_FORCE_DIST") == "1":   # the env knob exercises the RCCL path on a 1-GPU box
        import torch.distributed as dist
        os.environ.setdefault("MASTER_PORT", "29511")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if share:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    if a.dist != "bands" and a.workload != "wideband832":
        raise SystemExit("--dist %s distributes a wideband block: use --workload wideband832" % a.dist)

    from gr_amps_amd import capi
    lib_default = capi.SLICER_NAMES[capi.load().amps_recc_default_slicer()]
    is_default = a.slicer in ("default", lib_default)
    if a.slicer == "default":
        a.slicer = lib_default
    lib_decim = int(capi.load().amps_recc_default_wideband_decim())
    decim_is_default = a.decim in ("default", str(lib_decim))
    a.decim = lib_decim if a.decim == "default" else int(a.decim)
    broken_group = False
    res, iq_base = run_workload(a.workload, a, torch, dev, dist, rank, world, local, a.slicer, a.steps, a.warmup)
    last_records = res.pop("last_records", None)
    if rank == 0 and last_records is not None:
        dump_records(a.dump_outputs, *last_records)
    res["config"]["slicer_is_library_default"] = is_default
    if a.workload == "wideband832":
        res["config"]["decim_is_library_default"] = decim_is_default
    res["config"]["slicer_sensitivity"] = SLICER_SENSITIVITY
    out = {
        "metric": "AMPS RECC Manchester symbols demodulated+decoded per second (real-time channels = value/0.02); achieved HBM GB/s vs peak",
        "value": res["value"], "unit": "Msym/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": res["ms_per_step"], "higher_is_better": True,
        "scaling": "weak" if (a.dist == "bands" or world == 1) else "strong",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": res["config"], "roofline": res["roofline"], "roofline_compute": res["roofline_compute"], "prewarm_ms": a.prewarm_ms,
        "power": res.get("power"),
        "dist": a.dist,
    }
    if a.full and world == 1 and not a.no_other_specs:
        # the same workload under the other slicer specs (short runs: kernel time + the decode check), so that what the default
        # (spec D) saves against the arctangent of spec A -- and what the cheaper specs B / C would save on top -- is on the record
        other = {}
        for sp in SLICERS:
            if sp != a.slicer:
                o, _ = run_workload(a.workload, a, torch, dev, None, 0, 1, local, sp, 20, 3, light=True)
                other[SLICERS[sp]] = o
        out["other_slicer_specs"] = other
    if a.full and world == 1 and a.workload == "wideband832" and not a.no_other_decim:
        # the same workload at the other decimation of the filter bank: the library default (D = 512, three samples per symbol: the most
        # sensitive form) and the 4/3 x oversampled bank (D = 768, two samples per symbol: 1.5 x fewer frames per input byte) side by side
        od = 768 if a.decim == 512 else 512
        o_steps = min(a.steps, 2000)
        o, _ = run_workload("wideband832", a, torch, dev, None, 0, 1, local, a.slicer, o_steps, a.warmup, decim=od)
        out["other_decim"] = {"wideband_decim": od, "value": o["value"], "unit": "Msym/s", "steps": o_steps, "ms_per_step": o["ms_per_step"], "config": o["config"],
                              "roofline": o["roofline"], "roofline_compute": o["roofline_compute"], "power": o.get("power"),
                              "sensitivity": DECIM_SENSITIVITY}
    if a.full and world == 1 and a.secondary != "none" and a.secondary != a.workload:
        sec_steps = min(a.steps, 2000)
        sec, sec_base = run_workload(a.secondary, a, torch, dev, None, 0, 1, local, a.slicer, sec_steps, a.warmup)
        out["secondary"] = {"value": sec["value"], "unit": "Msym/s", "steps": sec_steps, "ms_per_step": sec["ms_per_step"], "config": sec["config"],
                            "roofline": sec["roofline"], "roofline_compute": sec["roofline_compute"], "power": sec.get("power")}
        if iq_base is None:
            iq_base = sec_base
    if world == 1 and a.secondary != "none" and "secondary" in out and not a.no_latency:
        out["secondary"]["latency"] = realtime_latency(torch, a.slicer, local)
    if dist is not None:
        # The N > 1 record describes its own ranks: per rank the device the library ran on (UUID + PCI address from the HIP
        # runtime), the rank's own ms_per_step and kernel time, and -- where the library owns a communicator -- RCCL's own rank count.  A
        # record with N distinct UUIDs proves N GPUs by itself.
        def gather_identities(mine):
            ids = [None] * world
            dist.all_gather_object(ids, mine)
            return ids
        ids = gather_identities(res.get("identity"))
        uu = [i.get("device_uuid") for i in ids if i]
        out["ranks"] = ids
        out["distinct_devices"] = len(set(uu))
        out["process_group"] = {"backend": dist.get_backend(), "world_size": dist.get_world_size()}
        if res.get("collective"):
            out["collective"] = res["collective"]
    if a.full and world > 1 and a.dist == "bands" and a.workload == "wideband832" and a.secondary != "none":
        # What BASELINE configs[4] names beside the band-per-GPU headline: ONE band, its block distributed from rank 0 over xGMI inside
        # the timed region, every rank decoding its interleaved channel group.  Two short passes, so that one driver invocation per N
        # yields all curves: `secondary` = RCCL ncclBroadcast through torch.distributed; `secondary_abi` = scatter + all-gather issued by
        # the library itself (amps_recc_push_wideband_dist).  `scaling` of these entries is "strong" (one band whatever N).
        # The headline above is already measured: whatever goes wrong in these passes is recorded in their place, not raised (a rank that
        # raised has left the collectives, so the process group is then not torn down either -- see the end of main), and a pass that
        # does not come back within --optional-pass-timeout is abandoned by a watchdog that prints the line as it stands.
        import threading
        bsteps = max(4, min(a.steps, 40))
        done = threading.Event()

        def emit_and_leave():
            if done.is_set():
                return
            for k in ("secondary", "secondary_abi"):
                out.setdefault(k, {"error": "not finished within %.0f s: abandoned by the watchdog" % a.optional_pass_timeout})
            if rank == 0:
                sys.stderr.flush()
                print(json.dumps(out), flush=True)
            os._exit(0)
        dog = threading.Timer(a.optional_pass_timeout, emit_and_leave)
        dog.daemon = True
        dog.start()
        for key, mode, label in (("secondary", "broadcast", "--dist broadcast"), ("secondary_abi", "scatter_allgather_abi", "--dist scatter_allgather_abi")):
            if broken_group:
                out[key] = {"workload": "wideband832, one band over all ranks (%s)" % label, "error": "skipped: the ranks left step in the pass before"}
                continue
            try:
                b, _ = run_workload("wideband832", a, torch, dev, dist, rank, world, local, a.slicer, bsteps, min(a.warmup, 3), dist_mode=mode)
                allk = torch.zeros(world, device=dev, dtype=torch.float64)     # per-rank kernel time, gathered with an all-reduce (gloo, the
                allk[rank] = b["roofline"]["kernel_ms"]                        # test backend, has no all-gather for device tensors)
                dist.all_reduce(allk, op=dist.ReduceOp.SUM)
                out[key] = {"workload": "wideband832, one band over all ranks (%s)" % label, "value": b["value"], "unit": "Msym/s", "steps": bsteps,
                            "ms_per_step": b["ms_per_step"], "scaling": "strong", "config": b["config"],
                            "collective": dict(b.get("collective") or {}, backend=dist.get_backend(), nranks=dist.get_world_size(),
                                               bytes_per_step=8 * b["config"]["wideband_samples_per_step"]),
                            "kernel_ms_per_rank": [round(float(k), 4) for k in allk.tolist()], "ranks": gather_identities(b.get("identity")),
                            "roofline_rank0": b["roofline"]}
            except Exception as e:                                             # noqa: BLE001 -- recorded, see above
                out[key] = {"workload": "wideband832, one band over all ranks (%s)" % label, "error": "%s: %s" % (type(e).__name__, e)}
                broken_group = True
        done.set()
        dog.cancel()
    if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline:
        if iq_base is None:
            iq_base = make_batch(torch, torch.device("cpu"), 16, 1 << 18, 10, seed=1)[1]
        out["cpu_baseline"] = cpu_baseline(iq_base[:, :1 << 18], 10, a.cpu_seconds)
        if a.workload == "wideband832":
            out["cpu_baseline"]["sample"] += ("; per channel at 200 ksps, i.e. downstream of the per-channel 299-tap channel filter the reference "
                                               "would also run -- 'with_channel_filter' times the chain including it")
    if dist is not None and not broken_group:
        dist.destroy_process_group()
    if rank == 0:          # the JSON line is the last thing written: RCCL's banner sits in the C library's stdout buffer until
        import ctypes      # exit when stdout is a pipe, so that buffer is flushed first
        try:
            ctypes.CDLL(None).fflush(None)
        except OSError:
            pass
        sys.stderr.flush()
        print(json.dumps(out), flush=True)
    if broken_group:       # the ranks are no longer in step: leave without the collective teardown (the line above is out)
        sys.stdout.flush()
        os._exit(0 if rank == 0 else 1)


if __name__ == "__main__":
    main()
