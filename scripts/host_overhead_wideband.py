"""host time of one wideband push (the call returns after queueing its launches): the path through channelizer_run.  AMPS_RECC_LIB selects the library."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gr_amps_amd import capi
dev = torch.device("cuda", 0)
out = []
for name, wb, fmt in (("M128/D96 fc32", dict(channels=128, decim=96), None), ("M500/D125 sc8", dict(channels=500, decim=125, taps_per_branch=3), capi.SAMPLES_SC8),
                      ("M1024/D768 fc32 fused", dict(channels=1024, decim=768), None)):
    M, D = wb["channels"], wb["decim"]
    n = D * 256
    r = capi.Recc(n_channels=min(64, M // 3), sps=2, max_samples=1024, max_bursts=1024, wideband=wb)
    if fmt is None:
        x = torch.zeros(n, 2, dtype=torch.float32, device=dev)
        push = lambda: r.push_wideband(torch.view_as_complex(x))
    else:
        x = torch.zeros(n, 2, dtype=torch.int8, device=dev)
        push = lambda: r.push_wideband_as(x, fmt)
    for _ in range(20):
        push()
    r.drain()
    best = []
    for rep in range(5):
        t0 = time.perf_counter()
        for _ in range(200):
            push()
        t1 = time.perf_counter()
        r.drain()
        best.append((t1 - t0) / 200 * 1e6)
    out.append("%s %.2f us (median of 5 x 200; min %.2f max %.2f)" % (name, sorted(best)[2], min(best), max(best)))
    r.close()
print("wideband push, host time per call: " + " | ".join(out))
