#!/usr/bin/env python3
"""Does amps_recc_create answer a sweep of cfgs as another build of the library does?  No GPU needed, and none wanted: without a
device a create answers -EINVAL (-22) for what its checks in front of the device refuse and -ENODEV (-19) for everything else, so
the codes say where the argument checks of two builds differ.  The sweep is that of tests/chz_banks_host.cc.

  python scripts/chz_cfg_identity.py OLD.so NEW.so > profiles/chz_banks/cfg_identity.txt

Each library is driven in a fresh process of its own (AMPS_RECC_LIB selects it).  A difference is expected only from -19 to -22, for a
cfg that OLD refused with -EINVAL behind the device -- the cases named below; anything else is printed as UNEXPLAINED and the exit
status is 1.  Printed: the counts, then per case its first cfg in full and every cfg of the case as its index in the sweep (sweep()
below, counted from 0; runs as first-last).  An unexplained difference is always printed in full."""
import itertools
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNELS = (0, 64, 127, 128, 129, 256, 300, 500, 512, 1000, 1024, 2000, 2048, 2500, 3000)
FLAG_NAMES = ("UNFUSED_WIDEBAND", "CHANNEL_POWER", "STREAM_POWER")
U32 = 0xffffffff


def sweep():
    """(channels, decim, sps, taps, n_channels, first, groups, group, max_samples, flag index) in the program's order"""
    for M in CHANNELS:
        for D, sps, taps, n, first, groups in itertools.product((0, M // 4, M // 4 + 1, M // 2, 3 * M // 4, M, 768), (0, 2, 3, 10), (0, 3, 5, 8),
                                                                (1, M // 3, M // 3 + 1, M, M + 1), (0, (M - 1) & U32, M), (0, 1, 2, 3, 8, 16)):
            for group, max_samples, f in itertools.product((0, 1, groups), (0, 1024), range(8)):
                yield M, D, sps, taps, n, first, groups, group, max_samples, f


def child(out_path):
    sys.path.insert(0, ROOT)
    import ctypes as C
    from gr_amps_amd import capi
    L = capi.load()
    bits = [getattr(capi, "FLAG_" + n) for n in FLAG_NAMES]
    cfg = capi.Cfg()
    cfg.struct_size = C.sizeof(capi.Cfg)
    cfg.max_bursts, cfg.device = 1, -1
    h = C.c_void_p()
    create, ref = L.amps_recc_create, (C.byref(h), C.byref(cfg))
    codes = []
    for M, D, sps, taps, n, first, groups, group, max_samples, f in sweep():
        cfg.wideband_channels, cfg.wideband_decim, cfg.samples_per_symbol, cfg.wideband_taps_per_branch, cfg.n_channels = M, D, sps, taps, n
        cfg.wideband_first_channel, cfg.wideband_groups, cfg.wideband_group, cfg.max_samples_per_push = first, groups, group, max_samples
        cfg.flags = sum(b for i, b in enumerate(bits) if f >> i & 1)
        codes.append(create(*ref))
        if h.value:
            raise SystemExit("a handle was created: this comparison is for a machine without a GPU")
    np.save(out_path, np.asarray(codes, np.int16))


def late_case(M, D, sps, taps, n, first, groups, group, max_samples, f):
    """which of the parent's checks behind the device refuses this cfg; None: none of them"""
    G = max(groups, 1)
    if M == 1024 and taps not in (0, 8):
        return "1024 bank, taps_per_branch not 0 or 8"
    if M == 1024 and n > 1024:
        return "n_channels > 1024"
    if M == 1024 and first >= 1024:
        return "first_channel >= 1024"
    if G not in (1, 2, 4, 8):
        return "groups not in {1, 2, 4, 8}"
    if group >= G:
        return "group >= groups"
    if G > 1 and f & 1:
        return "a group handle with UNFUSED_WIDEBAND"
    if G > 1 and not any(((first + c) % M) % 64 // (64 // G) == group for c in range(n)):
        return "a group with no rows"
    return None


def main(old, new):
    codes = []
    for i, lib in enumerate((old, new)):
        path = "/tmp/chz_cfg_identity_%d_%d.npy" % (os.getpid(), i)
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], check=True, env=dict(os.environ, AMPS_RECC_LIB=os.path.abspath(lib)))
        codes.append(np.load(path))
        os.remove(path)
    a, b = codes
    diff = np.flatnonzero(a != b)
    print("cfgs %d  equal codes %d  different %d" % (a.size, a.size - diff.size, diff.size))
    for name, c in (("old", a), ("new", b)):
        print("%s: %s" % (name, "  ".join("%d x %d" % (int(v), int(k)) for v, k in zip(*np.unique(c, return_counts=True)))))
    want = set(int(i) for i in diff)
    cases, bad = {}, 0
    for i, cfg in enumerate(sweep()):
        if i not in want:
            continue
        case = late_case(*cfg) if (a[i], b[i]) == (-19, -22) else None
        line = "%d -> %d  channels %d decim %d sps %d taps %d n_channels %d first %d groups %d group %d max_samples %d flags %s" % (
            (a[i], b[i]) + cfg[:9] + ("|".join(n for k, n in enumerate(FLAG_NAMES) if cfg[9] >> k & 1) or "0",))
        if case is None:
            print("UNEXPLAINED  index %d  %s" % (i, line))
            bad += 1
            continue
        first, idx = cases.setdefault(case, (line, []))
        idx.append(i)
    for case, (first, idx) in sorted(cases.items()):
        idx = np.asarray(idx)
        starts = np.flatnonzero(np.diff(idx, prepend=-2) != 1)
        ends = np.append(starts[1:], idx.size) - 1
        print("\n%s: %d cfgs, every one -19 -> -22\n  first: index %d  %s" % (case, idx.size, idx[0], first))
        runs = ["%d-%d" % (idx[s], idx[e]) if e > s else "%d" % idx[s] for s, e in zip(starts, ends)]
        for k in range(0, len(runs), 12):
            print("  " + " ".join(runs[k:k + 12]))
    return bad


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        sys.exit(1 if main(sys.argv[1], sys.argv[2]) else 0)
