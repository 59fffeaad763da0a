"""not gpu: the table of filter banks and the one verdict on a cfg's wideband fields (gr_amps_amd/csrc/recc_chz_banks.h) in a
stand-alone host program under the address and undefined-behaviour sanitizers, and what that program prints against a statement of
the banks and of the admission rules written out here.  Neither side is derived from the other: the header is C++ compiled from the
library's sources; the expectations below are DESIGN.md 4.2e-g and the comments of include/amps_recc.h on the wideband_* fields, and
the geometry constants the bank tests already keep (narrowblock, narrowstream, grid10block)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import grid10block as gb
import narrowblock as nb
import narrowstream as ns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the sweep, in the order of the program's loops (M = wideband_channels; uint32 arithmetic: M - 1 wraps at M = 0)
CHANNELS = (0, 64, 127, 128, 129, 256, 300, 500, 512, 1000, 1024, 2000, 2048, 2500, 3000)
U32 = 0xffffffff
UNFUSED, CHANNEL_POWER, STREAM_POWER = 1, 2, 4                    # bits of the sweep's flag index, not the ABI's values


def axes(M):
    return dict(decim=(0, M // 4, M // 4 + 1, M // 2, 3 * M // 4, M, 768), sps=(0, 2, 3, 10), taps=(0, 3, 5, 8), n=(1, M // 3, M // 3 + 1, M, M + 1),
                first=(0, (M - 1) & U32, M), groups=(0, 1, 2, 3, 8, 16), group=(0, 1, -1), max_samples=(0, 1024), flags=tuple(range(8)))


WIDTHS = (3, 4, 2, 1, 4)                                            # "verdict decim sps taps rows", right-aligned
LINE = sum(WIDTHS) + len(WIDTHS)
PER_M = int(np.prod([len(v) for v in axes(0).values()]))

# ---- the banks, as the documents state them
# 30 kHz bins, a channel on every bin, eight taps per branch, D = 3 M / 4 (the default) or M / 2; the 1024 bank has the fused form
# and with it channel groups, CHANNEL_POWER and RCCL; the narrow banks the tuner shift and the IQ seam's STREAM_* rings instead.
# 10 kHz bins, a channel on every third, three taps per branch, D = M / 4 and no default; otherwise like the narrow banks.
F_FUSED, F_GROUPS, F_CHANNEL_POWER, F_RCCL, F_SHIFT, F_STREAM = (1 << i for i in range(6))
BANKS = {1024: dict(family=0, bin_hz=30000, stride=1, taps=8, decims=(768, 512), default=768, features=F_FUSED | F_GROUPS | F_CHANNEL_POWER | F_RCCL, fr={})}
for M_ in (512, 256, 128):
    BANKS[M_] = dict(family=1, bin_hz=30000, stride=1, taps=8, decims=(3 * M_ // 4, M_ // 2), default=3 * M_ // 4, features=F_SHIFT | F_STREAM,
                     fr={D: ns.FR[(M_, D)] for D in (3 * M_ // 4, M_ // 2)})
for M_ in gb.SIZES:
    BANKS[M_] = dict(family=2, bin_hz=int(gb.BIN_HZ), stride=gb.STRIDE, taps=gb.P, decims=(gb.decim(M_),), default=0, features=F_SHIFT | F_STREAM,
                     fr={gb.decim(M_): 8 if M_ == 500 else 4})   # recc_chz_grid10.hip.h, "FR, LDS ...": M = 500: FR = 8, else 4


def rows_of(M, stride, n, first, G, group):
    """rows of a handle: the channels c < n of the band whose bin (first + stride c) mod M lies in the handle's group -- blocks of
    64 / G adjacent bins, every 64 (include/amps_recc.h, wideband_groups)"""
    k = (first + stride * np.arange(n)) % M
    return int(((k % 64) // (64 // G) == group).sum())


def expected(M):
    """(verdict, decim, sps, taps, rows) for every cfg of the sweep at wideband_channels = M, in the program's order"""
    ax = axes(M)
    g = np.meshgrid(*[np.asarray(v, np.int64) for v in ax.values()], indexing="ij")
    D, sps, taps, n, first, groups, group, max_samples, flags = [a.ravel() for a in g]
    group = np.where(group < 0, groups, group)
    ok = np.ones(D.size, bool)
    rows = n.copy()
    bank = BANKS.get(M)
    if M and bank is None:
        ok[:] = False                                              # "other values: -EINVAL"
    if bank:
        # decimation: one of the bank's, 0 = its default where it has one; samples per symbol: what that decimation delivers --
        # bin_hz M / D per channel over 20 k symbols per second -- or 0 for it; taps per branch: the bank's, or 0 for them
        D = np.where(D == 0, bank["default"], D)
        ok &= np.isin(D, bank["decims"])
        want_sps = np.where(ok, bank["bin_hz"] * M // np.maximum(D, 1) // 20000, 0)
        ok &= (sps == 0) | (sps == want_sps)
        sps = want_sps
        ok &= (taps == 0) | (taps == bank["taps"])
        taps = np.full_like(taps, bank["taps"])
        ok &= max_samples != 0                                     # the wideband seam needs its frame capacity
        ok &= (n >= 1) & (bank["stride"] * n <= M) & (first < M)   # "3 n_channels <= M", "first FFT bin ..., < M"
        # groups: 0 / 1 = the whole band selection (the only group is 0); 2, 4 or 8 on a bank with the fused form, in that form
        G = np.maximum(groups, 1)
        ok &= np.isin(G, (1, 2, 4, 8)) & (group < G)
        ok &= (G == 1) | (bool(bank["features"] & F_GROUPS) & ((flags & UNFUSED) == 0))
        cache = {}
        for i in np.flatnonzero(ok):
            key = (int(n[i]), int(first[i]), int(G[i]), int(group[i]))
            if key not in cache:
                cache[key] = rows_of(M, bank["stride"], *key)
            rows[i] = cache[key]
        ok &= rows >= 1                                            # a group that owns none of the band's channels is no handle
    # CHANNEL_POWER: behind the fused filter bank only; STREAM_POWER: the IQ seam's ring, for handles without a fused bank, and a
    # handle has at most one of the two flags
    has = bank["features"] if bank else 0
    ok &= ((flags & CHANNEL_POWER) == 0) | (bool(has & F_CHANNEL_POWER) & ((flags & UNFUSED) == 0))
    ok &= ((flags & STREAM_POWER) == 0) | ((bool(has & F_STREAM) or not M) & (max_samples != 0) & ((flags & CHANNEL_POWER) == 0))
    out = np.stack([np.where(ok, 0, -22), D, sps, taps, rows], axis=1)
    out[~ok, 1:] = 0
    return out


def parse(chunk):
    """int64 [lines][5] of whole sweep lines"""
    a = np.frombuffer(chunk, np.uint8).reshape(-1, LINE)
    seps = np.cumsum(WIDTHS) + np.arange(len(WIDTHS))
    assert (a[:, seps[:-1]] == ord(" ")).all() and (a[:, seps[-1]] == ord("\n")).all()
    digit = np.full(256, -1, np.int64)
    digit[[ord(" "), ord("-")]] = 0
    digit[ord("0"):ord("9") + 1] = np.arange(10)
    out = np.zeros((a.shape[0], len(WIDTHS)), np.int64)
    for f in range(len(WIDTHS)):
        for col in range(seps[f] - WIDTHS[f], seps[f]):
            d = digit[a[:, col]]
            assert d.min() >= 0
            out[:, f] = out[:, f] * 10 + d
    out[:, 0] = np.where(a[:, 0] == ord("-"), -out[:, 0], out[:, 0])
    return out


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    """(the table's lines, the sweep's bytes, the last line) of tests/chz_banks_host.cc, compiled with -fsanitize=address,undefined and
    run as a program of its own"""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("chz_banks") / "chz_banks_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "gr_amps_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "chz_banks_host.cc"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout
    start = 0
    while out[start:start + 5] in (b"bank ", b"geom "):
        start = out.index(b"\n", start) + 1
    end = start + LINE * PER_M * len(CHANNELS)
    return out[:start].decode().splitlines(), out[start:end], out[end:].decode()


def test_the_table_is_the_banks_the_tests_already_keep(printed):
    head, _, tail = printed
    assert tail.startswith("chz banks ok: %d cfgs, " % (PER_M * len(CHANNELS)))
    assert [int(l.split()[1]) for l in head if l.startswith("bank ")] == [1024, 512, 256, 128] + list(gb.SIZES)   # the plan calls' order: 30 kHz banks first
    seen_geoms = []
    for l in head:
        w = l.split()
        if w[0] == "bank":
            M, want = int(w[1]), BANKS[int(w[1])]
            d, fr = (int(w[13]), int(w[14])), (int(w[16]), int(w[17]))
            got = dict(family=int(w[3]), features=int(w[5]), bin_hz=int(w[7]), stride=int(w[9]), taps=int(w[11]), decims=tuple(x for x in d if x), default=int(w[19]),
                       fr={D: f for D, f in zip(d, fr) if D and f})
            assert got == want, (M, got, want)
            assert int(w[21]) == M // want["stride"] and int(w[23]) == M * want["bin_hz"]
            if want["family"] == 2:
                assert int(w[21]) == gb.max_channels(M)
        else:
            M, D = int(w[1]), int(w[2])
            b = BANKS[M]
            sps = 3 if 2 * D == M else 2                           # 60 ksps per channel at D = M / 2, 40 ksps at 3 M / 4 and on the 10 kHz grid
            assert b["bin_hz"] * M == sps * 20000 * D
            hist = b["taps"] * M - D + (4 * D if M == 1024 else 0)  # L - D, and the fused bank's pre-roll of four frames
            period = {2: 2, 4: 4}[M // np.gcd(M, D)]
            assert w[3:] == ["sps", str(sps), "cutoff", "15000" if sps == 2 else "13000", "hist", str(hist), "carry_cap", str(hist + 64 * D),
                             "period", str(period), "mask", str(period - 1), "fused_mask", "63"], l
            seen_geoms.append((M, D))
    assert sorted(seen_geoms) == sorted([(1024, 768), (1024, 512)] + nb.GEOMETRIES + [(M, gb.decim(M)) for M in gb.SIZES])
    assert sorted(g for g in seen_geoms if BANKS[g[0]]["family"] == 1) == sorted(nb.GEOMETRIES) == sorted(ns.FR)


def test_every_verdict_of_the_sweep_is_the_documents(printed):
    _, sweep, _ = printed
    assert len(sweep) == LINE * PER_M * len(CHANNELS)
    admitted = 0
    for i, M in enumerate(CHANNELS):
        got = parse(sweep[i * LINE * PER_M:(i + 1) * LINE * PER_M])
        want = expected(M)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (M, bad[:5], got[bad[:5]], want[bad[:5]])
        admitted += int((want[:, 0] == 0).sum())
    # every bank admits something in the sweep, and so does a handle without the seam
    assert admitted > 0 and all((expected(M)[:, 0] == 0).any() for M in (0,) + tuple(BANKS))
    print("chz_resolve_cfg: %d cfgs checked, %d admitted" % (PER_M * len(CHANNELS), admitted))
