"""not gpu: the window arithmetic of the block rings (gr_amps_amd/csrc/recc_ring_window.h: which entries a ring holds, which of them a
capture takes, how a range leaves the ring) in a stand-alone host program under the address and undefined-behaviour sanitizers, and
the table that program prints against the Python restatements the GPU tests of the four statistics trust.  Neither side is derived
from the other: the header is C++ compiled from the library's sources, the expectations below are powerref / streampowerref and the
window formula of include/amps_recc.h written out here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import powerref
import streampowerref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the table's lines are of one length, the numbers right-aligned: "rule slots origin n_done position sps lo hi j0 count"
WIDTHS = (1, 2, 4, 5, 5, 2, 3, 3, 3, 3)
LINE = sum(WIDTHS) + len(WIDTHS)
RULES = {ord("S"): (powerref.burst_window, powerref.first_snapshot), ord("B"): (streampowerref.burst_window, streampowerref.first_block)}
SLOTS, ORIGINS, SPS, STRIDE = (8, 64), (0, 64, 960, 1024), (2, 3, 10), 256


def grid_lines(slots):
    """lines of the grid for one (rule, slots): every n_done from origin on in steps of 64, every multiple of 37 in [origin, n_done]"""
    total = 0
    for origin in ORIGINS:
        for n_done in range(origin, origin + 3 * 256 * slots + 320 + 1, 64):
            total += (n_done // 37 - (origin + 36) // 37 + 1) * len(SPS)
    return total


def parse(chunk):
    """int64 [lines][fields] of whole table lines; the rule as its character code"""
    a = np.frombuffer(chunk, np.uint8).reshape(-1, LINE)
    seps = np.cumsum(WIDTHS) + np.arange(len(WIDTHS))
    assert (a[:, seps[:-1]] == ord(" ")).all() and (a[:, seps[-1]] == ord("\n")).all()
    value = np.full(256, -1, np.int64)                            # of a character behind the rule: digits, blanks and the newline only
    value[[ord(" "), ord("\n")]] = 0
    value[ord("0"):ord("9") + 1] = np.arange(10)
    d = value[a.T]                                                # [column][line]
    assert d[1:].min() >= 0
    out = np.empty((len(WIDTHS), a.shape[0]), np.int64)
    out[0] = a[:, 0]
    for f in range(1, len(WIDTHS)):
        out[f] = 0
        for col in range(seps[f] - WIDTHS[f], seps[f]):
            out[f] = out[f] * 10 + d[col]
    return out.T


def check(t, windows):
    """every line of t against the restatements; windows[rule][sps]: (j0, count) of burst_window by position"""
    rule, slots, origin, n_done, pos, sps, lo, hi, j0, count = t.T
    for code, (_, first_entry) in RULES.items():
        m = rule == code
        if not m.any():
            continue
        # include/amps_recc.h: snapshot j exists iff 256 j < produced, block j iff 256 (j + 1) <= produced; the held window is
        # [max(ceil(origin / 256), produced_entries - R / 256), produced_entries), and empty ([hi, hi)) where that maximum exceeds hi
        want_hi = -(-n_done[m] // STRIDE) if code == ord("S") else n_done[m] // STRIDE
        first = np.array([first_entry(o) for o in ORIGINS])[np.searchsorted(ORIGINS, origin[m])]
        want_lo = np.minimum(np.maximum(first, want_hi - slots[m]), want_hi)
        assert np.array_equal(hi[m], want_hi) and np.array_equal(lo[m], want_lo)
        for s in SPS:
            ms = m & (sps == s)
            w0, wn = windows[code][s][:, pos[ms]]
            held = (w0 >= lo[ms]) & (w0 + wn <= hi[ms]) & (wn > 0)       # every entry of the capture inside [lo, hi)
            assert np.array_equal(j0[ms], w0) and np.array_equal(count[ms], np.where(held, wn, 0))
    assert np.isin(rule, list(RULES)).all() and np.isin(slots, SLOTS).all() and np.isin(origin, ORIGINS).all() and np.isin(sps, SPS).all()
    assert (n_done >= origin).all() and ((n_done - origin) % 64 == 0).all() and (pos % 37 == 0).all() and (pos >= origin).all() and (pos <= n_done).all()


def test_ring_window_stand_alone_under_sanitizers_and_its_table_against_the_python_restatements(tmp_path):
    """tests/ring_window_host.cc has its own main, is compiled with -fsanitize=address,undefined and run as a program of its own: its
    fake rings pass, and every line of its table equals what powerref / streampowerref and the header's window formula give"""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "ring_window_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "gr_amps_amd", "csrc"),
                    "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "ring_window_host.cc"), "-o", exe], check=True)
    top = max(ORIGINS) + 3 * 256 * max(SLOTS) + 320
    windows = {code: {s: np.array([bw(p, s) for p in range(top + 1)], np.int64).T for s in SPS} for code, (bw, _) in RULES.items()}
    seen, tail = {}, b""
    with subprocess.Popen([exe], stdout=subprocess.PIPE) as proc:
        while True:
            chunk = proc.stdout.read(LINE << 18)
            end = chunk[::LINE].find(b"c")                        # behind the table's whole lines: "copy-outs ...", the fake rings' report
            if end >= 0:
                tail = chunk[end * LINE:] + proc.stdout.read()
                chunk = chunk[:end * LINE]
            if chunk:
                t = parse(chunk)
                check(t, windows)
                for key, n in zip(*np.unique(t[:, 0] * 256 + t[:, 1], return_counts=True)):
                    seen[divmod(int(key), 256)] = seen.get(divmod(int(key), 256), 0) + int(n)
            if end >= 0 or not chunk:
                break
    assert proc.returncode == 0
    assert "ring window ok" in tail.decode()
    assert seen, "the table is empty"
    assert seen == {(code, slots): grid_lines(slots) for code in RULES for slots in SLOTS}
    print("ring window table: %d lines checked" % sum(seen.values()))
