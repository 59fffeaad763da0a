"""not gpu: the 16-bit I/Q form of the wideband seam (amps_recc_push_wideband_short, include/amps_recc.h) as far as it can be
checked without a device -- the symbol and its argument validation, the register / LDS budget of the eight chz12_short_kernel
instantiations, and the scan of tests/test_cpu_inflight_loads.py restated for them.

The sc16 fold role loads a packed sample with an untracked `buffer_load_dword` into the LOW register of the ring slot's own pair and
expands it in place (two v_cvt_f32_i32 with a word select) behind the manual wait that covers it (recc_chz_fold.hip.h: chz_load1_ring,
chz_expand_short, chz_ring_wait).  That expansion is exactly the kind
of instruction the scan exists for: moved in front of its wait, or fed from a copy, it would read a register whose load has not
landed.  The walk is the one of test_cpu_inflight_loads.py (straight through the text, on at the loop's latch), the load pattern is
`buffer_load_dword` with a single destination register."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from gr_amps_amd import build, capi

KERNEL = re.compile(r"^(_ZN4amps18chz12_short_kernel\w+):")
LOAD = re.compile(r"\s*buffer_load_dword (v\d+), v\d+, s\[")
LATCH = re.compile(r"\s*s_branch\s+(\.LBB\d+_\d+)")
WAIT = re.compile(r"\s*s_waitcnt vmcnt\((\d+)\)")


def test_symbol_is_exported_and_validates_without_a_device():
    L = capi.load()
    assert "amps_recc_push_wideband_short" in capi.EXPORTS
    assert L.amps_recc_push_wideband_short is not None
    buf = (C.c_int16 * 8)()
    assert L.amps_recc_push_wideband_short(None, None, 0, 0) == -22          # -EINVAL: no handle, whatever the rest
    assert L.amps_recc_push_wideband_short(None, buf, 4, 0) == -22
    assert L.amps_recc_abi_version() == 4


# ---- kernel resources
@pytest.fixture(scope="module")
def res():
    if not os.path.exists(build.hipcc()) or not shutil.which("c++filt"):
        if os.path.exists(build.RESOURCES):
            import json
            with open(build.RESOURCES) as f:
                return json.load(f)
        pytest.skip("hipcc / c++filt not installed and no cached kernel_resources.json")
    return build.kernel_resources()


def test_short_filter_bank_kernel_budget(res):
    hits = {k: v for k, v in res.items() if k.startswith("void amps::chz12_short_kernel<8, ")}
    assert len(hits) == 8, sorted(hits)                               # fused only: four slicer specs at either decimation
    for name, r in hits.items():
        assert "<8, -1, " not in name, name                           # the unfused form takes an sc16 block through the conversion kernel
        # the spill budget of the fc32 twin (tests/test_cpu_kernel_resources.py)
        spill_ok = 16 if "<8, 3, 512>" in name else 12 if ", 768>" in name else 0
        assert r["vgprs"] <= 168 and r["scratch_bytes_per_lane"] <= 4 * spill_ok and r["vgpr_spill"] <= spill_ok, (name, r)
        assert r["waves_per_simd"] == 3, (name, r)
        assert r["lds_bytes"] <= 160 * 1024, (name, r)
    # the conversion kernel of the checking modes is there, small and spill-free
    cv = {k: v for k, v in res.items() if k.startswith("amps::chz_short_to_float_kernel(")}
    assert len(cv) == 1 and all(r["scratch_bytes_per_lane"] == 0 and r["vgprs"] <= 32 for r in cv.values()), cv


# ---- in-flight loads
def _regs(tok):
    m = re.match(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"v(\d+)$", tok)
    return {int(m.group(1))} if m else set()


def _named(t):
    used = set()
    for tk in re.findall(r"v\[\d+:\d+\]|v\d+", t):
        used |= _regs(tk)
    return used


def scan(asm_text):
    """Per chz12_short_kernel instantiation: (name, asm loads, waits of the loop that holds them, hazards) -- see
    tests/test_cpu_inflight_loads.py::scan, whose walk this is."""
    txt = asm_text.split("\n")
    out, i = [], 0
    while i < len(txt):
        m = KERNEL.match(txt[i])
        if not m:
            i += 1
            continue
        j = i
        while j < len(txt) and not txt[j].startswith(".Lfunc_end"):
            j += 1
        lines = txt[i:j]
        labels = {}
        for k, l in enumerate(lines):
            lm = re.match(r"^(\.LBB\d+_\d+):", l)
            if lm:
                labels[lm.group(1)] = k
        loads = [(k, _regs(LOAD.match(l).group(1))) for k, l in enumerate(lines) if LOAD.match(l)]
        waits = [k for k, l in enumerate(lines) if WAIT.match(l) and int(WAIT.match(l).group(1)) in (8, 13)]
        loop = [w for n, w in enumerate(waits) if any(w < k < (waits[n + 1] if n + 1 < len(waits) else w + 2000) for k, _ in loads)]
        issues = []
        for k, dst in loads:
            pos, younger, latched, covered, steps = k + 1, 0, set(), False, 0
            while pos < len(lines) and steps < 50000:
                steps += 1
                t = lines[pos].strip()
                wm = WAIT.match(lines[pos])
                lm = LOAD.match(lines[pos])
                if wm and younger >= int(wm.group(1)):
                    covered = True
                    break
                if lm:
                    younger += 1
                    if _regs(lm.group(1)) & dst:
                        issues.append((m.group(1), k + 1, pos + 1, "loaded again before the covering wait: " + t))
                        covered = True
                        break
                elif t and t[0] not in ";.":
                    if _named(t) & dst:
                        issues.append((m.group(1), k + 1, pos + 1, t))
                        covered = True
                        break
                    bm = LATCH.match(lines[pos])
                    if bm and labels.get(bm.group(1), len(lines)) < pos and pos not in latched:
                        latched.add(pos)
                        pos = labels[bm.group(1)]
                        continue
                    if "s_endpgm" in t:
                        break
                pos += 1
            if not covered:
                issues.append((m.group(1), k + 1, pos, "path left the kernel before the covering wait"))
        out.append((m.group(1), len(loads), len(loop), issues))
        i = j
    return out


def test_scanner_sees_a_planted_hazard():
    # the expansion in front of the wait that covers its load
    asm = "\n".join(["_ZN4amps18chz12_short_kernelXX:", ".LBB0_1:", "s_waitcnt vmcnt(1)", "buffer_load_dword v10, v1, s[4:7], s8 offen",
                     "v_cvt_f32_i32_sdwa v11, sext(v10) dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1", "s_cbranch_scc1 .LBB0_1", "s_barrier",
                     "s_waitcnt vmcnt(1)", "buffer_load_dword v12, v1, s[4:7], s8 offen offset:1024", "s_barrier", "s_branch .LBB0_1",
                     "v_add_f32 v0, v10, v12", ".Lfunc_end0:"])
    res = scan(asm)
    assert len(res) == 1 and len(res[0][3]) == 1 and "v_cvt_f32_i32_sdwa" in res[0][3][0][3]
    # a spill store of a register whose load is in flight, and the same code with the store behind the covering wait
    bad = ["_ZN4amps18chz12_short_kernelYY:", ".LBB1_1:", "s_waitcnt vmcnt(1)", "buffer_load_dword v10, v1, s[4:7], s8 offen",
           "scratch_store_dword off, v10, off", "buffer_load_dword v12, v1, s[4:7], s8 offen", "s_waitcnt vmcnt(0)", "s_endpgm", ".Lfunc_end1:"]
    good = bad[:4] + bad[5:7] + [bad[4]] + bad[7:]
    assert any("scratch_store" in h[3] for h in scan("\n".join(bad))[0][3]) and not scan("\n".join(good))[0][3]
    # a copy of the slot's PAIR while its low half is in flight
    pair = bad[:4] + ["v_mov_b64_e32 v[20:21], v[10:11]"] + bad[5:]
    assert any("v_mov_b64" in h[3] for h in scan("\n".join(pair))[0][3])


@pytest.fixture(scope="module")
def asm_text():
    if not os.path.exists(build.hipcc()):
        pytest.skip("hipcc not installed")
    flags = [f for f in build.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "amps.s")
        subprocess.run([build.hipcc()] + flags + ["--cuda-device-only", "-S", "-I" + os.path.join(build._ROOT, "include"), "-I" + build.CSRC,
                                                  os.path.join(build.CSRC, "amps_recc.hip"), "-o", out],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out).read()


def test_no_register_with_a_load_in_flight_is_touched(asm_text):
    res = scan(asm_text)
    assert len(res) == 8, [r[0] for r in res]                      # four slicer specs at D = 512 and at D = 768, fused
    for name, nloads, nwaits, issues in res:
        if "Li768E" in name:
            assert nloads == 48 and nwaits == 8, (name, nloads, nwaits)   # four unrolled half-steps of twelve loads and two waits
        else:
            assert nloads == 48 and nwaits == 6, (name, nloads, nwaits)   # six unrolled half-steps of eight loads
        assert not issues, (name, issues[:4])


def test_every_packed_sample_is_expanded_in_place(asm_text):
    """two conversions per loaded sample in the steady loop of the fold role -- the high word into the upper register of the slot's pair,
    then the low word over its own source -- and nothing else converts there: 48 pairs per instantiation (the compiler's own
    conversions, of the edge loader, lie outside the unrolled loop and are not counted)"""
    txt = asm_text.split("\n")
    cvt = re.compile(r"\s*v_cvt_f32_i32_sdwa v(\d+), sext\(v(\d+)\) .*src0_sel:WORD_([01])")
    i, seen = 0, 0
    while i < len(txt):
        m = KERNEL.match(txt[i])
        if not m:
            i += 1
            continue
        j = i
        while j < len(txt) and not txt[j].startswith(".Lfunc_end"):
            j += 1
        lines = [l for l in txt[i:j] if l.strip() and l.strip()[0] not in ";."]
        at = [k for k, l in enumerate(lines) if LOAD.match(l)]
        pairs, k = 0, 0
        while k < len(lines):
            hi = cvt.match(lines[k])
            lo = cvt.match(lines[k + 1]) if hi and k + 1 < len(lines) else None
            inplace = bool(lo) and hi.group(3) == "1" and lo.group(3) == "0" and hi.group(2) == lo.group(2) == lo.group(1) \
                and int(hi.group(1)) == int(lo.group(1)) + 1
            if at[0] <= k <= at[-1] and hi:
                assert inplace, (m.group(1), lines[k], lines[k + 1])     # inside the unrolled loop: only the in-place expansion
            if inplace and at[0] - 400 <= k <= at[-1] + 400:
                pairs += 1
                k += 2
            else:
                k += 1
        assert pairs == 48, (m.group(1), pairs)
        seen += 1
        i = j
    assert seen == 8


def role_bodies_with_scratch(asm):
    """tests/test_cpu_inflight_loads.py::role_bodies_with_scratch for the new kernel name.  The expanding waits of the sc16 fold role
    sit behind a wave-uniform branch each, which cuts a fold half-step into blocks of one frame pair (64 tap v_pk_fma_f32 + 6 twiddle
    ones): a fold body is recognised from 60 v_pk_fma_f32 on, and may hold two branches."""
    txt = asm.split("\n")
    bad, bodies, i = [], 0, 0
    while i < len(txt):
        m = KERNEL.match(txt[i])
        if not m:
            i += 1
            continue
        j = i
        while j < len(txt) and not txt[j].startswith(".Lfunc_end"):
            j += 1
        cur, counts = None, {}
        for l in txt[i:j]:
            lm = re.match(r"^(\.LBB\d+_\d+):", l)
            if lm:
                cur = lm.group(1)
                counts[cur] = {"fma": 0, "add": 0, "align": 0, "scratch": 0, "edge": 0, "tests": 0}
                continue
            if cur is None:
                continue
            t = l.strip()
            c = counts[cur]
            c["fma"] += t.startswith("v_pk_fma_f32")
            c["add"] += t.startswith("v_pk_add_f32")
            c["align"] += t.startswith("v_alignbit_b32")
            c["scratch"] += t.startswith("scratch_")
            c["edge"] += bool(re.match(r"global_load_dword(x2)? v(\[\d+:\d+\]|\d+), v\[\d+:\d+\], off", t))
            c["tests"] += t.startswith("s_cbranch")
        steady = {b: c for b, c in counts.items() if not c["edge"] and c["tests"] <= 2 and (c["fma"] >= 60 or c["add"] >= 60 or c["align"] >= 20)}
        bodies += len(steady)
        bad += [(m.group(1), b, c) for b, c in steady.items() if c["scratch"]]
        i = j
    return bad, bodies


def test_scratch_scanner_sees_a_planted_spill():
    body = ["v_alignbit_b32 v1, v2, v3, 31"] * 24
    asm = "\n".join(["_ZN4amps18chz12_short_kernelXX:", ".LBB0_1:"] + body + [".LBB0_2:"] + body + ["scratch_load_dword v0, off, off"] + [".Lfunc_end0:"])
    bad, bodies = role_bodies_with_scratch(asm)
    assert [b for _, b, _ in bad] == [".LBB0_2"] and bodies == 2


def test_no_role_body_of_the_short_filter_bank_touches_scratch(asm_text):
    bad, bodies = role_bodies_with_scratch(asm_text)
    assert bad == [] and bodies >= 8 * 6, (bad, bodies)
    # and nothing between the first and the last untracked load of an instantiation -- the unrolled steady loop of the fold role -- is a
    # scratch access
    txt = asm_text.split("\n")
    i = 0
    while i < len(txt):
        m = KERNEL.match(txt[i])
        if not m:
            i += 1
            continue
        j = i
        while j < len(txt) and not txt[j].startswith(".Lfunc_end"):
            j += 1
        at = [k for k in range(i, j) if LOAD.match(txt[k])]
        assert at and not [txt[k] for k in range(at[0], at[-1]) if txt[k].strip().startswith("scratch_")], m.group(1)
        i = j
