"""No GPU: amps_recc_set_wideband_shift / amps_recc_wideband_shift -- a tuner's frequency error corrected inside the filter banks below
1024 branches.  The header and the binding, the argument checks and the step arithmetic as a stand-alone program under sanitizers, the
mixing twins' register / LDS budget against the kernels they twin, and, on the models, that the inputs of
tests/test_gpu_wideband_shift.py need the feature and that the binary32 mixer stays inside the error bound the GPU test then uses."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from oracle import channelizer as cz
from gr_amps_amd import build, capi

import grid10block as gb
import narrowblock as nb
import shiftblock as shb
import slicerbound as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gr_amps_amd", "csrc")


# ---- 1. header, exports, errors
def test_header_and_binding_name_both_calls():
    hdr = open(os.path.join(ROOT, "include", "amps_recc.h")).read()
    assert "int amps_recc_set_wideband_shift(amps_recc_t *h, double shift_hz);" in hdr
    assert "int amps_recc_wideband_shift(const amps_recc_t *h, double *shift_hz);" in hdr
    assert re.search(r"#define AMPS_RECC_ABI_VERSION 4\b", hdr)
    assert "still 4, two entry points added and nothing changed: amps_recc_set_wideband_shift / amps_recc_wideband_shift" in hdr
    assert "amps_recc_set_wideband_shift" in capi.EXPORTS and "amps_recc_wideband_shift" in capi.EXPORTS
    assert callable(capi.Recc.set_wideband_shift) and isinstance(capi.Recc.wideband_shift, property)
    if os.path.exists(capi.LIB_PATH):
        L = capi.load()
        assert L.amps_recc_abi_version() == 4
        assert L.amps_recc_set_wideband_shift(None, 1e3) == -22 and L.amps_recc_wideband_shift(None, None) == -22   # -EINVAL: no handle


def test_argument_checks_stand_alone_under_sanitizers(tmp_path):
    """gr_amps_amd/csrc/recc_wideband_shift.h is free of HIP: tests/wideband_shift_host.cc has its own main, is compiled with
    -fsanitize=address,undefined and run as a program of its own -- every refusal, steps of 0, +- fs / 4 and fs / 2, a negative
    shift's two's complement, and the value read back within fs 2^-64 of what was set.  Which bank has a shift is the bank table's word
    (recc_chz_banks.h, CHZ_HAS_SHIFT), handed over as the library hands it: every bank below 1024 branches, and not the 1024 bank"""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "wideband_shift_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "wideband_shift_host.cc"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "wideband shift ok" in out


# ---- 2. kernel resources and names
_TWIN = {"float2": "HIP_vector_type<float, 2u>"}


def test_mixing_twins_fit_their_originals_budget():
    """every chz_narrow_mix_kernel / chz_grid10_mix_kernel instantiation: no scratch, no spilled register, static LDS no larger and waves
    per SIMD not fewer than the unmixed kernel of the same geometry and sample type; the old names count what they counted"""
    if not os.path.exists(build.hipcc()) or not shutil.which("c++filt"):
        if not os.path.exists(build.RESOURCES):
            pytest.skip("hipcc / c++filt not installed and no cached kernel_resources.json")
    res = build.kernel_resources()
    narrow = {k: v for k, v in res.items() if k.startswith("void amps::chz_narrow_mix_kernel<")}
    grid = {k: v for k, v in res.items() if k.startswith("void amps::chz_grid10_mix_kernel<")}
    assert len(narrow) == 24 and len(grid) == 16, (sorted(narrow), sorted(grid))     # six geometries, four sizes x four sample types
    assert sum(k.startswith("void amps::chz_narrow_kernel<") for k in res) == 12
    assert sum(k.startswith("void amps::chz_narrow_b8_kernel<") for k in res) == 12
    assert sum(k.startswith("void amps::chz_grid10_kernel<") for k in res) == 16
    seen = set()
    for name, r in list(narrow.items()) + list(grid.items()):
        m = re.match(r"void amps::chz_(narrow|grid10)_mix_kernel<(.*)>\(amps::ChzMixArgs\)$", name)
        assert m, name
        kind, targs = m.groups()
        twin = "void amps::chz_%s_kernel<%s>(amps::ChzNarrowArgs)" % (kind, targs)
        if twin not in res:
            twin = twin.replace("chz_narrow_kernel<", "chz_narrow_b8_kernel<")       # the 8-bit types of the narrow banks
        assert twin in res, (name, twin)
        seen.add(twin)
        o = res[twin]
        assert r["scratch_bytes_per_lane"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["lds_bytes"] <= o["lds_bytes"], (name, r, o)
        assert r["waves_per_simd"] >= o["waves_per_simd"], (name, r, o)
    assert len(seen) == 40                                                             # every unmixed kernel has exactly one twin


def test_twins_add_no_inline_assembly_and_leave_every_kernel_as_it_was():
    """the twins are the bodies' text with one call in the staging loop (recc_chz_stage.inc, which both bodies include); what that call adds is plain C++ (xl_mix as it stands).  The
    committed ISA comparison with the parent: nothing changed, nothing removed, the forty new names added"""
    for f in ("recc_chz_narrow_body.inc", "recc_chz_grid10_body.inc", "recc_chz_stage.inc", "recc_wideband_shift.h"):
        assert not re.search(r"\basm\b", open(os.path.join(CSRC, f)).read()), f
    narrow = open(os.path.join(CSRC, "recc_chz_narrow.hip.h")).read()
    mix = narrow[narrow.index("struct ChzMixArgs"):narrow.index("__host__ __device__ constexpr bool chz_narrow_geometry")]
    assert "chz_mix_staged" in mix and "xl_mix(" in mix and not re.search(r"\basm\b", mix)
    txt = open(os.path.join(ROOT, "profiles", "wideband_shift", "isa_identity.txt")).read()
    assert re.search(r"changed 0\s+removed 0\s+added 40\b", txt), txt[:200]
    added = re.findall(r"^added.*?: void amps::(\w+)<", txt, re.M)
    assert len(added) == 40 and set(added) == {"chz_narrow_mix_kernel", "chz_grid10_mix_kernel"}


# ---- 3. the GPU tests' inputs need the feature
def _decoded(rows, sps, truth):
    recs = oracle.fused_push_all(np.ascontiguousarray(rows).astype(np.complex64), sps=sps)
    mins = sorted(v[1] for v in truth.values())
    return len(recs), sorted(a["min"].decode() for a in recs if a["min"].decode() in mins), mins


def _narrow_rows(x, M, D):
    return cz.channelize(x, P=8, M=M, D=D, taps=nb.taps(M, D))[[k for k, _ in nb.planted(M)]]


def _grid_rows(x, M):
    bins = gb.row_bins(M, gb.FIRST, gb.max_channels(M))
    return cz.channelize(x, M=M, D=gb.decim(M), taps=gb.taps(M))[[int(bins[r]) for r, _ in gb.planted(M)]]


@pytest.mark.parametrize("case", ["M128-D96+9k", "M500+9k", "M500-9k"])
def test_a_9_khz_tuner_error_decodes_nothing_and_the_mixer_brings_all_six_back(case):
    """float64 bank, then oracle.fused_push_all: the block as delivered gives none of the six planted MINs; mixed back by the numpy
    binary32 statement of the mixer it gives all six"""
    if case.startswith("M128"):
        M, D, cfo = 128, 96, 9e3
        x, truth = nb.burst_block(M, D, cfo_hz=cfo)
        fs, rows = M * 30e3, lambda v: _narrow_rows(v, M, D)
    else:
        M, cfo = 500, (9e3 if case.endswith("+9k") else -9e3)
        x, truth = gb.burst_block(M, cfo_hz=cfo)
        fs, rows = M * gb.BIN_HZ, lambda v: _grid_rows(v, M)
    n_recs, good, mins = _decoded(rows(x), 2, truth)
    assert len(mins) == 6 and good == [], (n_recs, good)
    n_recs, good, _ = _decoded(rows(shb.mix32(x, shb.step_of(cfo, fs))), 2, truth)
    assert good == mins and n_recs == 6, (n_recs, good)


# ---- 4. the error bound, before any GPU run
def _bound_case(x, M, D, h, shift_hz, fs):
    step = shb.step_of(shift_hz, fs)
    P = h.size // M
    y32 = cz.channelize(shb.mix32(x, step), P=P, M=M, D=D, taps=h)
    y64 = cz.channelize(shb.mix64(x, step), P=P, M=M, D=D, taps=h)
    err = np.abs(y32 - y64)                                                  # [M][frames]
    unit = sb.U32 * np.log2(M) * np.sqrt((np.abs(y64) ** 2).sum(0))          # per frame
    allowed = shb.DELTA * shb.frame_weights(x, h, D)                         # per frame
    return err, unit, allowed


@pytest.mark.parametrize("shift_hz", shb.SHIFTS)
@pytest.mark.parametrize("geom", ["M500", "M128-D96", "M128-D64"])
def test_binary32_mixer_stays_inside_the_bound(geom, shift_hz):
    """|bank64(mix32(x)) - bank64(mix64(x))| <= DELTA sum_i |h[i]| |x[n0 + i]| for every bin and frame, DELTA = (2 pi + 5 sqrt 2) 2^-24
    from the mixer's code (tests/shiftblock.py): the part of a shifted handle's error that slicerbound.FFT_C, the banks' own constant,
    does not cover.  A shifted handle is held to FFT_C unit + that sum.  In the unit 2^-24 log2(M) ||Y64(frame)||_2 the mixer's part
    came out at 0.13 - 0.15 (M = 500, tone block) and 0.26 - 0.28 (M = 128, tests/shiftblock.py's tone block) -- on top of the banks'
    own 0.09 - 0.17, against FFT_C = 0.54 -- and at 0.08 - 0.14 of what DELTA allows."""
    if geom == "M500":
        M, D = 500, gb.decim(500)
        x, h, fs = gb.tone_block(M), gb.taps(M), M * gb.BIN_HZ
    else:
        M, D = 128, int(geom.split("D")[1])
        x, h, fs = shb.narrow_tone_block(M, D), nb.taps(M, D), M * 30e3
    err, unit, allowed = _bound_case(x, M, D, h, shift_hz, fs)
    live = slice(h.size // D + 1, None)                                      # frames whose whole history is signal
    in_units = (err / unit)[:, live].max()
    of_bound = (err / allowed)[:, live].max()
    print(f"\n{geom} shift {shift_hz:+.2f} Hz: mixer's part {in_units:.3f} units, {of_bound:.3f} of DELTA's allowance")
    assert np.all(err <= allowed + 1e-300)
    assert of_bound < 1.0 and in_units > 0.05                                # ... and it is not nothing: FFT_C alone would not do
