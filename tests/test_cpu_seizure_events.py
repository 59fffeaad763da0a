"""not gpu: the boundary of the seizure events (include/amps_recc_seizure.h: AMPS_RECC_FLAG_SEIZURE_EVENTS, amps_recc_drain_seizures --
the flag, the 32-byte event, the export, the ABI version) and their second statement (tests/seizureref.py) against the second statement of the captures
(tests/trackref.py) on the CPU model's slicer bits: one event per capture, in an earlier push than the capture, inside the delay
bound, with the DCC that refdecode.manchester reads from the same 14 symbols -- and none for a capture that completes in the push that
found it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
import refdecode
import seizureref
import trackref
from gr_amps_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPS, CUT = 10, 4096


def _header(name="amps_recc_seizure.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def test_the_header_has_the_flag_the_event_and_the_entry_point():
    """the extension header include/amps_recc_seizure.h, beside include/amps_recc.h, whose own flags and entry points stand as they were"""
    hdr, base = _header(), _header("amps_recc.h")
    assert re.search(r"#define\s+AMPS_RECC_FLAG_SEIZURE_EVENTS\s+0x2000u\b", hdr)
    assert re.search(r"#define\s+AMPS_SEIZURE_FLAG_DCC_COMPLETE\s+0x1u\b", hdr)
    assert re.search(r'#include\s+"amps_recc.h"', hdr) and re.search(r"#define\s+AMPS_RECC_ABI_VERSION\s+4\b", base)
    assert capi.FLAG_SEIZURE_EVENTS == 0x2000 and capi.SEIZURE_FLAG_DCC_COMPLETE == 1 == seizureref.DCC_COMPLETE
    # no flag of either header shares the bit, and it is the one behind the base header's highest
    flags = {n: int(v, 16) for n, v in re.findall(r"#define\s+(AMPS_RECC_FLAG_\w+)\s+(0x[0-9a-fA-F]+)u", base + hdr)}
    assert [n for n, v in flags.items() if v & 0x2000] == ["AMPS_RECC_FLAG_SEIZURE_EVENTS"]
    assert len(set(flags.values())) == len(flags) and sorted(flags.values())[-2:] == [0x1000, 0x2000]
    body = re.search(r"typedef struct amps_recc_seizure \{(.*?)\} amps_recc_seizure_t;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [" ".join(f.split()) for f in body.split(";") if f.strip()]
    assert fields == ["uint32_t channel", "uint32_t flags", "uint64_t position", "uint8_t dcc[7]", "uint8_t dcc_bad", "uint64_t found_at"]
    assert re.search(r"#define\s+AMPS_RECC_SEIZURE_BYTES\s+32\b", hdr)


def test_the_event_is_32_bytes_with_natural_alignment():
    dt = capi.SEIZURE_DTYPE
    assert dt.itemsize == 32
    assert [(n, dt.fields[n][1]) for n in dt.names] == [("channel", 0), ("flags", 4), ("position", 8), ("dcc", 16), ("dcc_bad", 23), ("found_at", 24)]
    assert dt == np.dtype([(n, seizureref.EVENT_DTYPE.fields[n][0]) for n in seizureref.FIELDS])        # the statement's fields, in the ABI's order


def test_the_export_is_in_the_table_and_the_abi_version_stands():
    """the binding's table of the extension headers' entry points (capi.EXTENSION_PROTOTYPES) against the declarations of
    include/amps_recc_seizure.h, as tests/test_cpu_capi_prototypes.py holds capi.PROTOTYPES to include/amps_recc.h"""
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S))
    decls = re.findall(r"^[ \t]*([A-Za-z_][\w \t]*?[ \t\*]+)(amps_(?:recc|bch)_\w+)\s*\(([^;{]*?)\)\s*;", code, flags=re.M)
    assert [d[1] for d in decls] == list(capi.EXTENSION_PROTOTYPES) == list(capi.EXTENSION_EXPORTS) == ["amps_recc_drain_seizures"]
    assert set(re.findall(r"\b(amps_(?:recc|bch)_[a-z_0-9]+)\s*\(", code)) == set(capi.EXTENSION_EXPORTS)
    assert not set(capi.EXTENSION_EXPORTS) & set(capi.EXPORTS)
    scalars = {"int": C.c_int, "size_t": C.c_size_t, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "double": C.c_double}
    for ret, name, params in decls:
        restype, argtypes = capi.EXTENSION_PROTOTYPES[name]
        params = [q.strip() for q in " ".join(params.split()).split(",")]
        assert ret.strip() == "int" and restype is C.c_int and len(params) == len(argtypes), (name, params)
        for q, t in zip(params, argtypes):
            if "*" in q:
                assert t is C.c_void_p or issubclass(t, C._Pointer), (name, q, t)
            else:
                assert t is scalars[q.replace("const", "").split()[0]], (name, q, t)
    assert capi.EXTENSION_PROTOTYPES["amps_recc_drain_seizures"][1] == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L = capi.load()
    fn = L.amps_recc_drain_seizures
    assert fn.restype is C.c_int and list(fn.argtypes) == capi.EXTENSION_PROTOTYPES["amps_recc_drain_seizures"][1]
    assert L.amps_recc_abi_version() == 4
    n = C.c_size_t(7)
    assert L.amps_recc_drain_seizures(None, None, 0, C.byref(n), None) == -22          # -EINVAL without a handle, no device touched


# ------------------------------------------------------------------------------------------------- the statement on the model's bits
@pytest.fixture(scope="module")
def stream():
    """slicer bits of the CPU model for three whole bursts at ten samples per symbol, and their captures by the second statement"""
    rng = np.random.default_rng(2024)
    plan, off = [], 5000
    for dcc in (1, 2, 3):
        _, _, _, _, words = synth.random_message(rng)
        bits = synth.burst_bits(words, dcc=dcc, rng=rng)
        plan.append((off, bits))
        off += 2 * SPS * len(bits) + 2777
    n = (off + 3000) // 64 * 64
    iq = synth.fsk_modulate(n, plan, sps=SPS, fs=20e3 * SPS, snr_db=25.0, rng=rng)
    f = oracle.Fused(0, SPS)
    f.push(iq, cap=8)
    g = f.taps()[2]
    assert len(g) == n
    caps = trackref.captures(g, SPS)
    assert len(caps) == 3
    return g, caps


def _first_boundary_with(nc, boundaries):
    """the index of the first push after which the second statement of the captures holds the capture n_c"""
    span = SPS * (trackref.CAPTURE_SYMS + 1) + trackref.TRACK_BLOCKS
    return next(k for k, n_k in enumerate(boundaries) if nc + span < n_k)


def test_every_capture_has_one_event_in_an_earlier_push_inside_the_delay_bound(stream):
    g, caps = stream
    boundaries = list(range(CUT, len(g) + 1, CUT))
    assert boundaries[-1] <= len(g)
    ev = seizureref.events(g, SPS, boundaries)
    assert sorted(int(p) for p in ev["position"]) == [nc for nc, _ in caps]           # exactly one event per capture, with its n_c
    for e, (nc, sym) in zip(ev, caps):
        k = int(e["push"])
        assert int(e["found_at"]) == boundaries[k] and int(e["channel"]) == 0
        assert k < _first_boundary_with(nc, boundaries)                                # reported in an earlier push than its capture
        assert 0 < int(e["found_at"]) - nc < CUT + 128                                 # the delay bound, P = the push's samples
        if int(e["flags"]) & seizureref.DCC_COMPLETE:
            assert nc + 14 * SPS < boundaries[k]
            dcc, bad = refdecode.manchester(trackref.capture(g, nc, SPS, track=False)[:14], 7)
            assert list(e["dcc"]) == dcc and int(e["dcc_bad"]) == bad
        else:
            assert nc + 14 * SPS >= boundaries[k] and not e["dcc"].any() and int(e["dcc_bad"]) == 0
    # a finer cut finds them no later, and a boundary list that repeats itself adds nothing
    fine = seizureref.events(g, SPS, list(range(64, len(g) + 1, 64)))
    assert list(fine["position"]) == list(ev["position"]) and all(fine["found_at"] <= ev["found_at"])
    assert all(fine["found_at"] - fine["position"] < 64 + 128)


def test_both_values_of_dcc_complete_occur_on_a_fine_cut(stream):
    """at ten samples per symbol the 14 symbols behind n_c span 140 samples: cut every 64 samples, no event can have them all; cut so
    that a boundary lies 141 samples or more behind n_c and fewer than 64 behind its run's word, it does"""
    g, caps = stream
    fine = seizureref.events(g, SPS, list(range(64, len(g) + 1, 64)))
    assert len(fine) == 3 and not (fine["flags"] & seizureref.DCC_COMPLETE).any()
    coarse = seizureref.events(g, SPS, list(range(CUT, len(g) + 1, CUT)))
    assert (coarse["flags"] & seizureref.DCC_COMPLETE).any()


def test_the_comparison_the_gpu_tests_use_sees_every_field(stream):
    g, _ = stream
    want = seizureref.events(g, SPS, list(range(CUT, len(g) + 1, CUT)))
    got = np.zeros(len(want), capi.SEIZURE_DTYPE)
    for f in seizureref.FIELDS:
        got[f] = want[f]
    seizureref.assert_equal(got, want)
    seizureref.assert_equal(got[:0], want[:0])
    seizureref.assert_equal(got[:1], want[:1])
    for f in seizureref.FIELDS:
        off = got.copy()
        off[f][-1] = off[f][-1] + 1 if off[f][-1].ndim == 0 else off[f][-1] ^ [0, 0, 1, 0, 0, 0, 0]
        with pytest.raises(AssertionError):
            seizureref.assert_equal(off, want)
    with pytest.raises(AssertionError):
        seizureref.assert_equal(got[:-1], want)


def test_one_block_gives_no_event_for_a_capture_that_completes_in_it(stream):
    g, caps = stream
    ev = seizureref.events(g, SPS, [len(g)])
    assert len(ev) == 0
    # cut behind the second capture's trigger: the first capture is complete there (no event), the second pending (one event)
    cut = (caps[1][0] + 2000) // 64 * 64
    ev = seizureref.events(g, SPS, [cut, len(g)])
    assert [int(p) for p in ev["position"]] == [caps[1][0]] and int(ev[0]["push"]) == 0
