"""not gpu: the boundary of the early messages (include/amps_recc_early.h: AMPS_RECC_FLAG_EARLY_MESSAGES, amps_recc_early_t,
amps_recc_drain_early -- the flag, the 744-byte event, the export in a binding table of its own, the ABI version) and what the feature
rests on, on the CPU model's slicer bits: the capture's timing walk is causal, so the second statement's prefix walk over n words
(tests/earlyref.py) gives the first 14 + 480 n symbols and the first 1 + 5 n delays of the walk over the whole burst, whose symbols
are trackref.capture's; and the event's record carries, for its words, what the decode of the whole capture carries.  The coverage
conditions of tests/test_gpu_early_messages.py are shown to hold on the model here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import earlyref
import earlystream as es
import oracle
import refdecode
import seizureref
import trackref
from gr_amps_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name="amps_recc_early.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _code(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


# ------------------------------------------------------------------------------------------------------------------ the boundary
def test_the_header_has_the_flag_the_event_and_the_entry_point():
    hdr, base, seiz = _header(), _header("amps_recc.h"), _header("amps_recc_seizure.h")
    assert re.search(r"#define\s+AMPS_RECC_FLAG_EARLY_MESSAGES\s+0x4000u\b", hdr)
    assert re.search(r'#include\s+"amps_recc.h"', hdr) and re.search(r"#define\s+AMPS_RECC_ABI_VERSION\s+4\b", base)
    assert capi.FLAG_EARLY_MESSAGES == 0x4000
    # no flag of the three headers shares a bit with another, and this one is the one behind the seizure events'
    flags = {n: int(v, 16) for n, v in re.findall(r"#define\s+(AMPS_RECC_FLAG_\w+)\s+(0x[0-9a-fA-F]+)u", base + seiz + hdr)}
    assert [n for n, v in flags.items() if v & 0x4000] == ["AMPS_RECC_FLAG_EARLY_MESSAGES"]
    assert len(set(flags.values())) == len(flags) and sorted(flags.values())[-3:] == [0x1000, 0x2000, 0x4000]
    body = re.search(r"typedef struct amps_recc_early \{(.*?)\} amps_recc_early_t;", hdr, flags=re.S).group(1)
    fields = [" ".join(f.split()) for f in _code(body).split(";") if f.strip()]
    assert fields == ["amps_recc_burst_t rec", "uint64_t found_at", "uint32_t n_words", "uint32_t _pad"]
    assert re.search(r"#define\s+AMPS_RECC_EARLY_BYTES\s+744\b", hdr)


def test_the_event_is_744_bytes_and_the_statement_lays_it_out_as_the_binding_does():
    dt = capi.EARLY_DTYPE
    assert dt.itemsize == 744 == earlyref.EVENT_DTYPE.itemsize and capi.BURST_DTYPE.itemsize == 728
    assert [(n, dt.fields[n][1]) for n in dt.names] == [("rec", 0), ("found_at", 728), ("n_words", 736), ("_pad", 740)]
    assert dt.fields["rec"][0] == capi.BURST_DTYPE
    # the statement states the record's layout again: the same names at the same offsets with the same types
    ours, theirs = earlyref.RECORD_DTYPE, capi.BURST_DTYPE
    assert ours.names == theirs.names
    assert [(ours.fields[n][0], ours.fields[n][1]) for n in ours.names] == [(theirs.fields[n][0], theirs.fields[n][1]) for n in theirs.names]


def test_the_export_is_in_a_table_of_its_own_and_the_other_tables_stand():
    code = _code(_header())
    decls = re.findall(r"^[ \t]*([A-Za-z_][\w \t]*?[ \t\*]+)(amps_(?:recc|bch)_\w+)\s*\(([^;{]*?)\)\s*;", code, flags=re.M)
    assert [d[1] for d in decls] == list(capi.EARLY_PROTOTYPES) == list(capi.EARLY_EXPORTS) == ["amps_recc_drain_early"]
    assert set(re.findall(r"\b(amps_(?:recc|bch)_[a-z_0-9]+)\s*\(", code)) == set(capi.EARLY_EXPORTS)
    assert not set(capi.EARLY_EXPORTS) & (set(capi.EXPORTS) | set(capi.EXTENSION_EXPORTS))
    assert list(capi.EXTENSION_PROTOTYPES) == list(capi.EXTENSION_EXPORTS) == ["amps_recc_drain_seizures"]
    base = re.findall(r"^[ \t]*[A-Za-z_][\w \t]*?[ \t\*]+(amps_(?:recc|bch)_\w+)\s*\([^;{]*?\)\s*;", _code(_header("amps_recc.h")), flags=re.M)
    assert base == list(capi.EXPORTS)                                                   # the base header's entry points, as they were
    scalars = {"int": C.c_int, "size_t": C.c_size_t, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}
    for ret, name, params in decls:
        restype, argtypes = capi.EARLY_PROTOTYPES[name]
        params = [q.strip() for q in " ".join(params.split()).split(",")]
        assert ret.strip() == "int" and restype is C.c_int and len(params) == len(argtypes), (name, params)
        for q, t in zip(params, argtypes):
            if "*" in q:
                assert t is C.c_void_p or issubclass(t, C._Pointer), (name, q, t)
            else:
                assert t is scalars[q.replace("const", "").split()[0]], (name, q, t)
    L = capi.load()
    fn = L.amps_recc_drain_early
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    assert L.amps_recc_abi_version() == 4
    n = C.c_size_t(7)
    assert L.amps_recc_drain_early(None, None, 0, C.byref(n), None) == -22              # -EINVAL without a handle, no device touched


# ---------------------------------------------------------------------------------------------------------------- the causality
def _one_burst(sps, ppm, seed):
    """the model's slicer bits of one whole seven-word burst (random filler behind the message: every block has transitions to measure)"""
    rng = np.random.default_rng(seed)
    _, _, _, _, words = synth.random_message(rng)
    bits = synth.burst_bits(words, dcc=int(rng.integers(0, 4)), rng=rng)
    n = (1500 + 2 * sps * len(bits) + 1500) // 64 * 64
    iq = synth.fsk_modulate(n, [(1000, bits)], sps=sps, fs=20e3 * sps, snr_db=25.0, rng=rng, sym_ppm=float(ppm))
    f = oracle.Fused(0, sps)
    f.push(iq, cap=4)
    return f.taps()[2]


@pytest.mark.parametrize("ppm", [0, 100, -100, 500, -500])
@pytest.mark.parametrize("sps", [2, 3, 10])
def test_a_prefix_of_the_walk_is_the_prefix_of_the_capture(sps, ppm):
    """The walk over the first n words, on the bits in front of T(n) ALONE (an index behind them would raise), gives the first
    14 + 480 n symbols and the first 1 + 5 n delays of the walk over everything, whose symbols are trackref.capture's; and the event's
    record carries for its words what the decode of the whole capture carries."""
    g = _one_burst(sps, ppm, 900 + 10 * sps + ppm)
    caps = trackref.captures(g, sps)
    assert len(caps) == 1
    nc, whole = caps[0]
    moved = None
    for track in (True, False):
        whole = trackref.capture(g, nc, sps, track)
        sym, delays = earlyref.walk(g, nc, sps, track)
        assert len(delays) == 36 and np.array_equal(sym, whole)
        moved = len(set(delays)) > 1 if track else moved
        full = refdecode.decode(whole)
        for n in range(1, 8):
            T = earlyref.due(nc, sps, n, track)
            ps, pd = earlyref.walk(g[:T], nc, sps, track, 1 + 5 * n)
            assert np.array_equal(ps, whole[:14 + 480 * n]) and pd == delays[:1 + 5 * n], (n, track)
            if n == 7:
                assert T == nc + seizureref.span_done(sps, track)              # T(7) is the span a record waits for
                continue
            rec = earlyref.event_record(g[:T], nc, sps, n, track)
            want = earlyref.record_of(full, 0, nc)
            earlyref.assert_relation({"rec": rec, "n_words": n}, want)
    if abs(ppm) == 500:
        assert moved                                                                    # the tracked walk had something to follow


def test_majority_mode_holds_the_same_relation():
    g = _one_burst(10, 0, 31)
    (nc, whole), = trackref.captures(g, 10)
    full = earlyref.record_of(refdecode.decode_majority(whole), 0, nc)
    for n in (1, 2, 3, 6):
        T = earlyref.due(nc, 10, n)
        earlyref.assert_relation({"rec": earlyref.event_record(g[:T], nc, 10, n, True, True), "n_words": n}, full)


# ----------------------------------------------------------------------------------------------- the GPU cases' coverage, on the model
@pytest.fixture(scope="module")
def model_bits():
    def bits(ppm):
        iq = es.iq_stream(3, ppm)
        rows = []
        for c in range(3):
            f = oracle.Fused(c, es.SPS)
            f.push(iq[c], cap=8)
            rows.append(f.taps()[2])
        return np.stack(rows)
    return bits


def check_iq_coverage(pushes, ev, bits, bounds, rows=(0, 1, 2), track=True, majority=False):
    """what the IQ-seam cases of the GPU tests need of their stream, from the statement: one event each for the 2-, 3- and 4-word
    messages on their rows, in three different pushes, each at the first boundary behind T(n_words); the 7-word message's capture is
    accepted and has no event"""
    assert [int(x) for x in ev["rec"]["channel"]] == list(rows) and [int(x) for x in ev["n_words"]] == [2, 3, 4], (ev["rec"]["channel"], ev["n_words"])
    assert len(set(pushes.tolist())) == 3 and list(pushes) == sorted(pushes)
    for k, e in zip(pushes, ev):
        T = earlyref.due(int(e["rec"]["position"]), es.SPS, int(e["n_words"]), track)
        assert bounds[k] == int(e["found_at"]) and T < bounds[k] and not T < bounds[k - 1]
        assert int(e["rec"]["msg_class"]) == {2: refdecode.PAGE_RESPONSE, 3: refdecode.REGISTRATION, 4: refdecode.ORIGINATION}[int(e["n_words"])]
    caps = trackref.captures(bits[rows[0]], es.SPS, 0, track, bounds[-1])
    assert len(caps) == 2 and caps[0][0] == int(ev[0]["rec"]["position"])
    seven = earlyref.decode(caps[1][1], majority)
    assert seven["valid"][0] and seven["a"]["NAWC"] == 6                              # announced seven words: never an event


@pytest.mark.parametrize("ppm", [0, 500, -500])
def test_the_iq_stream_of_the_gpu_cases_has_what_they_need(model_bits, ppm):
    bits, bounds = model_bits(ppm), es.boundaries()
    assert bounds[-1] == es.N // 64 * 64 <= bits.shape[1]
    pushes, ev = earlyref.events(bits, es.SPS, bounds)
    check_iq_coverage(pushes, ev, bits, bounds)
    for e in ev:
        # stream time from the trigger to the event: 49, 73 or 97 ms of symbols and at most a push
        late = (int(e["found_at"]) - int(e["rec"]["position"])) / (20e3 * es.SPS)
        assert 0.024 * int(e["n_words"]) < late < 0.024 * int(e["n_words"]) + 0.002 + es.PUSH / (20e3 * es.SPS)
        if ppm:
            _, delays = earlyref.walk(bits[int(e["rec"]["channel"])], int(e["rec"]["position"]), es.SPS, True, 1 + 5 * int(e["n_words"]))
            assert len(set(delays)) > 1                                                 # the delays inside the prefix move
    # the records that follow: the relation, and the same words where the message is well formed
    for e in ev:
        c, p = int(e["rec"]["channel"]), int(e["rec"]["position"])
        R = earlyref.record_of(refdecode.decode(trackref.capture(bits[c], p, es.SPS)), c, p)
        earlyref.assert_relation(e, R)
        for f in ("msg_class", "min", "esn", "has_esn", "dialed", "n_called_words", "flags"):
            assert e["rec"][f] == R[f], (f, e["rec"][f], R[f])


def test_flag_cases_have_their_events_on_the_model(model_bits):
    bits, bounds = model_bits(0), es.boundaries()
    for track, majority in ((False, False), (True, True)):
        pushes, ev = earlyref.events(bits, es.SPS, bounds, track=track, majority=majority)
        check_iq_coverage(pushes, ev, bits, bounds, track=track, majority=majority)


def test_overflow_and_reset_cases_have_their_events_on_the_model(model_bits):
    """max_bursts = 2 keeps the first two of three; the reset of the GPU case falls between the first trigger and the first event"""
    bits, bounds = model_bits(0), es.boundaries()
    pushes, ev = earlyref.events(bits, es.SPS, bounds)
    assert len(ev) == 3 > 2
    first = next(k for k, n_k in enumerate(bounds) if seizureref.pending(seizureref.accepted(seizureref.matches(bits[0], es.SPS)[0], es.SPS), es.SPS, n_k) is not None)
    assert first < RESET_AFTER_PUSHES <= pushes[0]


RESET_AFTER_PUSHES = 4                                # pushes of the stream before the reset of the GPU case


def test_the_wideband_blocks_messages_announce_two_and_three_words():
    """the eight bursts of tests/test_gpu_wideband_second_statement.py's block (a), replayed from its generator without the waveforms:
    the mobiles at 30 and 20 dB send two page responses (2 words) and the one at 30 dB a registration (3); their starts lie 7.5 ms
    apart, so their events cannot all fall into one 20 ms push.  (What the device's bits give is computed from the statement there.)"""
    rng = np.random.default_rng(101)
    kinds = []
    for _ in range(8):
        _, _, _, _, words = synth.random_message(rng)
        synth.burst_bits(words, dcc=int(rng.integers(0, 4)), rng=rng)
        rng.uniform(0, 2 * np.pi)
        kinds.append(len(words))
    cn = [30, 20, 14, 12, 30, 10, 25, 16]
    strong = [k for k, c in zip(kinds, cn) if c >= 20]
    assert strong.count(2) >= 2 and 3 in strong, kinds
    starts_ms = [(60000 + 230017 * i) / 30.72e3 for i in range(8)]
    due_ms = [s + 24.0 * k for s, k in zip(starts_ms, kinds)]
    assert max(due_ms[i] for i in (0, 1, 4)) - min(due_ms[i] for i in (0, 1, 4)) > 20.0


def test_the_comparison_the_gpu_tests_use_sees_every_byte(model_bits):
    bits, bounds = model_bits(0), es.boundaries()
    _, want = earlyref.events(bits, es.SPS, bounds)
    got = np.frombuffer(want.tobytes(), capi.EARLY_DTYPE).copy()
    earlyref.assert_equal(got, want)
    earlyref.assert_equal(got[:0], want[:0])
    for off in (0, 8, 23, 40, 60, 120, 500, 700, 728, 736):                             # a byte of the record, of found_at, of n_words
        raw = bytearray(want.tobytes())
        raw[744 + off] ^= 1
        with pytest.raises(AssertionError):
            earlyref.assert_equal(np.frombuffer(bytes(raw), capi.EARLY_DTYPE), want)
    with pytest.raises(AssertionError):
        earlyref.assert_equal(got[:-1], want)
