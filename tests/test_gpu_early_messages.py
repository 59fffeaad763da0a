"""-m gpu: early messages (AMPS_RECC_FLAG_EARLY_MESSAGES, amps_recc_drain_early) on every data seam, held to their second statement
(tests/earlyref.py) on the DEVICE'S OWN slicer bits (Recc.debug_slicer_bits) and the push boundaries the device reports.  Everything
behind the slicer is integer logic on those bits, so every comparison is exact: every byte of every event, push by push.  Each event's
record follows in a later push with the relation the header promises, and the records are byte-identical to those of a handle without
the flag.  The coverage conditions of each case are computed from the statement on those bits (tests/test_cpu_early_messages.py shows
them on the CPU model).  Inputs are synthesised once per process; the wideband blocks are those of
tests/test_gpu_wideband_second_statement.py and share its cache."""
import errno
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import bitsref
import earlyref
import earlystream as es
import grid10block as gb
import narrowblock as nb
import narrowstream as ns
import seizureref
from gr_amps_amd import capi, synth
from gr_amps_amd.host import build_host
from test_cpu_early_messages import RESET_AFTER_PUSHES, check_iq_coverage
from test_gpu_wideband_second_statement import A_ROWS, A_SAMPLES, _block_a, _handle, _silence

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _produced(r):
    return r.debug_slicer_bits(0, 0)[1]


def _feed(r, parts, push, early=True, records=True, seizures=False):
    """push every part; after each one drain the early messages and the records and read what the slicer has produced"""
    ev, recs, sz, bounds = [], [], [], []
    for part in parts:
        push(part)
        if seizures:
            sz.append(r.drain_seizures())
        if early:
            ev.append(r.drain_early())
        if records:
            recs.append(r.drain())
        bounds.append(_produced(r))
    return (ev, recs, bounds, sz) if seizures else (ev, recs, bounds)


def _check_events(r, ev, bounds, sps, track=True, majority=False, tol=0):
    """the events drained after each push are the statement's for that push, every byte; returns the statement's (pushes, events)"""
    bits, n_done = r.debug_slicer_bits(0, bounds[-1])
    assert n_done == bounds[-1]
    pushes, want = earlyref.events(bits, sps, bounds, tol, track, majority)
    for k, got in enumerate(ev):
        assert got.dtype == capi.EARLY_DTYPE
        earlyref.assert_equal(got, want[pushes == k], "push %d" % k)
    return pushes, want, bits


def _assert_records_follow(ev, recs):
    """every event is followed by exactly one record with its (channel, position), in a strictly later push, with the header's relation;
    where the record's parse read no word behind the event's, the parsed fields and the reply words are the record's"""
    where = {}
    for k, rr in enumerate(recs):
        for x in rr:
            key = (int(x["channel"]), int(x["position"]))
            assert key not in where
            where[key] = (k, x)
    n = same_reply = 0
    for k, ee in enumerate(ev):
        for e in ee:
            key = (int(e["rec"]["channel"]), int(e["rec"]["position"]))
            assert key in where and where[key][0] > k, (key, k)
            R = where[key][1]
            earlyref.assert_relation(e, R)
            if 2 + int(R["has_esn"]) + int(R["n_called_words"]) <= int(e["n_words"]):   # R's parse read no word behind the event's
                for f in ("flags", "msg_class", "min", "esn", "has_esn", "dialed", "n_called_words") + tuple(n_ for n_ in capi.BURST_DTYPE.names if n_.startswith("b_")):
                    assert np.array_equal(e["rec"][f], R[f]), (key, f)
                assert bytes(capi.reply_words(e["rec"])) == bytes(capi.reply_words(R))
                same_reply += 1
            n += 1
    return n, same_reply


def _same(a, b):
    return [x.tobytes() for x in a] == [x.tobytes() for x in b]


# ------------------------------------------------------------------------------------------------------------- 1. the IQ seam, sps 10
def _iq_case(nch, ppm=0.0, **flags):
    iq = es.iq_stream(nch, ppm)
    parts = es.parts(iq)
    with capi.Recc(n_channels=nch, sps=es.SPS, max_samples=iq.shape[1], max_bursts=16, early_messages=True, **flags) as r:
        ev, recs, bounds = _feed(r, parts, r.push_iq)
        pushes, want, bits = _check_events(r, ev, bounds, es.SPS, track=not flags.get("fixed_timing", False), majority=flags.get("majority", False))
        assert len(r.drain_early()) == 0
    with capi.Recc(n_channels=nch, sps=es.SPS, max_samples=iq.shape[1], max_bursts=16, **flags) as r:
        _, plain, bounds_off = _feed(r, parts, r.push_iq, early=False)
    assert bounds == es.boundaries() == bounds_off
    assert _same(recs, plain)                                                           # records byte-identical to a handle without the flag
    check_iq_coverage(pushes, want, bits, bounds, es.live_rows(nch), track=not flags.get("fixed_timing", False), majority=flags.get("majority", False))
    followed, same_reply = _assert_records_follow(ev, recs)
    assert followed == 3 == same_reply
    assert sum(len(a) for a in recs) == 4                                               # the 7-word message has a record and no event
    return pushes, want, bits


@pytest.mark.parametrize("nch", [3, 64], ids=["C3-queue", "C64-resolve"])
def test_iq_seam_messages_of_two_three_four_and_seven_words(gpu, nch):
    """a page response, a registration, an origination with seven digits and a 7-word message whose carriers end behind their last
    word, in pushes of 2000 samples: three events, each the statement's, each followed by its record; none for the 7-word message"""
    t0 = time.perf_counter()
    pushes, want, _ = _iq_case(nch)
    late = [(int(e["found_at"]) - int(e["rec"]["position"])) / 200.0 for e in want]
    print(f"\n(1) C={nch}: events in pushes {pushes.tolist()}, {late} ms behind their triggers; {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("ppm", [500, -500])
def test_iq_seam_with_a_clock_offset(gpu, ppm):
    """the same four messages from mobiles whose bit clock is 500 ppm off: the delays inside the prefix move (asserted from the
    statement), and the events are still the statement's"""
    _, want, bits = _iq_case(3, float(ppm))
    for e in want:
        _, delays = earlyref.walk(bits[int(e["rec"]["channel"])], int(e["rec"]["position"]), es.SPS, True, 1 + 5 * int(e["n_words"]))
        assert len(set(delays)) > 1, delays


@pytest.mark.parametrize("flags", [dict(majority=True), dict(fixed_timing=True)], ids=["majority", "fixed"])
def test_iq_seam_under_the_decode_and_timing_flags(gpu, flags):
    _iq_case(3, **flags)


def test_both_flags_on_an_early_message_never_precedes_its_seizure_event(gpu):
    iq = es.iq_stream(3)
    with capi.Recc(n_channels=3, sps=es.SPS, max_samples=iq.shape[1], max_bursts=16, early_messages=True, seizure_events=True) as r:
        ev, recs, bounds, sz = _feed(r, es.parts(iq), r.push_iq, seizures=True)
        _check_events(r, ev, bounds, es.SPS)
        bits, _ = r.debug_slicer_bits(0, bounds[-1])
        want_sz = seizureref.events(bits, es.SPS, bounds)
        for k, got in enumerate(sz):
            seizureref.assert_equal(got, want_sz[want_sz["push"] == k], "push %d" % k)
    seized = {(int(s["channel"]), int(s["position"])): k for k, ss in enumerate(sz) for s in ss}
    n = 0
    for k, ee in enumerate(ev):
        for e in ee:
            assert seized[(int(e["rec"]["channel"]), int(e["rec"]["position"]))] <= k
            n += 1
    assert n == 3 and len(seized) == 4


# ---------------------------------------------------------------------------------------------------- 2. the 1024 bank, 20 ms blocks
def test_wideband_bank_in_realtime_blocks(gpu, decim):
    """the eight impaired bursts of the second-statement test in 10 000 x 768 samples, pushed in 20 ms blocks plus silence: the events of
    all 832 rows are the statement's, each one's record arrives in a later push with the relation, and the records are byte-identical
    to those of a handle without the flag"""
    import torch
    t0 = time.perf_counter()
    D, sps = decim, 1536 // decim
    x, _ = _block_a(torch, gpu)
    quiet = _silence(torch, gpu, 64, D)
    parts = [x[o:o + bitsref.REALTIME_SAMPLES] for o in range(0, A_SAMPLES, bitsref.REALTIME_SAMPLES)] + [quiet]
    with _handle(D, A_SAMPLES // D + 64, early_messages=True) as r:
        ev, recs, bounds = _feed(r, parts, r.push_wideband)
        pushes, want, _ = _check_events(r, ev, bounds, sps)
        assert len(r.drain_early()) == 0
    with _handle(D, A_SAMPLES // D + 64) as r:
        _, plain, bounds_off = _feed(r, parts, r.push_wideband, early=False)
    assert bounds_off == bounds and _same(recs, plain)
    words = sorted(int(w) for w in want["n_words"])
    print(f"\n(2) D={D}: {len(want)} events of {words} words in pushes {sorted(set(pushes.tolist()))}; {time.perf_counter() - t0:.2f} s")
    assert 2 in words and 3 in words and len(set(pushes.tolist())) > 1                  # coverage, from the statement
    assert set(int(c) for c in want["rec"]["channel"]) <= set(A_ROWS)
    followed, _ = _assert_records_follow(ev, recs)
    assert followed == len(want)


# ---------------------------------------------------------------------------------------------------------------- 3. the other seams
def _bank_case(r, parts, sps, planted_rows):
    ev, recs, bounds = _feed(r, parts, r.push_wideband)
    pushes, want, _ = _check_events(r, ev, bounds, sps)
    assert len(want) >= 1 and set(int(c) for c in want["rec"]["channel"]) <= set(planted_rows)
    followed, _ = _assert_records_follow(ev, recs)
    assert followed == len(want)
    return pushes, want


def test_a_128_branch_bank(gpu):
    """the narrow bank's burst block (six bursts) at M = 128, D = 96, in 20 ms blocks and a flush"""
    M, D = 128, 96
    x = nb.burst_block(M, D)[0]
    block = 800 * D
    parts = [x[o:o + block] for o in range(0, len(x), block)] + [ns.flush(D)]
    with ns.handle(M, D, (len(x) + 64 * D) // D + 72, early_messages=True) as r:
        _bank_case(r, parts, nb.sps_of(M, D), {k for k, _ in nb.planted(M)})


def test_a_500_branch_bank_of_10_khz_bins(gpu):
    """the 10 kHz grid's burst block (six bursts) at M = 500, in 20 ms blocks and a flush"""
    M = 500
    D, Cg = gb.decim(M), gb.max_channels(M)
    x = gb.burst_block(M)[0]
    block = 800 * D
    parts = [x[o:o + block] for o in range(0, len(x), block)] + [np.zeros(64 * D, np.complex64)]
    with capi.Recc(n_channels=Cg, max_samples=(len(x) + 64 * D) // D + 72, max_bursts=64, early_messages=True,
                   wideband={"channels": M, "decim": D, "first_channel": gb.FIRST}) as r:
        _bank_case(r, parts, gb.SPS, {row for row, _ in gb.planted(M)})


def test_shared_translate_seam(gpu):
    """three centres of an 800 ksps stream, decimated by 4, in blocks of 16 384 samples"""
    from test_gpu_seizure_events import _stream800
    x, centres, fs = _stream800()
    parts = [x[o:o + 16384] for o in range(0, x.size, 16384)]
    with capi.Recc(n_channels=3, sps=10, max_samples=x.size // 4, max_bursts=16, early_messages=True) as r:
        r.set_xlate_shared(fs, centres, 4)
        ev, recs, bounds = _feed(r, parts, r.push_raw_shared)
        pushes, want, _ = _check_events(r, ev, bounds, 10)
    assert len(want) >= 1
    followed, _ = _assert_records_follow(ev, recs)
    assert followed == len(want)


# ------------------------------------------------------------------------------------------------------------------ 4. list behaviour
def test_overflow_keeps_the_first_two_and_says_so_once(gpu):
    iq = es.iq_stream(3)
    with capi.Recc(n_channels=3, sps=es.SPS, max_samples=iq.shape[1], max_bursts=2, early_messages=True) as r:
        _, recs, bounds = _feed(r, es.parts(iq), r.push_iq, early=False)
        bits, _ = r.debug_slicer_bits(0, bounds[-1])
        _, want = earlyref.events(bits, es.SPS, bounds)
        assert len(want) == 3
        with pytest.raises(capi.AmpsError) as e:
            r.drain_early()
        assert e.value.code == -errno.ENOSPC
        earlyref.assert_equal(e.value.early, want[:2], "what the overflow keeps")
        assert len(r.drain_early()) == 0                                                 # and no error: the overflow was reported once


def test_a_partial_drain_leaves_the_rest(gpu):
    L = capi.load()
    iq = es.iq_stream(3)
    with capi.Recc(n_channels=3, sps=es.SPS, max_samples=iq.shape[1], max_bursts=16, early_messages=True) as r:
        _, _, bounds = _feed(r, es.parts(iq), r.push_iq, early=False, records=False)
        bits, _ = r.debug_slicer_bits(0, bounds[-1])
        _, want = earlyref.events(bits, es.SPS, bounds)
        assert len(want) == 3
        out = np.zeros(1, capi.EARLY_DTYPE)
        nout, nleft = capi.C.c_size_t(0), capi.C.c_size_t(0)
        assert L.amps_recc_drain_early(r._h, capi._hostptr(out), 1, capi.C.byref(nout), capi.C.byref(nleft)) == 0
        assert (nout.value, nleft.value) == (1, 2)
        earlyref.assert_equal(out, want[:1])
        r.drain_begin()                                                                  # independent of an open split drain
        earlyref.assert_equal(r.drain_early(), want[1:])
        r.drain_end()
        assert L.amps_recc_drain_early(r._h, None, 3, capi.C.byref(nout), None) == -errno.EINVAL
        assert L.amps_recc_drain_early(r._h, capi._hostptr(out), 1, None, None) == -errno.EINVAL
        assert L.amps_recc_drain_early(r._h, None, 0, capi.C.byref(nout), None) == 0 and nout.value == 0


def test_a_reset_between_trigger_and_event_empties_the_list(gpu):
    iq = es.iq_stream(3)
    parts = es.parts(iq)
    with capi.Recc(n_channels=3, sps=es.SPS, max_samples=iq.shape[1], max_bursts=16, early_messages=True) as r:
        ev0, _, _ = _feed(r, parts[:RESET_AFTER_PUSHES], r.push_iq, records=False)      # the first trigger is pending, its message not in
        assert sum(len(a) for a in ev0) == 0
        r.reset()
        assert len(r.drain_early()) == 0
        ev, _, bounds = _feed(r, parts[RESET_AFTER_PUSHES:RESET_AFTER_PUSHES + 4], r.push_iq, records=False)
        assert sum(len(a) for a in ev) == 0                                             # the capture was forgotten with the stream
        r.reset()
        ev, recs, bounds = _feed(r, parts, r.push_iq)                                   # the whole stream again: the statement's events
        pushes, want, _ = _check_events(r, ev, bounds, es.SPS)
        assert len(want) == 3
        r.reset()
        _feed(r, parts[:pushes[0] + 1], r.push_iq, early=False, records=False)
        r.reset()                                                                        # with one undrained event
        assert len(r.drain_early()) == 0


def test_a_handle_without_the_flag_answers_enosys(gpu):
    with capi.Recc(n_channels=2, sps=10, max_samples=4096, max_bursts=4) as r:
        with pytest.raises(capi.AmpsError) as e:
            r.drain_early()
        assert e.value.code == -errno.ENOSYS
    with pytest.raises(capi.AmpsError) as e:                                             # the symbol seam alone has no capture coming in
        capi.Recc(n_channels=1, max_bursts=4, early_messages=True)
    assert e.value.code == -errno.EINVAL


# -------------------------------------------------------------------------------------------------------------------------- 5. tools
FS, CENTRES, CHUNK = 400e3, (-60e3, 90e3), 16384


def _one_burst_file():
    """a page response on the second centre of a 400 ksps stream, its carrier ending behind its last word"""
    n, sps = 120000, 20
    rng = np.random.default_rng(8200)
    bits = synth.burst_bits(synth.make_message("page_response", "2065550123"), dcc=2, pad_words=False)
    iq = synth.fsk_modulate(n, [(9000, bits)], sps=sps, fs=20e3 * sps, snr_db=30.0, rng=rng)
    return (iq * np.exp(2j * np.pi * CENTRES[1] * np.arange(n) / FS)).astype(np.complex64)


def test_the_tools_print_the_bindings_events(gpu, tmp_path):
    x = _one_burst_file()
    p = tmp_path / "one.raw"
    x.tofile(p)
    with capi.Recc(n_channels=2, sps=10, max_samples=x.size // 2, max_bursts=16, early_messages=True) as r:
        r.set_xlate_shared(FS, CENTRES, 2)
        ev, recs = [], []
        for o in range(0, x.size, CHUNK):
            r.push_raw_shared(x[o:o + CHUNK])
            ev.append(r.drain_early())
            recs.append(r.drain())
    ev, recs = np.concatenate(ev), np.concatenate(recs)
    assert len(ev) == 1 and len(recs) == 1 and int(ev[0]["n_words"]) == 2
    e = ev[0]
    want = "MSG early channel 1 position %d found_at %d words 2 class %d min %s" % (
        int(e["rec"]["position"]), int(e["found_at"]), int(e["rec"]["msg_class"]), e["rec"]["min"].decode())
    _, exe = build_host()
    args = [exe, "sub", str(p), str(CHUNK), "%g" % FS, "2", ",".join("%g" % c for c in CENTRES)]
    out = subprocess.run(args + ["early"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [l for l in out.stdout.splitlines() if l.startswith("MSG ")]
    assert [l for l in lines if l.startswith("MSG early")] == [want]
    assert lines.index(want) < lines.index("MSG channel 1")                              # the early message in front of the record's lines
    plain = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0, plain.stderr
    assert [l for l in plain.stdout.splitlines() if l.startswith("MSG ")] == [l for l in lines if l != want]


def test_the_example_prints_per_mobile_the_time_to_the_message_and_to_the_record(gpu):
    """examples/decode_subband.py --early: 21 mobiles, 2 ms blocks.  Every early message it prints is one of the records it prints (same
    channel, same MIN), came 24 ms per announced word (+ 15 symbols and the tracking margin) and at most a block behind its trigger, and
    its record 169 ms and at most a block"""
    ex = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "decode_subband.py"), "--early"], capture_output=True, text=True, timeout=300)
    assert ex.returncode == 0, ex.stdout + ex.stderr
    recs = {int(m.group(1)): m.group(2) for m in re.finditer(r"^  channel +(\d+) \(AMPS \d+, [\d.]+ MHz\)  MIN (\d+)  class \d+  words valid \d+  ok$", ex.stdout, flags=re.M)}
    lines = re.findall(r"^  channel +(\d+)  position +(\d+)  words (\d)  MIN (\d+)  message after +([\d.]+) ms, record after +([\d.]+) ms  ok$", ex.stdout, flags=re.M)
    assert len(recs) == 21 and len(lines) >= 10 and "early messages: %d," % len(lines) in ex.stdout
    fs, block = 200e3, 400 + 64                                                          # channel rate; channel-rate samples of a 2 ms block, and a ring word
    for ch, pos, n, min10, t_msg, t_rec in lines:
        assert recs[int(ch)] == min10
        due = earlyref.due(0, 10, int(n)) / fs * 1e3
        assert due - 0.006 < float(t_msg) <= due + block / fs * 1e3 + 0.006, (ch, n, t_msg)
        done = seizureref.span_done(10) / fs * 1e3
        assert done - 0.006 < float(t_rec) <= done + block / fs * 1e3 + 0.006, (ch, t_rec)
    assert len({n for _, _, n, _, _, _ in lines}) >= 2                                   # messages of different lengths
