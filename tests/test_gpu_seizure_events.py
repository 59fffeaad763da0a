"""-m gpu: seizure events (AMPS_RECC_FLAG_SEIZURE_EVENTS, amps_recc_drain_seizures) on every data seam, held to their second statement
(tests/seizureref.py) on the DEVICE'S OWN slicer bits (Recc.debug_slicer_bits) and the push boundaries the device reports.  Everything
behind the slicer is integer logic on those bits, so every comparison is exact, every field of every event, push by push.  The
coverage conditions of each case (events in more than one push, both values of DCC_COMPLETE) are computed from the statement on those
bits, not assumed from the synthesis.  Inputs are synthesised once per process; the wideband blocks are those of
tests/test_gpu_wideband_second_statement.py and share its cache."""
import errno
import functools
import time

import numpy as np
import pytest

import bitsref
import narrowblock as nb
import narrowstream as ns
import seizureref
from gr_amps_amd import capi, synth
from test_gpu_wideband_second_statement import A_ROWS, A_SAMPLES, B_CUT, B_FRAMES, B_ROWS, C, _block_a, _block_b, _handle, _silence

pytestmark = pytest.mark.gpu
COMPLETE = capi.SEIZURE_FLAG_DCC_COMPLETE


def _produced(r):
    return r.debug_slicer_bits(0, 0)[1]


def _feed(r, parts, push, seizures=True, records=True):
    """push every part; after each one drain the events and the records and read what the slicer has produced: (events per push,
    records per push, boundaries)"""
    ev, recs, bounds = [], [], []
    for part in parts:
        push(part)
        if seizures:
            ev.append(r.drain_seizures())
        if records:
            recs.append(r.drain())
        bounds.append(_produced(r))
    return ev, recs, bounds


def _check_events(r, ev, bounds, sps, track=True, tol=0):
    """the events drained after each push are the statement's for that push, every field; returns the statement's events"""
    bits, n_done = r.debug_slicer_bits(0, bounds[-1])
    assert n_done == bounds[-1]
    want = seizureref.events(bits, sps, bounds, tol, track)
    for k, got in enumerate(ev):
        assert got.dtype == capi.SEIZURE_DTYPE
        seizureref.assert_equal(got, want[want["push"] == k], "push %d" % k)
    return want


def _assert_records_follow(ev, recs):
    """every event is followed by exactly one record with its (channel, position), in a strictly later push"""
    where = {}
    for k, rr in enumerate(recs):
        for x in rr:
            key = (int(x["channel"]), int(x["position"]))
            assert key not in where
            where[key] = k
    n = 0
    for k, ee in enumerate(ev):
        for e in ee:
            key = (int(e["channel"]), int(e["position"]))
            assert key in where and where[key] > k, (key, k, where.get(key))
            n += 1
    return n


def _delay_bound(want, bounds):
    """found_at - position < P + 128, P the samples the reporting push processed"""
    prev = [0] + list(bounds[:-1])
    for e in want:
        k = int(e["push"])
        assert 0 < int(e["found_at"]) - int(e["position"]) < bounds[k] - prev[k] + 128, e


# ----------------------------------------------------------------------------------------------------- 1. the 1024 bank, 20 ms blocks
def test_wideband_bank_in_realtime_blocks(gpu, decim):
    """the eight impaired bursts of the second-statement test in 10 000 x 768 samples, pushed in 20 ms blocks plus silence, events and
    records drained after every push: the events of all 832 rows are the statement's, each one's record arrives in a later push, and
    the records are byte-identical to those of a handle without the flag"""
    import torch
    t0 = time.perf_counter()
    D, sps = decim, 1536 // decim
    x, _ = _block_a(torch, gpu)
    quiet = _silence(torch, gpu, 64, D)
    parts = [x[o:o + bitsref.REALTIME_SAMPLES] for o in range(0, A_SAMPLES, bitsref.REALTIME_SAMPLES)] + [quiet]
    with _handle(D, A_SAMPLES // D + 64, seizure_events=True) as r:
        ev, recs, bounds = _feed(r, parts, r.push_wideband)
        want = _check_events(r, ev, bounds, sps)
        assert len(r.drain_seizures()) == 0
    with _handle(D, A_SAMPLES // D + 64) as r:
        _, plain, bounds_off = _feed(r, parts, r.push_wideband, seizures=False)
    assert bounds_off == bounds
    assert [a.tobytes() for a in recs] == [b.tobytes() for b in plain]
    assert len(want) >= 8 and set(A_ROWS) <= {int(c) for c in want["channel"]}
    followed = _assert_records_follow(ev, recs)
    _delay_bound(want, bounds)
    print(f"\n(1) D={D}: {len(want)} events in pushes {sorted(set(want['push'].tolist()))}, {followed} followed by their record, "
          f"{sum(len(a) for a in recs)} records identical without the flag; {time.perf_counter() - t0:.2f} s")
    assert followed == len(want)


# ------------------------------------------------------------------------------------------------------------- 2. the push-edge sweep
B_SHORT = 4096                                                 # frames of the second push in its short form: fewer than a burst's at either decimation


@pytest.mark.parametrize("second", ["short", "whole"])
def test_wideband_run_starts_swept_across_a_push_edge(gpu, decim, second):
    """the 192-row preamble sweep across the cut at frame 512: two pushes, then silence; events exact per push.  short: the second push
    is 4096 frames, fewer than a capture at either decimation, so every sweep row has an event, some found in the first push and some
    in the second.  whole: the second push is the rest of the block, 9488 frames -- at two samples per symbol more than a capture
    (6786), so the rows whose trigger it finds have no event, their record is there at once; at three (10 161) they have one."""
    import torch
    t0 = time.perf_counter()
    D, sps = decim, 1536 // decim
    x = _block_b(torch, gpu, D)
    F = B_CUT
    end = B_FRAMES if second == "whole" else F + B_SHORT
    quiet = max(64, -(-(F + 64 + bitsref.tail_frames(sps) + 64 - end) // 64) * 64)
    parts = (x[:F * D], x[F * D:end * D], _silence(torch, gpu, quiet, D))
    with _handle(D, B_FRAMES + quiet, seizure_events=True) as r:
        ev, recs, bounds = _feed(r, parts, r.push_wideband)
        want = _check_events(r, ev, bounds, sps)
    assert bounds[0] == F and bounds[1] == end // 64 * 64
    sweep = want[np.isin(want["channel"], B_ROWS)]
    per_push = [int((sweep["push"] == k).sum()) for k in range(3)]
    silent = sorted(set(B_ROWS) - set(sweep["channel"].tolist()))
    print(f"\n(2) D={D} {second}: {len(want)} events, of the sweep rows {per_push} per push, {len(silent)} rows without one; "
          f"{time.perf_counter() - t0:.2f} s")
    assert len(set(sweep["channel"].tolist())) == len(sweep) and per_push[0] > 0 and per_push[2] == 0
    if second == "short" or sps * (seizureref.CAPTURE_SYMS + 1) + seizureref.TRACK_BLOCKS >= bounds[1] - bounds[0]:
        assert not silent and per_push[1] > 0                  # some found in the first push and some in the second
    else:
        # found and completed in the second push: no event, and the record in that very push
        assert silent and per_push[1] == 0
        assert set(silent) <= {int(c) for c in recs[1]["channel"]}
    _delay_bound(want, bounds)
    assert _assert_records_follow(ev, recs) == len(want)
    assert sorted(set(int(c) for rr in recs for c in rr["channel"]) & set(B_ROWS)) == sorted(B_ROWS)


# --------------------------------------------------------------------------------------------------------------- 3. the IQ seam, sps 10
IQ_SPS, IQ_BLOCK, IQ_EDGE = 10, 4096, 2 * 4096


@functools.lru_cache(maxsize=None)
def _iq_stream(nch, step, first_nc, second=False):
    """complex64 [nch][n]: one whole burst per channel (two with `second`, the second one 200 symbols behind the first one's hold-off),
    the n_c of channel i aimed at first_nc + step i (a burst's 41 preamble bits end at its n_c: bitsref.iq_sustained_stream)"""
    rng = np.random.default_rng(1000 + nch)
    hold = IQ_SPS * bitsref.HOLD_SYMBOLS
    n = -(-(first_nc + step * nch + (2 if second else 1) * (hold + 200 * IQ_SPS) + 2000) // IQ_BLOCK) * IQ_BLOCK
    rows = []
    for i in range(nch):
        plan = []
        for k in range(2 if second else 1):
            _, _, _, _, words = synth.random_message(rng)
            nc = first_nc + step * i + k * (hold + 200 * IQ_SPS)
            plan.append((nc - 82 * IQ_SPS + 1, synth.burst_bits(words, dcc=int(rng.integers(0, 4)), rng=rng)))
        rows.append(synth.fsk_modulate(n, plan, sps=IQ_SPS, fs=20e3 * IQ_SPS, snr_db=30.0, rng=rng))
    iq = np.stack(rows)
    iq.setflags(write=False)
    return iq


def _iq_parts(iq):
    return [np.ascontiguousarray(iq[:, o:o + IQ_BLOCK]) for o in range(0, iq.shape[1], IQ_BLOCK)]


@pytest.mark.parametrize("fixed", [False, True], ids=["tracked", "fixed"])
@pytest.mark.parametrize("nch,step,first", [(8, 24, IQ_EDGE - 200), (64, 8, IQ_EDGE - 300)], ids=["C8-queue", "C64-resolve"])
def test_iq_seam_events_straddle_a_push_edge(gpu, nch, step, first, fixed):
    """one burst per channel whose n_c climb across the push edge at 8192, blocks of 4096: the channels whose n_c lie 140 samples or
    more in front of the edge have their DCC at once, those inside [edge - 140, edge - 64) are reported without it, the rest one push
    later.  With fixed timing a complete event's DCC is its record's."""
    t0 = time.perf_counter()
    iq = _iq_stream(nch, step, first)
    with capi.Recc(n_channels=nch, sps=IQ_SPS, max_samples=iq.shape[1], max_bursts=2 * nch, seizure_events=True, fixed_timing=fixed) as r:
        ev, recs, bounds = _feed(r, _iq_parts(iq), r.push_iq)
        want = _check_events(r, ev, bounds, IQ_SPS, track=not fixed)
    assert bounds == list(range(IQ_BLOCK, iq.shape[1] + 1, IQ_BLOCK))
    assert len(want) == nch and len(set(want["push"].tolist())) >= 2                     # events in at least two different pushes
    flags = set((want["flags"] & COMPLETE).tolist())
    assert flags == {0, COMPLETE}                                                        # both values of DCC_COMPLETE occur
    _delay_bound(want, bounds)
    assert _assert_records_follow(ev, recs) == nch
    allrecs = np.concatenate(recs)
    by_key = {(int(x["channel"]), int(x["position"])): x for x in allrecs}
    same = 0
    for e in np.concatenate(ev):
        rec = by_key[(int(e["channel"]), int(e["position"]))]
        if int(e["flags"]) & COMPLETE and fixed:
            assert e["dcc"].tolist() == rec["dcc"].tolist() and int(e["dcc_bad"]) == int(rec["dcc_bad"]), (e, rec["dcc"], rec["dcc_bad"])
            same += 1
    print(f"\n(3) C={nch} fixed={fixed}: {len(want)} events in pushes {sorted(set(want['push'].tolist()))}, "
          f"{int((want['flags'] & COMPLETE != 0).sum())} with their DCC ({same} compared with the record's); {time.perf_counter() - t0:.2f} s")
    assert not fixed or same > 0


# ---------------------------------------------------------------------------------------------------------------- 4. the other seams
@functools.lru_cache(maxsize=None)
def _stream800():
    """three mobiles' channels in one 800 ksps stream, one burst each"""
    n, fs = 200000, 800e3
    centres = (-90e3, 30e3, 150e3)
    k = np.arange(n)
    x = np.zeros(n, np.complex128)
    for c, fc in enumerate(centres):
        iq, _ = synth.make_channel_block(n, 1, seed=6100 + c, sps=40, first=6000 + 7001 * c)
        x += iq * np.exp(2j * np.pi * fc * k / fs)
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x, centres, fs


def test_shared_translate_seam(gpu):
    """three centres of an 800 ksps stream, decimated by 4, in blocks of 16 384 samples"""
    x, centres, fs = _stream800()
    parts = [x[o:o + 16384] for o in range(0, x.size, 16384)]
    with capi.Recc(n_channels=3, sps=10, max_samples=x.size // 4, max_bursts=16, seizure_events=True) as r:
        r.set_xlate_shared(fs, centres, 4)
        ev, recs, bounds = _feed(r, parts, r.push_raw_shared)
        want = _check_events(r, ev, bounds, 10)
    assert len(want) == 3 and sorted(want["channel"].tolist()) == [0, 1, 2]
    _delay_bound(want, bounds)
    assert _assert_records_follow(ev, recs) == 3


def test_a_128_branch_bank(gpu):
    """the narrow bank's burst block (six bursts) at M = 128, D = 96, in 20 ms blocks and a flush"""
    M, D = 128, 96
    x = nb.burst_block(M, D)[0]
    block = 800 * D
    parts = [x[o:o + block] for o in range(0, len(x), block)] + [ns.flush(D)]
    with ns.handle(M, D, (len(x) + 64 * D) // D + 72, seizure_events=True) as r:
        ev, recs, bounds = _feed(r, parts, r.push_wideband)
        want = _check_events(r, ev, bounds, nb.sps_of(M, D))
    assert len(want) >= 6 and {k for k, _ in nb.planted(M)} <= set(want["channel"].tolist())
    _delay_bound(want, bounds)
    assert _assert_records_follow(ev, recs) == len(want)


# ------------------------------------------------------------------------------------------------------------------------ 5. overflow
def test_overflow_keeps_the_first_events_in_order(gpu):
    """C = 8, max_bursts = 8, two bursts per channel: sixteen events, never drained while the records are drained every push.  The first
    drain_seizures delivers the first eight in (found_at, channel) order and answers -ENOSPC; the next one is empty and answers 0."""
    iq = _iq_stream(8, 24, IQ_EDGE - 200, second=True)
    with capi.Recc(n_channels=8, sps=IQ_SPS, max_samples=iq.shape[1], max_bursts=8, seizure_events=True) as r:
        _, recs, bounds = _feed(r, _iq_parts(iq), r.push_iq, seizures=False)
        bits, _ = r.debug_slicer_bits(0, bounds[-1])
        want = seizureref.events(bits, IQ_SPS, bounds)
        assert len(want) == 16 and sum(len(a) for a in recs) == 16
        with pytest.raises(capi.AmpsError) as e:
            r.drain_seizures()
        assert e.value.code == -errno.ENOSPC
        seizureref.assert_equal(e.value.seizures, want[:8], "what the overflow keeps")
        assert len(r.drain_seizures()) == 0                                              # and no error: the overflow was reported once


def test_a_partial_drain_leaves_the_rest(gpu):
    """cap below what is held: the oldest go out, the call says how many stay, and the next one delivers them"""
    L = capi.load()
    iq = _iq_stream(8, 24, IQ_EDGE - 200)
    with capi.Recc(n_channels=8, sps=IQ_SPS, max_samples=iq.shape[1], max_bursts=16, seizure_events=True) as r:
        _, _, bounds = _feed(r, _iq_parts(iq)[:4], r.push_iq, seizures=False, records=False)
        bits, _ = r.debug_slicer_bits(0, bounds[-1])
        want = seizureref.events(bits, IQ_SPS, bounds)
        assert len(want) == 8
        out = np.zeros(3, capi.SEIZURE_DTYPE)
        nout, nleft = capi.C.c_size_t(0), capi.C.c_size_t(0)
        assert L.amps_recc_drain_seizures(r._h, capi._hostptr(out), 3, capi.C.byref(nout), capi.C.byref(nleft)) == 0
        assert (nout.value, nleft.value) == (3, 5)
        seizureref.assert_equal(out, want[:3])
        r.drain_begin()                                                                  # independent of an open split drain
        seizureref.assert_equal(r.drain_seizures(), want[3:])
        r.drain_end()
        # argument errors
        assert L.amps_recc_drain_seizures(r._h, None, 3, capi.C.byref(nout), None) == -errno.EINVAL
        assert L.amps_recc_drain_seizures(r._h, capi._hostptr(out), 3, None, None) == -errno.EINVAL
        assert L.amps_recc_drain_seizures(r._h, None, 0, capi.C.byref(nout), None) == 0 and nout.value == 0


# ------------------------------------------------------------------------------------------------------------ 6. reset and flag off
def test_reset_empties_the_list_and_forgets_what_was_reported(gpu):
    iq = _iq_stream(8, 24, IQ_EDGE - 200)
    parts = _iq_parts(iq)[:4]
    with capi.Recc(n_channels=8, sps=IQ_SPS, max_samples=iq.shape[1], max_bursts=16, seizure_events=True) as r:
        _feed(r, parts, r.push_iq, seizures=False, records=False)
        r.reset()                                                                        # with eight undrained events
        assert len(r.drain_seizures()) == 0
        ev, _, bounds = _feed(r, parts, r.push_iq, records=False)
        want = _check_events(r, ev, bounds, IQ_SPS)
        assert len(want) == 8
        r.reset()
        ev2, _, _ = _feed(r, parts, r.push_iq, records=False)
        assert [a.tobytes() for a in ev2] == [a.tobytes() for a in ev]                   # the same stream again: the same events


def test_a_handle_without_the_flag_answers_enosys(gpu):
    with capi.Recc(n_channels=2, sps=10, max_samples=4096, max_bursts=4) as r:
        with pytest.raises(capi.AmpsError) as e:
            r.drain_seizures()
        assert e.value.code == -errno.ENOSYS
    with pytest.raises(capi.AmpsError) as e:                                             # the symbol seam alone has nothing to report
        capi.Recc(n_channels=1, max_bursts=4, seizure_events=True)
    assert e.value.code == -errno.EINVAL
