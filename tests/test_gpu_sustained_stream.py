"""-m gpu: the wideband and the IQ seam over SEVERAL TURNS of the slicer-bit ring.  Every other GPU test creates its handle for the
whole stream of the test, so the ring (R = next_pow2(max_samples_per_push + sps * 3586 + 1024) samples) holds all of it; a receiver
creates the handle for one block and pushes blocks for hours.  Here the handles are created for a BLOCK and the streams are a little
over three turns long: captures wait in pending[c] for eight or nine pushes, the capture gather, block 0 of the timing rule and the
in-kernel search read across the physical end of the ring, the filter bank writes its words at wrapped positions, next_allowed[c] is
carried across pushes and turns, and the ring's capacity formula alone keeps a capture taken at the last possible push in the ring.

The yardstick is the second statement (tests/trackref.py, tests/refdecode.py, through tests/bitsref.py) on the DEVICE'S OWN slicer
bits, read push by push (Recc.debug_slicer_bits) and concatenated; on the IQ seam also the CPU model (oracle.Fused) push by push.
Everything behind the slicer is integer logic on those bits: every comparison is exact -- positions, every record field, every one of
the 3374 kept symbols, the push after which a record is drained -- on all rows, no record excluded.  The coverage conditions (a capture
window holds each ring end; n_c lies just behind one and in the last word in front of one; captures complete on both sides of a push
edge; a second trigger is dropped here and accepted there across a ring end) are computed from the second statement on those bits, not
assumed from the synthesis; tests/test_cpu_sustained_stream.py rehearses them without a GPU.  bitsref.sustained_plan says what is planted.
Every test prints the number of records compared and its own wall time (the first of a decimation includes the synthesis)."""
import errno
import time

import numpy as np
import pytest

import bitsref
import oracle
from gr_amps_amd import capi
from conftest import wb_cfg
from test_gpu_short_input import LIMIT

pytestmark = pytest.mark.gpu

FIRST, C = bitsref.FIRST, bitsref.ROWS
WHOLE = 12 + 8 + 1                                             # whole bursts with a tail: round three ring ends, the sweep, "tight"
_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _handle(D, max_samples, **kw):
    wb, sps = wb_cfg(D, FIRST)
    return capi.Recc(n_channels=C, sps=sps, max_samples=max_samples, max_bursts=512, wideband=wb, **kw)


def _stream(dev, D):
    """(plan, x on the device, MINs)"""
    def make():
        plan = bitsref.sustained_plan(D)
        x, mins = bitsref.sustained_stream(plan, device=dev)
        return plan, x, mins
    return _cached(("stream", D), make)


def _parts(x, D, frames, block):
    """the stream (one sample per entry of its first axis) cut into blocks of `block` frames; the last one is what is left"""
    return [x[a * D:min(a + block, frames) * D] for a in range(0, frames, block)]


def _by_channel(recs, blobs=None):
    order = np.lexsort((recs["position"], recs["channel"]))
    return recs[order] if blobs is None else (recs[order], blobs[order])


def _read_every_push(r, parts, push="push_wideband", keep=True):
    """push, drain, read `produced` and the new slicer bits -- after every block: (records per push, blobs per push, produced after each
    push, bits [rows][produced])"""
    got, blobs, produced, bits, prev = [], [], [], [], 0
    for part in parts:
        getattr(r, push)(part)
        if keep:
            rec, blob = r.drain_bursts()
            blobs.append(blob)
        else:
            rec = r.drain()
        got.append(rec)
        now = r.debug_slicer_bits(0, 0)[1]
        bits.append(r.debug_slicer_bits(prev, now - prev)[0])
        produced.append(now)
        prev = now
    return got, blobs, produced, np.concatenate(bits, axis=1)


def _attributed(got, produced, sps):
    """every record was drained after push k, the first push with n_c + span_done < produced[k]; returns the push of every record"""
    pushes = []
    for k, recs in enumerate(got):
        for nc in recs["position"].astype(np.int64).tolist():
            first = next((i for i, p in enumerate(produced) if nc + bitsref.span_done(sps) < p), None)
            assert first == k, ("n_c", nc, "drained after push", k, "its tail was complete after push", first)
            pushes.append(k)
    return pushes


def _ring_edge(r, R):
    """the ring holds exactly the last R samples produced: one word further back is -ERANGE"""
    produced = r.debug_slicer_bits(0, 0)[1]
    assert produced > 3 * R
    r.debug_slicer_bits(produced - R, 64)
    with pytest.raises(capi.AmpsError) as e:
        r.debug_slicer_bits(produced - R - 64, 64)
    assert e.value.code == -errno.ERANGE
    return produced


def _run1(dev, D, tol):
    """the yardstick run: 20 ms blocks, device-resident, everything read after every push"""
    def make():
        plan, x, _ = _stream(dev, D)
        with _handle(D, plan["block"] + 72, sync_tolerance=tol, keep_bursts=True) as r:
            got, blobs, produced, bits = _read_every_push(r, _parts(x, D, plan["frames"], plan["block"]))
        return dict(got=got, blobs=blobs, produced=produced, bits=bits, records=np.concatenate(got), kept=np.concatenate(blobs))
    return _cached(("run1", D, tol), make)


def _planted_rows(plan):
    return sorted({row for _, row, _ in plan["bursts"]} | set(bitsref.HOLD_ROWS))


def _upto(recs, blobs, sps, n_done):
    """the records (sorted by channel and position) whose tail was complete once n_done samples had been produced"""
    recs, blobs = _by_channel(recs, blobs)
    keep = recs["position"].astype(np.int64) + bitsref.span_done(sps) < n_done
    return recs[keep], blobs[keep]


# --------------------------------------------------------------------------------------------------- 1. real-time blocks, read every push
@pytest.mark.parametrize("tol", [0, 3])
def test_real_time_blocks_read_every_push(gpu, decim, tol):
    """51 200 frames in 20 ms blocks (800 frames at D = 768, 1200 at D = 512: no multiple of 64, the filter bank's carry changes from push
    to push) through a handle created for ONE block: R = 16384, more than three turns.  All records, with their kept symbols, against
    the second statement on the concatenated bits; every record drained after exactly the push that completed its tail."""
    t0 = time.perf_counter()
    D, sps = decim, 1536 // decim
    plan, _, mins = _stream(gpu, D)
    R, block, frames = plan["R"], plan["block"], plan["frames"]
    assert bitsref.ring_samples(block + 72, sps) == R == 16384
    run = _run1(gpu, D, tol)
    produced, bits, recs = run["produced"], run["bits"], run["records"]
    n_done = produced[-1]
    assert produced == [min((k + 1) * block, frames) // 64 * 64 for k in range(-(-frames // block))] and n_done == frames > 3 * R
    m = bitsref.matches_all_rows(bits, sps, tol)
    assert sorted(np.nonzero(m.any(axis=1))[0].tolist()) == _planted_rows(plan)     # triggers on planted rows only: all other rows are checked by this
    rows = sorted(set(_planted_rows(plan)) | {int(c) for c in recs["channel"]})
    compared = bitsref.check_records(recs, run["kept"], bits, rows, sps, tol, True, n_done)
    pushes = _attributed(run["got"], produced, sps)
    # the conditions, from the second statement on the device's bits
    f = bitsref.sustained_facts(bits, plan, mins, tol, n_done)
    lead = bitsref.capture_lead(sps)
    print(f"\n(1) D={D} tol={tol}: {compared} records compared ({WHOLE} + {f['held']}), drained after pushes {min(pushes)}..{max(pushes)} of "
          f"{len(produced)}; ring ends in capture windows { {k: len(v) for k, v in f['wraps'].items()} }; n_c - R behind / last word: "
          f"{f['nc']['wrap 1 behind'][0] - R} / {f['nc']['wrap 1 last word'][0] - R}; sweep n_c + span - E: {f['sweep']}; "
          f"hold-off gaps {f['gaps']}; {time.perf_counter() - t0:.2f} s")
    assert all(f["min_ok"].values()), f["min_ok"]             # one record with the planted MIN per whole burst, none for the unfinished one
    assert set(f["wraps"]) == {1, 2, 3} and all(len(v) >= 2 for v in f["wraps"].values())
    for k in (1, 2):
        (behind,), (last,) = f["nc"][f"wrap {k} behind"], f["nc"][f"wrap {k} last word"]
        assert 0 <= behind - k * R < lead and -64 <= last - k * R < 0
    assert len(f["sweep"]) == 8 and min(f["sweep"]) < 0 <= max(f["sweep"])
    E, p = plan["E"], bitsref.SWEEP_PUSH[D]
    assert produced[p - 1] == E
    for row, nc in zip(bitsref.SWEEP_ROWS, [f["nc"][f"sweep {i}"][0] for i in range(8)]):
        (at,) = [k for k, g in enumerate(run["got"]) if row in g["channel"]]
        assert at == (p - 1 if nc + bitsref.span_done(sps) < E else p), (row, nc, at)
    assert set(f["held"]) == {1, 2} and all(len(h) == 2 and h[0] < R <= h[1] for h in f["hold_runs"]), (f["held"], f["hold_runs"])
    assert [g[0] for g in f["gaps"]] == [-2, -1, 0, 1, 2]
    assert compared == len(recs) == WHOLE + sum(f["held"]) and WHOLE + 5 < compared < WHOLE + 10


# ------------------------------------------------------------------------------------------------------------------ 2. back to back
def test_real_time_blocks_back_to_back_from_host_memory(gpu, decim):
    """the same blocks from pageable host memory (the staging path), nothing read in between: the split drain every fourth push and once
    at the end gives run 1's records, byte for byte.  Then once more from another origin (the physical ring ends lie elsewhere), drained
    with the kept symbols every fourth push -- the split drain has no form that returns them: records equal after subtracting the
    origin, and every kept symbol."""
    t0 = time.perf_counter()
    D, sps = decim, 1536 // decim
    plan, x, _ = _stream(gpu, D)
    run = _run1(gpu, D, 0)
    want, want_kept = _by_channel(run["records"], run["kept"])
    parts = _parts(x.cpu().numpy(), D, plan["frames"], plan["block"])
    with _handle(D, plan["block"] + 72) as r:
        got, open_ = [], False
        for k, part in enumerate(parts):
            r.push_wideband(part)
            if k % 4 == 3:                                     # collect the list closed four pushes ago, close the current one: no wait for this push
                if open_:
                    got.append(r.drain_end())
                r.drain_begin()
                open_ = True
        got.append(r.drain_end())
        r.drain_begin()
        got.append(r.drain_end())
        assert len(r.drain()) == 0
    got = _by_channel(np.concatenate(got))
    assert len(got) == len(want) and got.tobytes() == want.tobytes()
    origin = (1 << 42) + 64 * 999 + 8192
    with _handle(D, plan["block"] + 72, keep_bursts=True) as r:
        r.set_origin(origin)
        moved = []
        for k, part in enumerate(parts):
            r.push_wideband(part)
            if k % 4 == 3 or k == len(parts) - 1:
                moved.append(r.drain_bursts())
        assert r.debug_slicer_bits(0, 0)[1] == origin + plan["frames"]
    recs, kept = _by_channel(np.concatenate([a for a, _ in moved]), np.concatenate([b for _, b in moved]))
    assert (recs["position"] >= origin).all()
    recs["position"] -= origin
    assert recs.tobytes() == want.tobytes() and np.array_equal(kept, want_kept)
    print(f"\n(2) D={D}: {len(got)} + {len(recs)} records byte-equal to the read-every-push run; {time.perf_counter() - t0:.2f} s")
    assert len(got) == len(recs) > WHOLE


# ---------------------------------------------------------------------------------------------------------------- 3. the tightest ring
def test_tightest_ring_read_every_push(gpu, decim):
    """max_samples_per_push = the largest multiple of 64 for which the ring is still 16384 samples, blocks of exactly that many frames
    (the carry stays 0, every push produces max_samples_per_push): a capture that just misses a push is taken a whole block later and
    uses the most of the ring the formula ever lets one use.  What is left of the stream goes in as a last, shorter block."""
    t0 = time.perf_counter()
    D, sps = decim, 1536 // decim
    plan, x, mins = _stream(gpu, D)
    R, block, frames = plan["R"], plan["tight_block"], plan["frames"]
    assert block == bitsref.largest_block(R, sps) == {768: 8128, 512: 4544}[D] and block % 64 == 0
    assert bitsref.ring_samples(block, sps) == R and bitsref.ring_samples(block + 64, sps) == 2 * R
    run = _run1(gpu, D, 0)
    with _handle(D, block, keep_bursts=True) as r:
        got, blobs, produced, bits = _read_every_push(r, _parts(x, D, frames, block))
        _ring_edge(r, R)
    whole = frames // block
    assert produced == [(k + 1) * block for k in range(whole)] + [frames]
    assert np.array_equal(bits, run["bits"])
    recs, kept = np.concatenate(got), np.concatenate(blobs)
    rows = sorted(set(_planted_rows(plan)) | {int(c) for c in recs["channel"]})
    compared = bitsref.check_records(recs, kept, bits, rows, sps, 0, True, frames)
    pushes = _attributed(got, produced, sps)
    # after the last whole block: run 1's records whose tail is complete by then, byte for byte
    n_b = whole * block
    early, early_kept = _by_channel(np.concatenate(got[:whole]), np.concatenate(blobs[:whole]))
    want, want_kept = _upto(run["records"], run["kept"], sps, n_b)
    assert len(early) and early.tobytes() == want.tobytes() and np.array_equal(early_kept, want_kept)
    all_, all_kept = _by_channel(recs, kept)
    want, want_kept = _by_channel(run["records"], run["kept"])
    assert all_.tobytes() == want.tobytes() and np.array_equal(all_kept, want_kept)
    # the capture that needs the most of the ring: its tail was complete a few samples AFTER the end of a push
    f = bitsref.sustained_facts(bits, plan, mins, 0, frames)
    (late,) = f["tight"]
    (at,) = [k for k, g in enumerate(got) if bitsref.TIGHT_ROW in g["channel"]]
    print(f"\n(3) D={D}: {compared} records compared, blocks of {block}; {len(early)} of them by sample {n_b}; the tight capture's tail ends "
          f"{late} samples behind push {bitsref.TIGHT_PUSH[D]} and is drained after push {at + 1}; needs "
          f"{block + late + bitsref.capture_lead(sps) + 63} of {R} ring samples at most; {time.perf_counter() - t0:.2f} s")
    assert 0 <= late < 64 and at == bitsref.TIGHT_PUSH[D] and produced[at - 1] == plan["tight_E"]
    if D == 768:
        # the exact edge, n_c + span_done == produced, of a trigger found in that very push (the block is longer than a burst): the
        # resolve kernel decides it where it walks the push's own hits, not where it looks at pending[c]
        assert late == 0 and f["nc"]["tight"][0] > produced[at - 2]
    assert compared == len(run["records"]) and len(set(pushes)) > 3


# -------------------------------------------------------------------------------------------------------------------- 4. one-shot tie
def test_one_push_of_the_whole_stream_gives_the_same(gpu, decim):
    """what the rest of the suite does -- a handle for the whole stream, one push, 64 frames of silence -- gives the same bits, and the
    same records as far as the blocks' stream received their tails"""
    import torch
    t0 = time.perf_counter()
    D, sps = decim, 1536 // decim
    plan, x, _ = _stream(gpu, D)
    frames = plan["frames"]
    run = _run1(gpu, D, 0)
    quiet = torch.zeros(64 * D, dtype=torch.complex64, device=gpu)
    with _handle(D, frames + 72, keep_bursts=True) as r:
        r.push_wideband(x)
        r.push_wideband(quiet)
        recs, kept = r.drain_bursts()
        n_done = r.debug_slicer_bits(0, 0)[1]
        bits = r.debug_slicer_bits(0, frames)[0]
    assert n_done == frames + 64 and np.array_equal(bits, run["bits"])
    got, got_kept = _upto(recs, kept, sps, frames)
    want, want_kept = _by_channel(run["records"], run["kept"])
    print(f"\n(4) D={D}: {len(got)} of the one push's {len(recs)} records have their tail inside the stream; {time.perf_counter() - t0:.2f} s")
    assert len(got) > WHOLE and got.tobytes() == want.tobytes() and np.array_equal(got_kept, want_kept)


# -------------------------------------------------------------------------------------------------------------------- 5. 16-bit input
def test_real_time_blocks_of_16_bit_samples(gpu, decim):
    """run 1's form through push_wideband_short, on the stream scaled by a power of two and rounded to int16 (as
    tests/test_gpu_short_input.py quantises): its own bits, its own records -- nothing is compared across the sample types"""
    import torch
    t0 = time.perf_counter()
    D, sps = decim, 1536 // decim
    plan, x, _ = _stream(gpu, D)
    xr = torch.view_as_real(x)
    peak = float(xr.abs().max())
    s = 2.0 ** np.floor(np.log2(LIMIT / peak))
    if peak * s >= LIMIT:
        s /= 2
    assert peak * s < LIMIT <= peak * 2 * s
    q = torch.round(xr * float(s)).to(torch.int16)            # a power of two: the product is exact, the rounding is to nearest even (np.rint)
    assert int(q.abs().max()) < LIMIT
    with _handle(D, plan["block"] + 72, keep_bursts=True) as r:
        got, blobs, produced, bits = _read_every_push(r, _parts(q, D, plan["frames"], plan["block"]), "push_wideband_short")
        _ring_edge(r, plan["R"])
    assert produced[-1] == plan["frames"]
    recs, kept = np.concatenate(got), np.concatenate(blobs)
    compared = bitsref.check_records(recs, kept, bits, range(C), sps, 0, True, produced[-1])
    pushes = _attributed(got, produced, sps)
    print(f"\n(5) D={D}: {compared} records compared, scale {s:g}, drained after pushes {min(pushes)}..{max(pushes)}; {time.perf_counter() - t0:.2f} s")
    assert compared == len(recs) > WHOLE


# ------------------------------------------------------------------------------------------------------- 6. reset clears what waits
def test_reset_clears_the_capture_that_waits(gpu, decim):
    """after the last block the ring has turned three times (one word behind its window is -ERANGE) and the unfinished burst's capture
    waits in pending[c]; reset() forgets it: silence long enough to cover its tail -- counted from the old stream's start, where a
    capture that survived the reset would wait -- yields no record on any row, and `produced` restarts with the silence"""
    import torch
    t0 = time.perf_counter()
    D, sps = decim, 1536 // decim
    plan, x, _ = _stream(gpu, D)
    R, block, frames = plan["R"], plan["block"], plan["frames"]
    run = _run1(gpu, D, 0)
    row = bitsref.UNFINISHED_ROW
    runs = bitsref.run_starts(bitsref.matches_all_rows(run["bits"][row], sps, 0)[0], sps)
    assert len(runs) == 1 and runs[0][0] + 64 < frames <= runs[0][0] + bitsref.span_done(sps)      # found, and its tail never received
    assert row not in run["records"]["channel"]
    quiet = torch.zeros(block * D, dtype=torch.complex64, device=gpu)
    pushes = -(-(runs[0][0] + 2 + bitsref.span_done(sps)) // block) + 2
    with _handle(D, block + 72) as r:
        for part in _parts(x, D, frames, block):
            r.push_wideband(part)
        before = r.drain()
        assert _ring_edge(r, R) == frames
        r.reset()
        assert r.debug_slicer_bits(0, 0)[1] == 0
        after = []
        for k in range(pushes):
            r.push_wideband(quiet)
            if k % 8 == 7 or k == pushes - 1:
                after.append(r.drain())
        produced = r.debug_slicer_bits(0, 0)[1]
    assert _by_channel(before).tobytes() == _by_channel(run["records"]).tobytes() and row not in before["channel"]
    print(f"\n(6) D={D}: {len(before)} records before the reset, {sum(len(a) for a in after)} in {pushes * block} frames of silence behind it; "
          f"{time.perf_counter() - t0:.2f} s")
    assert produced == pushes * block // 64 * 64 > runs[0][0] + 1 + bitsref.span_done(sps)
    assert all(len(a) == 0 for a in after)


# ------------------------------------------------------------------------------------------------------------------------ the IQ seam
IQ_RAGGED = [4096, 1, 63, 777, 4095, 2049]


def _iq_stream(sps, n_channels):
    def make():
        live, R, offsets = _cached(("iq live", sps), lambda: bitsref.iq_sustained_stream(sps))
        iq = np.zeros((n_channels, live.shape[1]), np.complex64)               # the live channels, then idle all-zero ones
        iq[:bitsref.IQ_LIVE] = live
        return iq, R, offsets
    return _cached(("iq", sps, n_channels), make)


def _iq_steady(sps, n_channels):
    """pushes of IQ_BLOCK samples; after every push the drained records against the CPU model's, and the new bits"""
    def make():
        iq, R, _ = _iq_stream(sps, n_channels)
        models = [oracle.Fused(c, sps) for c in range(bitsref.IQ_LIVE)]
        got, bits, prev = [], [], 0
        with capi.Recc(n_channels=n_channels, sps=sps, max_samples=bitsref.IQ_BLOCK, max_bursts=64) as r:
            for off in range(0, iq.shape[1], bitsref.IQ_BLOCK):
                r.push_iq(np.ascontiguousarray(iq[:, off:off + bitsref.IQ_BLOCK]))
                rec = r.drain()
                want = np.concatenate([m.push(iq[c, off:off + bitsref.IQ_BLOCK]) for c, m in enumerate(models)])
                assert rec.tobytes() == want.tobytes(), f"push at {off}: {len(rec)} records, the model has {len(want)}"
                now = r.debug_slicer_bits(0, 0)[1]
                assert now == off + bitsref.IQ_BLOCK
                bits.append(r.debug_slicer_bits(prev, now - prev)[0])
                got.append(rec)
                prev = now
            _ring_edge(r, R)
        return np.concatenate(got), np.concatenate(bits, axis=1)
    return _cached(("iq steady", sps, n_channels), make)


@pytest.mark.parametrize("n_channels", [4, 66], ids=["queue", "workgroup"])
@pytest.mark.parametrize("sps", [3, 10])
def test_iq_steady_pushes_over_three_turns(gpu, sps, n_channels):
    """a handle for blocks of 4096 samples (R = 16384 at three samples per symbol, 65536 at ten), a stream of 3 R + 4096: after every
    push the drain is byte-equal to the CPU model's push of the same block; at the end all records against the second statement on the
    bits read push by push.  4 channels take the capture queue; with 62 idle channels behind them the resolve kernel's own workgroup decodes."""
    t0 = time.perf_counter()
    iq, R, offsets = _iq_stream(sps, n_channels)
    assert R == bitsref.ring_samples(bitsref.IQ_BLOCK, sps) == {3: 16384, 10: 65536}[sps] and iq.shape[1] == 3 * R + bitsref.IQ_BLOCK
    recs, bits = _iq_steady(sps, n_channels)
    n_done = bits.shape[1]
    assert n_done == iq.shape[1] and bits.shape[0] == n_channels
    compared = bitsref.check_records(recs, None, bits, range(n_channels), sps, 0, True, n_done)
    f = bitsref.iq_sustained_facts(bits, sps, R, offsets, n_done)
    print(f"\n(iq) sps={sps} C={n_channels}: {compared} records compared over {n_done // bitsref.IQ_BLOCK} pushes; n_c {f['nc']}; "
          f"ring ends in capture windows {f['wraps']}; {time.perf_counter() - t0:.2f} s")
    bitsref.assert_iq_sustained_facts(f, sps, R, offsets)
    assert compared == 6


@pytest.mark.parametrize("resident", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("n_channels", [4, 66], ids=["queue", "workgroup"])
@pytest.mark.parametrize("sps", [3, 10])
def test_iq_ragged_pushes_over_three_turns(gpu, sps, n_channels, resident):
    """the same stream in pushes of 4096, 1, 63, 777, 4095, 2049, ... samples, drained every fifth push: the steady run's records"""
    import torch
    t0 = time.perf_counter()
    iq, _, _ = _iq_stream(sps, n_channels)
    want = _by_channel(_iq_steady(sps, n_channels)[0])
    got, alive, off, k = [], [], 0, 0
    with capi.Recc(n_channels=n_channels, sps=sps, max_samples=bitsref.IQ_BLOCK, max_bursts=64) as r:
        while off < iq.shape[1]:
            m = min(IQ_RAGGED[k % len(IQ_RAGGED)], iq.shape[1] - off)
            blk = np.ascontiguousarray(iq[:, off:off + m])
            if resident:                                       # a device block is read in place: it lives until a drain has covered its push
                blk = torch.from_numpy(blk).to(gpu)
                alive.append(blk)
            r.push_iq(blk)
            off += m
            k += 1
            if k % 5 == 0:
                got.append(r.drain())
                alive.clear()
        got.append(r.drain())
        assert r.debug_slicer_bits(0, 0)[1] == iq.shape[1]
    got = _by_channel(np.concatenate(got))
    print(f"\n(iq ragged) sps={sps} C={n_channels} resident={resident}: {len(got)} records over {k} pushes; {time.perf_counter() - t0:.2f} s")
    assert len(got) == 6 and got.tobytes() == want.tobytes()
