"""-m gpu: on the wideband seam, the device's trigger search (inside the resolve kernel), hold-off walk, capture (with the rule of its own
at two samples per symbol) and decode, held to the SECOND statement -- tests/trackref.py, tests/refdecode.py, through tests/bitsref.py --
on the DEVICE'S OWN slicer bits (Recc.debug_slicer_bits).  Everything behind the slicer is integer logic on those bits, so every
comparison is exact: positions, every record field, and with keep_bursts every one of the 3374 captured symbols; no record is excluded
and nothing depends on the filter bank's float arithmetic.  The coverage conditions of each case (the timing does move; the run starts
do lie on the edges; the second trigger is dropped here and accepted there) are computed from the second statement on those bits, not
assumed from the synthesis.

The handle is the 832-channel one whose band wraps past bin 1023 (first_channel = 700): the search runs inside the resolve kernel, and
the bit ring (max_samples) holds the whole stream of a test.  tests/test_cpu_wideband_second_statement.py rehearses the synthesiser
and the helper without a GPU.  Every test prints the number of records compared and its own wall time, synthesis included."""
import time

import numpy as np
import pytest

import bitsref
import trackref
from gr_amps_amd import capi
from conftest import wb_cfg

pytestmark = pytest.mark.gpu

FIRST, C = bitsref.FIRST, bitsref.ROWS
WRAP = ((1023 - FIRST) % 1024, (0 - FIRST) % 1024)            # the rows of bins 1023 and 0
_cache = {}


def _handle(D, frames, **kw):
    wb, sps = wb_cfg(D, FIRST)
    return capi.Recc(n_channels=C, sps=sps, max_samples=frames + 72, max_bursts=512, wideband=wb, **kw)


def _bits(r):
    produced = r.debug_slicer_bits(0, 0)[1]
    return r.debug_slicer_bits(0, produced)


def _silence(torch, dev, frames, D):
    return torch.zeros(frames * D, dtype=torch.complex64, device=dev)


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ------------------------------------------------------------------------------------------------ (a) capture where the timing decides
# (bit clock in ppm, carrier offset in Hz, C/N in dB) of the eight mobiles
IMPAIRED = [(500, 0, 30), (-500, 2000, 20), (300, -1000, 14), (-100, 2000, 12), (100, -2000, 30), (0, 0, 10), (700, 0, 25), (-300, 1000, 16)]
A_ROWS = (0, C - 1) + WRAP + (100, 600, 37, 777)
A_SAMPLES = 10000 * 768                                       # 0.25 s: whole frames at both decimations


def _block_a(torch, dev):
    def make():
        plants = [(bitsref.row_bin(r), 60000 + 230017 * i) + imp for i, (r, imp) in enumerate(zip(A_ROWS, IMPAIRED))]
        return bitsref.plant_bursts(A_SAMPLES, plants, seed=101, device=dev)
    return _cached("a", make)


@pytest.mark.parametrize("keep", [True, False], ids=["blobs", "records"])
@pytest.mark.parametrize("fixed", [False, True], ids=["tracked", "fixed"])
def test_capture_where_the_timing_decides(gpu, decim, fixed, keep):
    """eight whole bursts with clock offsets to 700 ppm, carrier offsets to 2 kHz and C/N down to 10 dB, on the band's first and last
    rows and the two round the bin wrap among others: one push, 64 frames of silence, one drain; all 832 rows are checked"""
    import torch
    t0 = time.perf_counter()
    D, sps = decim, 1536 // decim
    x, mins = _block_a(torch, gpu)
    quiet = _silence(torch, gpu, 64, D)                       # alive until the drain: device blocks are read in place
    with _handle(D, A_SAMPLES // D + 64, fixed_timing=fixed, keep_bursts=keep) as r:
        r.push_wideband(x)
        r.push_wideband(quiet)
        recs, blobs = r.drain_bursts() if keep else (r.drain(), None)
        bits, n_done = _bits(r)
    assert n_done == (A_SAMPLES // D + 64) // 64 * 64
    compared = bitsref.check_records(recs, blobs, bits, range(C), sps, 0, not fixed, n_done)
    differing = []
    for row, min10 in zip(A_ROWS, mins):
        (nc, sym, dec), = bitsref.expected(bits[row], sps, 0, not fixed, n_done)
        differing.append(int((trackref.capture(bits[row], nc, sps, True) != trackref.capture(bits[row], nc, sps, False)).sum()))
        if not fixed:
            assert dec["min"] == min10, (row, dec["min"], min10)
    print(f"\n(a) D={D} fixed={fixed} keep={keep}: {compared} records compared; symbols that tracking changes: {differing}; "
          f"{time.perf_counter() - t0:.2f} s")
    assert compared == 8
    assert sum(d > 0 for d in differing) >= 4                 # the timing rule had something to decide


# ------------------------------------------------------------------------------- (b) run starts across dword, lane, push and quarter edges
B_FRAMES, B_CUT = 10000, 512
B_ROWS = [0, C - 1, WRAP[0], WRAP[1]] + list(range(401, 777, 2))          # 192 rows, two channels apart behind the first four (bitsref.sweep_plants)


def _block_b(torch, dev, D):
    return _cached(("b", D), lambda: bitsref.plant_preambles(B_FRAMES * D, bitsref.sweep_plants(D, B_ROWS, B_CUT - 128), seed=7, device=dev))


@pytest.mark.parametrize("tol", [0, 3])
def test_run_starts_swept_across_a_push_edge(gpu, decim, tol):
    """192 preambles on 192 rows whose run starts climb one position per row while the sub-frame phase sweeps a whole frame (one
    position near the sweep's end is stepped over: bitsref.sweep_plants) -- every dword and lane phase of the search, and both the
    push edge F and the edge F - 64 up to which a push's search attributes run starts to itself.  Two pushes cut at F, then silence long
    enough for the last tail; once drained (and the ring's `produced` read) after every push, once with nothing read in between.  What
    follows the 48 bits of a preamble is noise: 192 random captures for the decode."""
    import torch
    t0 = time.perf_counter()
    D, sps = decim, 1536 // decim
    x = _block_b(torch, gpu, D)
    F = B_CUT
    quiet = max(64, -(-(F + 64 + bitsref.tail_frames(sps) + 64 - B_FRAMES) // 64) * 64)
    parts = (x[:F * D], x[F * D:], _silence(torch, gpu, quiet, D))
    with _handle(D, B_FRAMES + quiet, sync_tolerance=tol) as r:
        got, produced = [], []
        for part in parts:
            r.push_wideband(part)
            got.append(r.drain())
            produced.append(r.debug_slicer_bits(0, 0)[1])
        bits, n_done = _bits(r)
    assert produced == [F, B_FRAMES // 64 * 64, n_done] and n_done == (B_FRAMES + quiet) // 64 * 64
    compared = [bitsref.check_records(np.concatenate(got[:k + 1]), None, bits, range(C), sps, tol, True, produced[k]) for k in range(3)]
    with _handle(D, B_FRAMES + quiet, sync_tolerance=tol) as r:
        for part in parts:
            r.push_wideband(part)
        once = r.drain()
        bits2, n_done2 = _bits(r)
    assert n_done2 == n_done and np.array_equal(bits2, bits)
    assert bitsref.check_records(once, None, bits, range(C), sps, tol, True, n_done) == compared[-1]
    # the conditions, from the second statement on the device's bits
    m = bitsref.matches_all_rows(bits, sps, tol)
    assert sorted(np.nonzero(m.any(axis=1))[0].tolist()) == sorted(B_ROWS)      # no trigger anywhere else: "no record elsewhere" is a verdict
    runs = [bitsref.run_starts(m[row], sps) for row in B_ROWS]
    assert all(len(r) == 1 for r in runs)
    starts, lengths = [r[0][0] for r in runs], {r[0][1] for r in runs}
    print(f"\n(b) D={D} tol={tol}: {compared[-1]} records compared ({compared} after each push), run starts {min(starts)}..{max(starts)}, "
          f"run lengths {sorted(lengths)}, cut at {F}; {time.perf_counter() - t0:.2f} s")
    assert compared[-1] == 192
    assert {s % 128 for s in starts} == set(range(128))
    p0 = min(starts)
    assert p0 + 64 <= F - 64 and F <= p0 + 128                 # F - 64 and F lie inside the sweep,
    assert set(range(p0, F + 48)) <= set(starts)               # which has no hole from its first run start to well behind F
    if sps == 2:
        assert lengths == {1, 2}


# ------------------------------------------------------------------------- (c) one push that holds block edges, and the hold-off edges
P = 36864                                                      # four quarters of 9216 frames
Q1 = P // 4 - 64                                               # the first run start the search of quarter 1 attributes to itself
C_QROWS = [0, C - 1, WRAP[0], WRAP[1]] + list(range(2, 314, 2)) # 160 rows
C_BROWS = list(range(330, 650, 2))                             # 160 other rows
C_HROWS = list(range(700, 714, 2))                             # seven rows with two preambles each
H_START = 2000


def _block_c(torch, dev, D):
    def make():
        sps = 1536 // D
        plants = bitsref.sweep_plants(D, C_QROWS, Q1 - 80) + bitsref.sweep_plants(D, C_BROWS, Q1 + 8192 - 64 - 80)
        for j, row in zip(range(-3, 4), C_HROWS):
            off = (H_START - bitsref.RUN_START[D]) * D + 3
            plants += [(bitsref.row_bin(row), off), (bitsref.row_bin(row), off + (sps * bitsref.HOLD_SYMBOLS + j) * D)]
        return bitsref.plant_preambles(P * D, plants, seed=13, device=dev)
    return _cached(("c", D), make)


@pytest.mark.parametrize("tol", [0, 3])
def test_one_push_with_block_edges_and_the_hold_off_edges(gpu, decim, tol):
    """ONE push of 36 864 frames (synthesised on the device): each channel's four search waves take 9216 frames, more than one 8192-position
    block.  160 rows sweep their run starts over 160 positions (consecutive but for one near the sweep's end) centred on the start of quarter 1's attribution (9216 - 64),
    160 others over positions centred 8192 - 64 further on.  That the second sweep holds a block edge rests on the geometry described at
    the top of gr_amps_amd/csrc/recc_bits.hip.h: a segment's blocks of 8192 positions start at its first dword (which lies the dedup
    window in front of its first run start) rounded down to four dwords, less than 128 + 6 positions in front of 9216 - 64, so the first
    block edge of quarter 1 lies in (9216 - 64 - 134 + 8192, 9216 - 64 + 8192].  Seven further rows carry TWO preambles, the second one
    exactly the hold-off (3448 symbols) + j frames behind the first, j = -3 .. 3: dropped on some rows, accepted on others."""
    import torch
    t0 = time.perf_counter()
    D, sps = decim, 1536 // decim
    x = _block_c(torch, gpu, D)
    with _handle(D, P, sync_tolerance=tol) as r:
        r.push_wideband(x)
        recs = r.drain()
        bits, n_done = _bits(r)
    assert n_done == P
    planted = C_QROWS + C_BROWS + C_HROWS
    rows = sorted(set(planted) | {int(c) for c in recs["channel"]})
    compared = bitsref.check_records(recs, None, bits, rows, sps, tol, True, n_done)
    m = bitsref.matches_all_rows(bits[planted], sps, tol)
    runs = {row: bitsref.run_starts(m[j], sps) for j, row in enumerate(planted)}
    assert all(len(runs[row]) == 1 for row in C_QROWS + C_BROWS) and all(len(runs[row]) == 2 for row in C_HROWS)
    qs, bs = {runs[row][0][0] for row in C_QROWS}, {runs[row][0][0] for row in C_BROWS}
    assert qs >= set(range(Q1 - 80, Q1 + 65)), sorted(set(range(Q1 - 80, Q1 + 65)) - qs)
    assert bs >= set(range(Q1 + 8192 - 134, Q1 + 8192 + 1)), sorted(set(range(Q1 + 8192 - 134, Q1 + 8192 + 1)) - bs)
    held = [len(bitsref.expected(bits[row], sps, tol, True, n_done)) for row in C_HROWS]
    gaps = [runs[row][1][0] - runs[row][0][0] - sps * bitsref.HOLD_SYMBOLS for row in C_HROWS]
    print(f"\n(c) D={D} tol={tol}: {compared} records compared (320 + {held}); second run start minus first minus hold-off: {gaps}; "
          f"{time.perf_counter() - t0:.2f} s")
    assert set(held) == {1, 2}                                 # the second trigger is dropped on some rows and accepted on others
    assert compared == 320 + sum(held) and 327 < compared < 334


# ----------------------------------------------------------------- (d) a tolerant trigger that begins in front of the wideband stream
@pytest.mark.parametrize("lead", [4, 6, 10])
def test_tolerant_trigger_that_begins_in_front_of_the_wideband_stream(gpu, decim, lead):
    """the stream starts `lead` symbols INTO the trigger of a whole burst: with sync_tolerance = 8 the trigger is found with its first
    symbols never received, and block 0 of the capture's timing rule looks in front of the stream (at two samples per symbol: the
    branch of manchester_from_ring that shifts ones into its window); with tolerance 0 there is nothing.  All rows are checked."""
    import torch
    t0 = time.perf_counter()
    D, sps = decim, 1536 // decim
    x, min10 = bitsref.front_block(D, lead)
    x = torch.from_numpy(x).to(gpu)
    frames = bitsref.FRONT_FRAMES[D]
    quiet = _silence(torch, gpu, 64, D)
    out = {}
    for tol in (8, 0):
        with _handle(D, frames + 64, sync_tolerance=tol, keep_bursts=True) as r:
            r.push_wideband(x)
            r.push_wideband(quiet)
            recs, blobs = r.drain_bursts()
            bits, n_done = _bits(r)
        assert n_done == (frames + 64) // 64 * 64
        compared = bitsref.check_records(recs, blobs, bits, range(C), sps, tol, True, n_done)
        out[tol] = (compared, bitsref.expected(bits[bitsref.FRONT_ROW], sps, tol, True, n_done))
    print(f"\n(d) D={D} lead={lead}: {out[8][0]} record compared at tolerance 8 (n_c = {[nc for nc, _, _ in out[8][1]]}), "
          f"{out[0][0]} at tolerance 0; {time.perf_counter() - t0:.2f} s")
    assert out[8][0] == 1 and len(out[8][1]) == 1
    nc, _, dec = out[8][1][0]
    assert nc <= 73 * sps and dec["min"] == min10             # block 0's window lies partly in front of the stream
    assert out[0][0] == 0 and out[0][1] == []
