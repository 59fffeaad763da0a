"""not gpu: the inputs and the yardstick of tests/test_gpu_wideband_second_statement.py, rehearsed without a GPU.  Same synthesiser,
same bitsref.check_records; the slicer bits come from the CPU model (oracle.Fused(...).taps()[2]) run on the float64 filter-bank model
(oracle.channelizer.channelize) of the block, and the records from the CPU model too.  It shows that the second statement ALONE meets
the coverage conditions the GPU tests assert (a trigger that begins in front of the stream; consecutive run starts, both run lengths),
that the model agrees with it there, and that the helper rejects a corrupted record."""
import numpy as np
import pytest

import bitsref
import oracle
import trackref
from oracle import channelizer as cz
from conftest import wb_cfg


def _model(x, D, rows, tol, track=True, silence=0):
    """(records of `rows` in row order, bits [ROWS][n_done] with those rows filled in, n_done): the CPU model on the float64 bank's
    frames of x, `silence` zero samples per channel behind them"""
    sps = wb_cfg(D, bitsref.FIRST)[1]
    chan = cz.channelize(x, P=8, D=D, first_bin=bitsref.FIRST, n_channels=bitsref.ROWS)
    n_done = ((chan.shape[1] + silence) // 64) * 64
    bits = np.zeros((bitsref.ROWS, n_done), np.uint8)
    recs = []
    for row in rows:
        f = oracle.Fused(row, sps, tol, False, None, track)
        recs.append(f.push(np.concatenate([chan[row], np.zeros(silence)]).astype(np.complex64), cap=16))
        bits[row] = f.taps()[2]
    return np.concatenate(recs), bits, n_done


@pytest.mark.parametrize("lead", [4, 6, 10])
def test_tolerant_trigger_in_front_of_the_wideband_stream(decim, lead):
    D, sps = decim, 1536 // decim
    x, min10 = bitsref.front_block(D, lead)
    rows = [0, bitsref.FRONT_ROW - 1, bitsref.FRONT_ROW, bitsref.FRONT_ROW + 1, 400, bitsref.ROWS - 1]
    for tol in (8, 0):
        recs, bits, n_done = _model(x, D, rows, tol)
        compared = bitsref.check_records(recs, None, bits, rows, sps, tol, True, n_done)
        want = bitsref.expected(bits[bitsref.FRONT_ROW], sps, tol, True, n_done)
        print(f"\nD={D} lead={lead} tol={tol}: {compared} record(s) compared, n_c = {[nc for nc, _, _ in want]}")
        if tol == 8:
            # block 0's window (37 bits in front of n_c) lies partly in front of the stream, and the burst is the planted one
            assert compared == 1 and len(want) == 1 and want[0][0] <= 73 * sps and want[0][2]["min"] == min10
        else:
            assert compared == 0 and want == []
        assert np.array_equal(bitsref.matches_all_rows(bits[rows], sps, tol),
                              np.stack([trackref.matches(bits[r], sps, tol) for r in rows]))


@pytest.mark.parametrize("tol", [0, 3])
def test_sweep_of_run_starts_and_a_corrupted_record(decim, tol):
    """48 preambles in 900 frames, their run starts on 48 consecutive positions; the channels then fall silent long enough for the
    captures' tails (zeros pushed at the channel rate: the float64 bank is not needed for silence)"""
    D, sps = decim, 1536 // decim
    frames, p0 = 900, 384
    rows = [0, bitsref.ROWS - 1, (1023 - bitsref.FIRST) % 1024, (0 - bitsref.FIRST) % 1024] + list(range(100, 188, 2))
    x = bitsref.plant_preambles(frames * D, bitsref.sweep_plants(D, rows, p0), seed=5)
    silence = bitsref.tail_frames(sps) + 64
    recs, bits, n_done = _model(x, D, rows, tol, silence=silence)
    compared = bitsref.check_records(recs, None, bits, rows, sps, tol, True, n_done)
    print(f"\nD={D} tol={tol}: {compared} records compared")
    m = bitsref.matches_all_rows(bits[rows], sps, tol)
    runs = [bitsref.run_starts(m[j], sps) for j in range(len(rows))]
    assert all(len(r) == 1 for r in runs) and compared == len(rows)
    starts = [r[0][0] for r in runs]
    print("run starts - p0:", [s - p0 for s in starts], "lengths:", [r[0][1] for r in runs])
    # one frame per D samples, and one position stepped over near the sweep's end (bitsref.sweep_plants)
    assert starts[:36] == list(range(p0, p0 + 36)) and starts[-1] == p0 + len(rows) and all(b - a in (1, 2) for a, b in zip(starts, starts[1:]))
    assert {r[0][1] for r in runs} == ({1, 2} if sps == 2 else {2, 3})
    # the helper sees a wrong position, a wrong symbol of a blob, a missing record and a record on a row that has none
    blobs = np.stack([sym for row in rows for _, sym, _ in bitsref.expected(bits[row], sps, tol, True, n_done)])
    assert bitsref.check_records(recs, blobs, bits, rows, sps, tol, True, n_done) == len(rows)
    bad = recs.copy()
    bad["position"][7] += 1
    with pytest.raises(AssertionError):
        bitsref.check_records(bad, blobs, bits, rows, sps, tol, True, n_done)
    flipped = blobs.copy()
    flipped[11, 2000] ^= 1
    with pytest.raises(AssertionError):
        bitsref.check_records(recs, flipped, bits, rows, sps, tol, True, n_done)
    with pytest.raises(AssertionError):
        bitsref.check_records(recs[1:], blobs[1:], bits, rows, sps, tol, True, n_done)
    with pytest.raises(AssertionError):
        bitsref.check_records(recs, blobs, bits, rows[1:], sps, tol, True, n_done)
    field = recs.copy()
    field["b_MIN2"][3] ^= 1
    with pytest.raises(AssertionError):
        bitsref.check_records(field, blobs, bits, rows, sps, tol, True, n_done)
