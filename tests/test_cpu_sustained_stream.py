"""not gpu: the streams and the conditions of tests/test_gpu_sustained_stream.py, rehearsed without a GPU.  The wideband stream is the
same plan (bitsref.sustained_plan) shortened to ONE turn of the ring: the offsets relative to a ring end k R are the same for every k
(a whole number of frames more moves a run start by exactly that many frames), so what holds round R holds round 2 R and 3 R.  The slicer
bits come from the CPU model (oracle.Fused(...).taps()[2]) on the float64 filter-bank model, for the planted rows only; the IQ seam's
stream is rehearsed whole.  This is where the offsets were tuned: the GPU tests are not the first place the conditions are evaluated."""
import time

import numpy as np
import pytest

import bitsref
import oracle
from oracle import channelizer as cz

CPU_FRAMES = {768: 24512, 512: 27392}                         # one ring end, the tails behind it, and the "tight" capture


def test_ring_and_block_geometry(decim):
    """the header's formula (include/amps_recc.h, amps_recc_debug_slicer_bits) gives R = 16384 for the real-time handle and for the
    largest block of the tightest ring, and no more than that block"""
    D, sps = decim, 1536 // decim
    plan = bitsref.sustained_plan(D)
    assert plan["block"] == {768: 800, 512: 1200}[D]
    assert bitsref.ring_samples(plan["block"] + 72, sps) == plan["R"] == 16384
    assert plan["tight_block"] == {768: 8128, 512: 4544}[D]
    assert bitsref.ring_samples(plan["tight_block"], sps) == 16384 and bitsref.ring_samples(plan["tight_block"] + 64, sps) == 32768
    assert plan["frames"] > 3 * plan["R"]
    # the window a capture taken at the last possible push needs, and what the formula leaves: a capture that just
    # misses a push (n_c + span_done == produced) is taken one block later and reads from n_c - capture_lead, rounded down to a word
    need = plan["tight_block"] + bitsref.span_done(sps) + bitsref.capture_lead(sps) + 63
    assert need == plan["tight_block"] + sps * 3448 + 135 and plan["R"] - need == {768: 1225, 512: 1361}[D]
    # rows of bursts that are on the air together lie at least two channels apart (the two rows round the bin wrap carry theirs a turn apart)
    rows = sorted(row for _, row, _ in plan["bursts"]) + bitsref.HOLD_ROWS
    close = [(a, b) for a, b in zip(sorted(rows), sorted(rows)[1:]) if b - a < 2]
    assert close == [((1023 - bitsref.FIRST) % 1024, (0 - bitsref.FIRST) % 1024)]
    # nothing that crosses a ring end lies on the band's last row
    assert max(rows) < bitsref.ROWS - 1


def test_the_conditions_hold_round_one_ring_end(decim):
    t0 = time.perf_counter()
    D, sps = decim, 1536 // decim
    plan = bitsref.sustained_plan(D, CPU_FRAMES[D])
    x, mins = bitsref.sustained_stream(plan)
    rows = sorted({row for _, row, _ in plan["bursts"]} | set(bitsref.HOLD_ROWS))
    chan = cz.channelize(x, P=8, D=D, first_bin=bitsref.FIRST, n_channels=bitsref.ROWS)[rows].astype(np.complex64)
    n_done = CPU_FRAMES[D]
    assert chan.shape == (len(rows), n_done)
    R, lead = plan["R"], bitsref.capture_lead(sps)
    tags = [t for t, _, _ in plan["bursts"]]
    assert tags[:5] == ["wrap 1 behind", "wrap 1 last word", "wrap 1 middle", "wrap 1 end", "wrap 1 late end"] and len(tags) == 5 + 8 + 2
    for tol in (0, 3):
        models = [oracle.Fused(row, sps, tol) for row in rows]
        recs = np.concatenate([m.push(chan[j], cap=16) for j, m in enumerate(models)])
        bits = np.zeros((bitsref.ROWS, n_done), np.uint8)
        bits[rows] = np.stack([m.taps()[2] for m in models])
        compared = bitsref.check_records(recs, None, bits, rows, sps, tol, True, n_done)
        f = bitsref.sustained_facts(bits, plan, mins, tol, n_done)
        print(f"\nD={D} tol={tol}: {compared} records compared; n_c - R: { {t: [n - R for n in v] for t, v in f['nc'].items() if t.startswith('wrap')} }; "
              f"sweep {f['sweep']}; tight {f['tight']}; held {f['held']} gaps {f['gaps']}; {time.perf_counter() - t0:.1f} s")
        assert all(f["min_ok"].values()), f["min_ok"]
        assert f["wraps"] == {1: tags[:5]}
        (behind,), (last,) = f["nc"]["wrap 1 behind"], f["nc"]["wrap 1 last word"]
        assert 0 <= behind - R < lead and -64 <= last - R < 0
        assert len(f["sweep"]) == 8 and min(f["sweep"]) < 0 <= max(f["sweep"])
        assert f["tight"] == [{768: 0, 512: 1}[D]]          # 0: n_c + span_done == produced, the exact edge of "<"
        assert set(f["held"]) == {1, 2} and all(len(r) == 2 and r[0] < R <= r[1] for r in f["hold_runs"]), (f["held"], f["hold_runs"])
        assert [g[0] for g in f["gaps"]] == [-2, -1, 0, 1, 2]
        assert compared == 14 + sum(f["held"])


@pytest.mark.parametrize("sps", [3, 10])
def test_the_iq_stream_meets_its_conditions(sps):
    iq, R, offsets = bitsref.iq_sustained_stream(sps)
    assert R == {3: 16384, 10: 65536}[sps] and iq.shape == (bitsref.IQ_LIVE, 3 * R + bitsref.IQ_BLOCK)
    models = [oracle.Fused(c, sps) for c in range(bitsref.IQ_LIVE)]
    recs = np.concatenate([m.push(iq[c]) for c, m in enumerate(models)])
    bits = np.stack([m.taps()[2] for m in models])
    n_done = bits.shape[1]
    assert n_done == iq.shape[1]
    assert bitsref.check_records(recs, None, bits, range(bitsref.IQ_LIVE), sps, 0, True, n_done) == 6
    f = bitsref.iq_sustained_facts(bits, sps, R, offsets, n_done)
    print(f"\nsps={sps}: n_c {f['nc']}, run starts {f['runs']}, ring ends in capture windows {f['wraps']}")
    bitsref.assert_iq_sustained_facts(f, sps, R, offsets)
