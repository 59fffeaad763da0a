"""not gpu: the inputs and the conditions of tests/test_gpu_narrow_handles.py, rehearsed on the reference alone -- the float64 filter
bank (oracle/channelizer.py) rounded to complex64, sliced by the CPU model (oracle.Fused).  What holds here is what the GPU tests may
ask of the device: the caps of the float64 statement, the count of differing bits inside the bursts, what the ragged schedule holds,
and every planted condition of the stream that turns the bit ring three times."""
import time

import numpy as np
import pytest

import bitsref
import oracle
from oracle import channelizer as cz
from test_gpu_wideband_bits import EXPLAINED_FRAC

import narrowblock as nb
import narrowstream as ns

GEO = pytest.mark.parametrize("M,D", nb.GEOMETRIES, ids=nb.IDS)


@GEO
def test_ragged_schedule_holds_what_it_claims(M, D):
    x, _ = nb.burst_block(M, D)
    n = len(x)
    sizes = ns.ragged(M, D, n)
    ends = np.cumsum(sizes)
    produced = [int(e // D) & ~63 for e in ends]
    deltas = list(zip(sizes, np.diff([0] + produced).tolist()))
    ns.assert_ragged_holds_what_it_claims(M, D, sizes, deltas)
    left, launches, wgs = ns.ragged_facts(M, D, sizes)
    assert sum(launches) == n // D // ns.period(M, D) * ns.period(M, D) and sum(sizes) == n


@GEO
def test_reference_meets_the_caps_of_the_float64_statement(M, D):
    """the float64 bank rounded to complex64 through oracle.Fused, all M rows, every spec: nothing unexplained, explained differences
    under the cap, and inside each burst at most one differing bit -- the count the GPU test allows the device"""
    t0 = time.perf_counter()
    sps = nb.sps_of(M, D)
    y64, norm = ns.bank64(M, D)
    y32 = y64.astype(np.complex64)
    for spec, sid in ns.SPECS:
        bits = ns.ref_bits(M, D, sid)
        assert bits.shape == (M, y64.shape[1] // 64 * 64)
        worst, explained = ns.statement_check(bits, y32, M, D, sid)
        inside = ns.burst_diffs(bits, M, D, sid)
        print(f"\nM={M} D={D} spec {spec}: rounding / bound {worst:.4f}, explained differences {explained} of {bits.size}, inside the bursts {inside}")
        assert explained <= EXPLAINED_FRAC * bits.size and explained <= 4
        assert max(inside) <= 1
        if sid in (1, 3):
            assert bits[:, :sps].all()
    print(f"{time.perf_counter() - t0:.1f} s")


def test_touched_frames():
    """ns.touched against the definition: frame m reads samples [(m + 1) D - 8 M, (m + 1) D)"""
    for M, D in nb.GEOMETRIES:
        for p0, p1 in ((0, 0), (0, 99), (5 * D - 1, 5 * D - 1), (5 * D, 5 * D + 99), (123457, 123556)):
            reads = [m for m in range(p1 // D + 8 * M // D + 4) if (m + 1) * D > p0 and (m + 1) * D - 8 * M <= p1]
            assert ns.touched(p0, p1, M, D) == (reads[0], reads[-1])


@pytest.mark.parametrize("D", [96, 64])
def test_ring_stream_meets_its_conditions(D):
    """the stream of three turns of the ring at M = 128: on the reference's bits the second statement finds every planted condition, at
    both tolerances, and the CPU model's records are the second statement's"""
    t0 = time.perf_counter()
    plan, x, truth = ns.ring_stream(D)
    sps, R, frames = plan["sps"], plan["R"], plan["frames"]
    assert bitsref.ring_samples(plan["block"] + 72, sps) == R == 16384 and frames > 3 * R and plan["block"] == {96: 800, 64: 1200}[D]
    assert plan["block"] % 64 and (ns.SWEEP_PUSH[D] * plan["block"]) // 64 * 64 == plan["E"]
    rows = ns.ring_rows(plan)
    assert {0, 127} <= set(rows) and all(b - a >= 2 for a, b in zip(rows, rows[1:]))
    chan = cz.channelize(x, P=8, M=ns.RING_M, D=D, taps=nb.taps(ns.RING_M, D))[rows].astype(np.complex64)
    assert chan.shape == (len(rows), frames)
    mins = {}
    for tol in (0, 3):
        models = [oracle.Fused(row, sps, tol) for row in rows]
        recs = np.concatenate([m.push(chan[j], cap=16) for j, m in enumerate(models)])
        bits = np.zeros((ns.RING_M, frames), np.uint8)
        bits[rows] = np.stack([m.taps()[2] for m in models])
        compared = bitsref.check_records(recs, None, bits, rows, sps, tol, True, frames)
        f = ns.ring_facts(bits, plan, tol, frames)
        print(f"\nD={D} tol={tol}: {compared} records; n_c {f['nc']}; ring ends in capture windows {f['wraps']}; sweep {f['sweep']}; runs {f['runs']}")
        ns.assert_ring_facts(f, plan, tol)
        assert compared == len(plan["whole"]) - 1 + 1 + 2 + (1 if tol else 0)
        mins[tol] = sorted(r["min"].decode() for r in recs if r["valid"].all())
    # every whole burst with a tail decodes to what was sent
    sent = sorted(v[1] for (b, off), v in truth.items() if b != ns.LATE_BIN)
    assert set(sent) <= set(mins[0]) and set(sent) <= set(mins[3])
    print(f"{time.perf_counter() - t0:.1f} s")
