"""-m gpu: a handle of a narrow filter bank (512, 256, 128 branches; chz_narrow_kernel, then capture_run_iq -- at D = 3 M / 4 the only
production route into recc_front_kernel<2, ...> and the two-sample resolve, capture and search kernels) held to what the suite holds
the 1024 bank's handles to:

  1  the slicer bits of every channel and frame (amps_recc_debug_slicer_bits), every spec: exactly the CPU model's (oracle.Fused) on
     the bank's own output, exactly the same under a ragged push schedule read after every push, and against the float64 statement
     (tests/slicerbound.py on oracle/channelizer.py) within the row's own measured bank error;
  2  16-bit input at bit level: one-shot, ragged, alternating with fc32, the ends of the int16 range, device-resident blocks;
  3  several turns of the bit ring at M = 128: a handle for one 20 ms block, a stream of 3 R + 2048 frames, everything read after every
     push, all records and kept symbols against the second statement (tests/bitsref.py) on the device's own bits;
  4  reset, set_origin, a refused oversized push;
  5  containment of non-finite wideband samples.
Every comparison but 1c is exact.  tests/narrowstream.py holds the schedule, the float64 statement and the ring stream;
tests/test_cpu_narrow_handles.py rehearses the inputs without a GPU.  The block is narrowblock.burst_block: 0.19 s of stream, six bursts."""
import errno
import time

import numpy as np
import pytest

import bitsref
import valuecases as vc
from gr_amps_amd import capi
from test_gpu_short_input import quantise
from test_gpu_wideband_bits import EXPLAINED_FRAC

import narrowblock as nb
import narrowstream as ns

pytestmark = pytest.mark.gpu
GEO = pytest.mark.parametrize("M,D", nb.GEOMETRIES, ids=nb.IDS)
SPEC = pytest.mark.parametrize("spec,sid", ns.SPECS)
TWO = pytest.mark.parametrize("M,D", [(512, 256), (128, 96)], ids=["M512-D256", "M128-D96"])
POISONED = pytest.mark.parametrize("M,D", [(128, 96), (256, 128), (512, 384)], ids=["M128-D96", "M256-D128", "M512-D384"])

_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _cap(M, D):
    return (len(nb.burst_block(M, D)[0]) + 64 * D) // D + 72


def _chan(M, D):
    """the bank's own output of the block (debug_channelize), complex64 [M][frames]"""
    def make():
        with ns.handle(M, D, _cap(M, D)) as r:
            return r.debug_channelize(nb.burst_block(M, D)[0])
    return _cached(("chan", M, D), make)


def _oneshot(M, D, spec):
    def make():
        with ns.handle(M, D, _cap(M, D), slicer=spec) as r:
            r.push_wideband(nb.burst_block(M, D)[0])
            return ns.all_bits(r)
    return _cached(("one", M, D, spec), make)


def _push_ragged(r, M, D, blocks, kinds, check=None):
    """the ragged schedule: blocks = {"f": complex64 [n], "s": int16 [n, 2]}, kinds = the sample type of each push in turn ("f", "s",
    "fs", "sf"); after every push `produced` is read, and with `check` the new bits and the refusal of one sample more"""
    n = len(next(iter(blocks.values())))
    sizes = ns.ragged(M, D, n)
    off, prev, parts, deltas = 0, 0, [], []
    for k, m in enumerate(sizes):
        kind = kinds[k % len(kinds)]
        (r.push_wideband_short if kind == "s" else r.push_wideband)(blocks[kind][off:off + m])
        off += m
        produced = r.debug_slicer_bits(0, 0)[1]
        assert produced == (off // D) & ~63, (off, produced)
        if check:
            bits, _ = r.debug_slicer_bits(prev, produced - prev)
            assert bits.shape == (M, produced - prev)
            parts.append(bits)
            with pytest.raises(capi.AmpsError) as e:                    # the next sample is not produced yet
                r.debug_slicer_bits(produced, 1)
            assert e.value.code == -errno.ERANGE
        deltas.append((m, produced - prev))
        prev = produced
    assert off == n
    ns.assert_ragged_holds_what_it_claims(M, D, sizes, deltas)
    return (np.concatenate(parts, axis=1) if check else ns.all_bits(r)[0]), prev


# ------------------------------------------------------------------------------------------------------------------ 1. slicer bits
@SPEC
@GEO
def test_bits_equal_the_cpu_model_every_channel_and_frame(gpu, M, D, spec, sid):
    sps = nb.sps_of(M, D)
    x, _ = nb.burst_block(M, D)
    bits, produced = _oneshot(M, D, spec)
    assert produced == (len(x) // D) & ~63 and bits.shape == (M, produced)
    model = _cached(("model", M, D, sid), lambda: ns.model_bits(_chan(M, D), sps, sid))
    assert model.shape[1] >= produced
    count, where = ns.mismatches(bits, model[:, :produced])
    assert count == 0, (count, where)
    if sid in (1, 3):
        assert bits[:, :sps].all()                                       # specs B and D slice ones while no partner exists


@SPEC
@GEO
def test_bits_ragged_pushes_equal_one_shot_read_after_every_push(gpu, M, D, spec, sid):
    x, _ = nb.burst_block(M, D)
    one, produced = _oneshot(M, D, spec)
    with ns.handle(M, D, _cap(M, D), slicer=spec) as r:
        many, p = _push_ragged(r, M, D, {"f": x}, "f", check=True)
    assert p == produced
    count, where = ns.mismatches(many, one)
    assert count == 0, (count, where)


@SPEC
@GEO
def test_bits_against_the_float64_statement(gpu, M, D, spec, sid):
    """eps is the row's own measured max |y32 - y64|, held first to FFT_C 2^-24 log2(M) ||Y64(frame)||_2 per frame.  No unexplained bit;
    explained ones at most 1e-3 of all; inside each burst no more differing bits than the reference alone has there
    (tests/test_cpu_narrow_handles.py: at most one per burst; it measures none)."""
    bits, produced = _oneshot(M, D, spec)
    worst, explained = ns.statement_check(bits, _chan(M, D), M, D, sid)
    assert explained <= EXPLAINED_FRAC * bits.size, explained
    got, ref = ns.burst_diffs(bits, M, D, sid), ns.burst_diffs(ns.ref_bits(M, D, sid), M, D, sid)
    print(f"\nM={M} D={D} spec {spec}: eps/bound max {worst:.3f}, explained differences {explained} of {bits.size}; inside the bursts: device {got}, reference {ref}")
    assert max(ref) <= 1 and all(g <= w for g, w in zip(got, ref)), (got, ref)


# ---------------------------------------------------------------------------------------------------------------- 2. 16-bit input
def _short_block(M, D):
    def make():
        q, xf, s = quantise(nb.burst_block(M, D)[0])
        print(f"\nM={M} D={D}: quantised with s = {s:g}, peak component {np.abs(q).max()}")
        return q, xf
    return _cached(("short", M, D), make)


def _twin(M, D, spec):
    def make():
        with ns.handle(M, D, _cap(M, D), slicer=spec) as r:
            r.push_wideband(_short_block(M, D)[1])
            return ns.all_bits(r)
    return _cached(("twin", M, D, spec), make)


@SPEC
@GEO
def test_short_bits_equal_the_fc32_twin(gpu, M, D, spec, sid):
    """one-shot, in the ragged schedule, and alternating sc16 and fc32 push by push in both starting orders"""
    q, xf = _short_block(M, D)
    want, produced = _twin(M, D, spec)
    assert produced == (len(q) // D) & ~63 and want.shape == (M, produced)
    with ns.handle(M, D, _cap(M, D), slicer=spec) as r:
        r.push_wideband_short(q)
        got, p = ns.all_bits(r)
    assert p == produced
    count, where = ns.mismatches(got, want)
    assert count == 0, ("one shot", count, where)
    for kinds in ("s", "sf", "fs"):
        with ns.handle(M, D, _cap(M, D), slicer=spec) as r:
            got, p = _push_ragged(r, M, D, {"s": q, "f": xf}, kinds)
        assert p == produced
        count, where = ns.mismatches(got, want)
        assert count == 0, (kinds, count, where)


@pytest.mark.parametrize("spec", ["default", "atan"])
@GEO
def test_extreme_components_ragged_pushes(gpu, M, D, spec):
    """a random 1 % of the components are -32768, -32767, -1, 0, 1 or 32767: the 16-bit reader's conversion meets the ends of its range"""
    q = _short_block(M, D)[0].copy()
    rng = np.random.default_rng(16 + M + D)
    flat = q.reshape(-1)
    idx = np.nonzero(rng.random(flat.size) < 0.01)[0]
    flat[idx] = rng.choice(np.array([-32768, -32767, -1, 0, 1, 32767], np.int16), idx.size)
    assert flat.min() == -32768 and flat.max() == 32767
    assert all((flat[idx] == v).sum() >= 1000 for v in (-32768, -32767, -1, 0, 1, 32767))
    xf = (q[:, 0].astype(np.float32) + 1j * q[:, 1].astype(np.float32)).astype(np.complex64)
    with ns.handle(M, D, _cap(M, D), slicer=spec) as r:
        r.push_wideband(xf)
        want, produced = ns.all_bits(r)
    assert produced == (len(q) // D) & ~63
    with ns.handle(M, D, _cap(M, D), slicer=spec) as r:
        got, p = _push_ragged(r, M, D, {"s": q}, "s")
    assert p == produced
    count, where = ns.mismatches(got, want)
    assert count == 0, (count, where)


@pytest.mark.parametrize("spec", ["default", "atan"])
@GEO
def test_device_blocks_give_the_host_blocks_bits(gpu, M, D, spec):
    import torch
    q, xf = _short_block(M, D)
    want, produced = _twin(M, D, spec)
    t = torch.from_numpy(q).to(gpu)                                   # [n, 2]
    pad = torch.from_numpy(np.concatenate([np.zeros((1, 2), np.int16), q])).to(gpu)
    sl = pad.reshape(-1)[2:]                                          # flat, from sample 1 of a padded buffer: 4-byte aligned, not 8
    assert sl.data_ptr() % 8 == 4
    for what, pushes in (("tensor", [t]), ("odd slice", [sl]), ("behind a one-sample host push", [q[:1], t[1:]])):
        with ns.handle(M, D, _cap(M, D), slicer=spec) as r:
            for p in pushes:
                r.push_wideband_short(p)
            got, p = ns.all_bits(r)
        assert p == produced
        count, where = ns.mismatches(got, want)
        assert count == 0, (what, count, where)


# ------------------------------------------------------------------------------------------------ 3. several turns of the bit ring
def _read_every_push(r, parts, push="push_wideband"):
    got, blobs, produced, bits, prev = [], [], [], [], 0
    for part in parts:
        getattr(r, push)(part)
        rec, blob = r.drain_bursts()
        got.append(rec)
        blobs.append(blob)
        now = r.debug_slicer_bits(0, 0)[1]
        bits.append(r.debug_slicer_bits(prev, now - prev)[0])
        produced.append(now)
        prev = now
    return got, blobs, produced, np.concatenate(bits, axis=1)


def _attributed(got, produced, sps):
    """every record was drained after push k, the first push with n_c + span_done < produced[k]"""
    pushes = []
    for k, recs in enumerate(got):
        for nc in recs["position"].astype(np.int64).tolist():
            first = next((i for i, p in enumerate(produced) if nc + bitsref.span_done(sps) < p), None)
            assert first == k, ("n_c", nc, "drained after push", k, "its tail was complete after push", first)
            pushes.append(k)
    return pushes


def _by_channel(recs, blobs):
    order = np.lexsort((recs["position"], recs["channel"]))
    return recs[order], blobs[order]


def _ring_run(D, tol):
    def make():
        plan, x, _ = ns.ring_stream(D)
        with ns.handle(ns.RING_M, D, plan["block"] + 72, max_bursts=128, sync_tolerance=tol, keep_bursts=True) as r:
            got, blobs, produced, bits = _read_every_push(r, ns.ring_parts(x, D, plan["block"]))
            # the ring holds exactly the last R samples
            r.debug_slicer_bits(produced[-1] - plan["R"], 64)
            with pytest.raises(capi.AmpsError) as e:
                r.debug_slicer_bits(produced[-1] - plan["R"] - 64, 64)
            assert e.value.code == -errno.ERANGE
        return dict(got=got, produced=produced, bits=bits, records=np.concatenate(got), kept=np.concatenate(blobs))
    return _cached(("ring", D, tol), make)


@pytest.mark.parametrize("tol", [0, 3])
@pytest.mark.parametrize("D", [96, 64])
def test_ring_turns_20ms_blocks_read_every_push(gpu, D, tol):
    """M = 128: a handle for one 20 ms block (800 frames at D = 96, 1200 at D = 64; R = 16384), 51 200 frames.  sync_tolerance 3 selects
    recc_front_kernel<sps, 1, true, SL>."""
    t0 = time.perf_counter()
    plan, x, truth = ns.ring_stream(D)
    sps, R, block, frames = plan["sps"], plan["R"], plan["block"], plan["frames"]
    assert bitsref.ring_samples(block + 72, sps) == R == 16384
    run = _ring_run(D, tol)
    produced, bits, recs = run["produced"], run["bits"], run["records"]
    n_done = produced[-1]
    assert produced == [min((k + 1) * block, frames) // 64 * 64 for k in range(-(-frames // block))] and n_done == frames > 3 * R
    compared = bitsref.check_records(recs, run["kept"], bits, range(ns.RING_M), sps, tol, True, n_done)
    pushes = _attributed(run["got"], produced, sps)
    f = ns.ring_facts(bits, plan, tol, n_done)
    print(f"\nD={D} tol={tol}: {compared} records compared, drained after pushes {min(pushes)}..{max(pushes)} of {len(produced)}; ring ends in "
          f"capture windows {f['wraps']}; sweep n_c + span - E {f['sweep']}; hold-off runs {f['runs']}; {time.perf_counter() - t0:.2f} s")
    ns.assert_ring_facts(f, plan, tol)
    # captures complete on both sides of the push edge E, each drained after the push the second statement says
    p = ns.SWEEP_PUSH[D]
    assert produced[p - 1] == plan["E"]
    for i, b in enumerate(ns.SWEEP_BINS):
        (at,) = [k for k, g in enumerate(run["got"]) if b in g["channel"]]
        assert at == (p - 1 if f["nc"][f"sweep {i}"][0] + bitsref.span_done(sps) < plan["E"] else p), (b, at)
    sent = {v[1] for (b, off), v in truth.items() if b != ns.LATE_BIN}
    assert sent <= {r["min"].decode() for r in recs} and compared == len(recs) >= len(sent) + 3 + (1 if tol else 0)


@pytest.mark.parametrize("D", [96, 64])
def test_ring_one_push_of_the_whole_stream_gives_the_same(gpu, D):
    plan, x, _ = ns.ring_stream(D)
    sps, frames = plan["sps"], plan["frames"]
    run = _ring_run(D, 0)
    with ns.handle(ns.RING_M, D, frames + 72, max_bursts=128, keep_bursts=True) as r:
        r.push_wideband(x)
        recs, kept = r.drain_bursts()
        bits, n_done = ns.all_bits(r)
    assert n_done == frames and np.array_equal(bits, run["bits"])
    got, got_kept = _by_channel(recs, kept)
    want, want_kept = _by_channel(run["records"], run["kept"])
    assert len(got) > 10 and got.tobytes() == want.tobytes() and np.array_equal(got_kept, want_kept)


@pytest.mark.parametrize("D", [96, 64])
def test_ring_turns_16_bit_blocks_give_the_fc32_twins_records(gpu, D):
    plan, x, _ = ns.ring_stream(D)
    sps, block = plan["sps"], plan["block"]
    q, xf, s = quantise(x)
    with ns.handle(ns.RING_M, D, block + 72, max_bursts=128, keep_bursts=True) as r:
        want = _read_every_push(r, ns.ring_parts(xf, D, block))
    with ns.handle(ns.RING_M, D, block + 72, max_bursts=128, keep_bursts=True) as r:
        got = _read_every_push(r, ns.ring_parts(q, D, block), "push_wideband_short")
    assert got[2] == want[2] and np.array_equal(got[3], want[3])
    assert sum(len(g) for g in want[0]) > 10
    for k, (a, b, ka, kb) in enumerate(zip(got[0], want[0], got[1], want[1])):             # push by push
        assert a.tobytes() == b.tobytes() and np.array_equal(ka, kb), k
    compared = bitsref.check_records(np.concatenate(got[0]), np.concatenate(got[1]), got[3], range(ns.RING_M), sps, 0, True, got[2][-1])
    print(f"\nD={D}: {compared} records of the 16-bit blocks (scale {s:g}) equal the fc32 twin's, push by push")


# ------------------------------------------------------------------------------------------------- 4. reset, origin, oversized push
def _fresh(M, D):
    """(bits, produced, records, kept) of a fresh handle: the block, then 64 frames of silence"""
    def make():
        with ns.handle(M, D, _cap(M, D), keep_bursts=True) as r:
            r.push_wideband(nb.burst_block(M, D)[0])
            r.push_wideband(ns.flush(D))
            recs, kept = r.drain_bursts()
            return ns.all_bits(r) + (recs, kept)
    return _cached(("fresh", M, D), make)


@TWO
def test_reset_forgets_the_carry_and_the_capture_that_waits(gpu, M, D):
    x, _ = nb.burst_block(M, D)
    sps = nb.sps_of(M, D)
    bits, produced, recs, kept = _fresh(M, D)
    assert len(recs) == 6
    step = ns.period(M, D) * D
    cut = 2 * len(x) // 5 // step * step + D + 17                      # the first 40 %: a frame and 17 samples wait in the bank's carry
    with ns.handle(M, D, _cap(M, D), keep_bursts=True) as r:
        r.push_wideband(x[:cut])
        early, p = ns.all_bits(r)
        assert len(r.drain()) == 0
        runs = [bitsref.run_starts(m, sps) for m in bitsref.matches_all_rows(early[[k for k, _ in nb.planted(M)]], sps)]
        assert all(len(s) == 1 and s[0][0] + bitsref.span_done(sps) > p for s in runs), runs      # six captures wait for their tails
        r.reset()
        assert r.debug_slicer_bits(0, 0)[1] == 0
        r.push_wideband(x)
        r.push_wideband(ns.flush(D))
        again, again_kept = r.drain_bursts()
        got, p = ns.all_bits(r)
    assert p == produced and np.array_equal(got, bits)
    assert again.tobytes() == recs.tobytes() and np.array_equal(again_kept, kept)


@pytest.mark.parametrize("origin", [64, (1 << 40) - 64 * 300, (1 << 43) + 64 * 12345])
@TWO
def test_origin_shifts_positions_and_nothing_else(gpu, M, D, origin):
    x, _ = nb.burst_block(M, D)
    bits, produced, recs, kept = _fresh(M, D)
    with ns.handle(M, D, _cap(M, D), keep_bursts=True) as r:
        r.set_origin(origin)
        assert r.debug_slicer_bits(0, 0)[1] == origin
        r.push_wideband(x[:len(x) // 3])
        with pytest.raises(capi.AmpsError) as e:                       # only on a fresh or reset handle
            r.set_origin(origin + 64)
        refused = e.value.code
        r.push_wideband(x[len(x) // 3:])
        r.push_wideband(ns.flush(D))
        moved, moved_kept = r.drain_bursts()
        got, p = r.debug_slicer_bits(origin, produced)
        with pytest.raises(capi.AmpsError) as e:                       # nothing before the origin is held
            r.debug_slicer_bits(origin - 64, 64)
        assert e.value.code == -errno.ERANGE
    assert p == origin + produced and np.array_equal(got, bits)
    assert (moved["position"] >= origin).all()
    moved["position"] -= origin
    assert moved.tobytes() == recs.tobytes() and np.array_equal(moved_kept, kept)
    # the code a handle of the 1024 bank gives
    with capi.Recc(n_channels=4, max_samples=128, max_bursts=4, wideband={"channels": 1024, "decim": 512}) as w:
        w.push_wideband(np.zeros(100, np.complex64))
        with pytest.raises(capi.AmpsError) as e:
            w.set_origin(64)
    assert refused == e.value.code == -errno.EBUSY


@TWO
def test_refused_oversized_push_leaves_the_handle_as_it_was(gpu, M, D):
    """max_samples_per_push = F: a push that would produce more than F frames answers -E2BIG, from host memory (staged, never armed) and
    from device memory; the handle then takes the stream in smaller pushes as a handle that never saw the refused ones"""
    import torch
    x, _ = nb.burst_block(M, D)
    xz = np.concatenate([x, ns.flush(D)])
    F = 2048
    sizes = [5 * D + 7] + [(F - 8) * D - 3] * 8
    cuts = np.minimum(np.cumsum([0] + sizes), len(xz))
    cuts = cuts[:int(np.argmax(cuts == len(xz))) + 1]
    assert cuts[-1] == len(xz) and len(cuts) >= 4
    big = xz[:(F + 4 + ns.period(M, D)) * D]
    dbig = torch.from_numpy(big).to(gpu)

    def run(refuse):
        with ns.handle(M, D, F, keep_bursts=True) as r:
            for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                if refuse and k in (0, 1, 2):                       # on the fresh handle, with frames in the carry, in mid-stream
                    for blk in (big, dbig):
                        with pytest.raises(capi.AmpsError) as e:
                            r.push_wideband(blk)
                        assert e.value.code == -errno.E2BIG
                    assert r.debug_slicer_bits(0, 0)[1] == (a // D) & ~63
                r.push_wideband(xz[a:b])
            recs, kept = r.drain_bursts()
            return ns.all_bits(r) + (recs, kept)

    bits, produced, recs, kept = run(False)
    want = _fresh(M, D)
    assert produced == want[1] and np.array_equal(bits, want[0]) and recs.tobytes() == want[2].tobytes() and len(recs) == 6
    got = run(True)
    assert got[1] == produced and np.array_equal(got[0], bits)
    assert got[2].tobytes() == recs.tobytes() and np.array_equal(got[3], kept)
    # exactly F frames are taken
    with ns.handle(M, D, F) as r:
        r.push_wideband(xz[:F * D + D - 1])
        assert r.debug_slicer_bits(0, 0)[1] == F


# ------------------------------------------------------------------------------- 5. containment of non-finite wideband samples
def _three_pushes(M, D, x, cuts):
    xz = np.concatenate([x, ns.flush(D)])
    edges = [0] + list(cuts) + [len(xz)]
    with ns.handle(M, D, _cap(M, D)) as r:
        chan = np.concatenate([r.debug_channelize(xz[a:b]) for a, b in zip(edges[:-1], edges[1:])], axis=1)
    with ns.handle(M, D, _cap(M, D)) as r:
        for a, b in zip(edges[:-1], edges[1:]):
            r.push_wideband(xz[a:b])
        recs = r.drain()
        return chan, ns.all_bits(r)[0], recs


@pytest.mark.parametrize("kind", sorted(vc.POISON))
@POISONED
def test_non_finite_wideband_samples_are_contained(gpu, M, D, kind):
    """one poisoned sample, and a run of 100, in the middle of a push, on the last sample of a push that ends mid-frame (the poison
    crosses pushes in the carry's leftover) and on sample 0: the bank's frames whose window does not read it, the bits outside
    [first touched, last touched + sps + 1] and the records of bursts wholly outside are the clean run's.  Nothing is asserted inside."""
    x, _ = nb.burst_block(M, D)
    sps, n = nb.sps_of(M, D), len(x)
    cuts = (n // 2 // D * D + 100, n - 9037)
    assert all(c % D for c in cuts)
    chan0, bits0, recs0 = _cached(("clean", M, D), lambda: _three_pushes(M, D, x, cuts))
    assert len(recs0) == 6
    lead, span = bitsref.capture_lead(sps), bitsref.span_done(sps)
    whole = 0
    for where, start in (("middle", (cuts[0] + cuts[1]) // 2), ("edge", cuts[1] - 1), ("start", 0)):
        for length in (1, 100):
            p0, p1 = start, start + length - 1
            chan, bits, recs = _three_pushes(M, D, vc.poison(x, kind, start, length), cuts)
            assert chan.shape == chan0.shape and bits.shape == bits0.shape
            lo, hi = ns.touched(p0, p1, M, D)
            clean = np.ones(chan.shape[1], bool)
            clean[lo:hi + 1] = False
            assert np.array_equal(np.ascontiguousarray(chan[:, clean]).view(np.uint32), np.ascontiguousarray(chan0[:, clean]).view(np.uint32)), (where, length)
            clean[lo:hi + sps + 2] = False
            count, at = ns.mismatches(bits[:, clean[:bits.shape[1]]], bits0[:, clean[:bits.shape[1]]])
            assert count == 0, (where, length, count, at)
            outside = [g for g in recs0 if int(g["position"]) + span < lo or int(g["position"]) - lead > hi + sps + 1]
            for g in outside:
                same = recs[(recs["channel"] == g["channel"]) & (recs["position"] == g["position"])]
                assert len(same) == 1 and same[0].tobytes() == g.tobytes(), (where, length, int(g["channel"]))
            whole += len(outside)
            # the middle lies inside all six bursts; all six are over before the edge; the stream's start precedes them, but at
            # D = 384 the first triggers begin within the dozen frames the poison reaches
            assert len(outside) == {"middle": 0, "edge": 6}.get(where, len(outside)) and (where != "start" or len(outside) >= 2), (where, len(outside))
    assert whole >= 16
