"""TEST INFRASTRUCTURE: the SECOND statement (tests/trackref.py: trigger runs, hold-off, the wait for a tail, the capture with its
timing rule; tests/refdecode.py + tests/bchref.py: bursts_message) as a yardstick for RECORDS, on slicer bits that somebody else made --
the device's own (Recc.debug_slicer_bits) on the GPU, the CPU model's (oracle.Fused(...).taps()[2]) without one.  Everything behind the
slicer is integer logic on those bits, so every comparison here is exact: no tolerance, no excluded record, and nothing depends on the
filter bank's float arithmetic.  This module imports no kernel code and nothing of the C model.

It also holds the synthesiser of the inputs: bursts (whole ones, or cut to their first 48 bits: dotting, word sync, coded DCC -- enough
for a trigger, cheap enough for hundreds) added to one wideband block at chosen (FFT bin, sample offset) pairs.

Measured on the float64 filter-bank model (oracle/channelizer.py) at a 30 dB floor, and relied on by the callers (who assert what they
need of it on the bits they are given): a preamble planted at sample offset `off` gives a trigger run that starts at frame
off // D + RUN_START[D], one frame later where off % D >= RUN_JUMP[D] (+- 10 samples or so: the first phase is marginal there); D
samples more move it by exactly one frame; a run is one or two matching phases long at two samples per symbol, two or three at three."""
import numpy as np

import refdecode
import trackref
from gr_amps_amd import synth, synth_wideband as sw
from test_second_restatement import _check

FS, M, SPS_WIDE = sw.FS_WIDE, sw.M, 1536                 # 30.72 Msps, 1024 bins, wideband samples per Manchester symbol
RUN_START = {768: 168, 512: 252}
RUN_JUMP = {768: 498, 512: 250}
HOLD_SYMBOLS = trackref.CAPTURE_SYMS + trackref.TRIGGER_SYMS
FIRST, ROWS = 700, 832                                   # the band of the tests: bins 700 .. 1023, 0 .. 507 (it wraps past bin 1023)


def row_bin(row):
    return (FIRST + row) % M


def sweep_plants(D, rows, first_start, slack=6):
    """(bin, offset) of one preamble per row, staggered by D + D / len(rows) samples: the sub-frame phase of the offsets sweeps one
    whole frame, and the run starts are first_start, first_start + 1, ... in the order of `rows`.  A whole frame of phase is one frame
    of position, so ONE position of the sweep is stepped over, where the phase passes RUN_JUMP[D]; the sweep begins at the phase that
    puts that step `slack` rows before its end (the rows of a sweep lie at least two channels apart, or the step smears over a
    quarter of the sweep: the neighbour's preamble, on the air at the same time, then decides a marginal first phase)."""
    n = len(rows)
    phase0 = (RUN_JUMP[D] - ((n - slack) * D) // n) % D
    base = first_start - RUN_START[D] - (1 if phase0 >= RUN_JUMP[D] else 0)
    return [(row_bin(r), (base + i) * D + phase0 + (i * D) // n) for i, r in enumerate(rows)]


def tail_frames(sps, track=True):
    """frames that must have been processed behind a capture's n_c before it is taken (trackref.captures: n_c + span < n_done)"""
    return sps * (trackref.CAPTURE_SYMS + 1) + (trackref.TRACK_BLOCKS if track else 0) + 1


# ---------------------------------------------------------------------------------------------------------------- the yardstick
def expected(bits_row, sps, tol, track, n_done):
    """[(n_c, symbols[3374], refdecode.decode(symbols))] of one row's slicer bits once n_done samples have been processed"""
    return [(nc, sym, refdecode.decode(sym)) for nc, sym in trackref.captures(bits_row, sps, tol, track, n_done)]


def matches_all_rows(bits, sps, tol=0):
    """trackref.matches for every row of bits[rows][n] at once: counts, per position, the ones under the trigger's zeros and the ones
    under its ones (what lies in front of the stream reads 1)"""
    g = np.asarray(bits, np.uint8)
    g = g[None, :] if g.ndim == 1 else g
    t = trackref.trigger_symbols()
    n = g.shape[1]
    gp = np.concatenate([np.ones((g.shape[0], sps * (len(t) - 1)), np.uint8), g], axis=1)
    under = [np.zeros(g.shape, np.uint8), np.zeros(g.shape, np.uint8)]
    for k in range(len(t)):
        under[int(t[k])] += gp[:, k * sps:k * sps + n]
    wrong = under[0].astype(np.int16) + (int(t.sum()) - under[1].astype(np.int16))
    return wrong <= tol


def run_starts(m_row, sps):
    """(start, number of matching phases) of every trigger run of one row of matches_all_rows"""
    d = trackref.DEDUP_SYMBOLS * sps
    return [(int(i), int(m_row[i:i + d].sum())) for i in np.nonzero(m_row)[0] if not m_row[max(i - d, 0):i].any()]


def check_records(records, blobs, bits, rows, sps, tol, track, n_done):
    """The records (in the order they were drained) are, row by row of `rows`, exactly what the second statement captures from
    bits[row][:n_done]: as many, in stream order, position == n_c, every field of the record (_check of
    tests/test_second_restatement.py), and -- where `blobs` (the kept 3374 symbol bytes per record) is given -- every captured symbol.
    No record may lie on a row outside `rows`.  Returns the number of records compared."""
    rows = sorted({int(r) for r in rows})
    ch = np.asarray(records["channel"]).astype(np.int64)
    stray = sorted(set(ch.tolist()) - set(rows))
    assert not stray, ("records on rows that were not to have any", stray[:8])
    assert blobs is None or len(blobs) == len(records)
    sub = np.asarray(bits)[rows][:, :n_done]
    # a row without a single match has nothing to capture (trackref.captures says so too: the screen only saves it the walk)
    live = matches_all_rows(sub, sps, tol).any(axis=1)
    compared = 0
    for j, row in enumerate(rows):
        idx = np.nonzero(ch == row)[0]
        want = expected(sub[j], sps, tol, track, n_done) if live[j] else []
        got_pos = [int(records["position"][i]) for i in idx]
        assert got_pos == [nc for nc, _, _ in want], (row, got_pos, [nc for nc, _, _ in want])
        for i, (nc, sym, dec) in zip(idx, want):
            _check(records[i], dec, (row, nc))
            if blobs is not None:
                d = np.nonzero(np.asarray(blobs[i], np.uint8) != sym)[0]
                assert d.size == 0, (row, nc, d.size, d[:8].tolist())
            compared += 1
    assert compared == len(records)
    return compared


# ---------------------------------------------------------------------------------------------------------------- the synthesiser
def noise(n, seed, floor_db=30.0, device=None):
    """complex64 [n] of white noise, floor_db below a unit carrier inside 60 kHz (sw.make_wideband's convention); numpy, or torch on
    `device` (counter-based generator, elementwise)"""
    sigma = 10.0 ** (-floor_db / 20.0) / np.sqrt(2.0) * np.sqrt(FS / 60e3)
    if device is None:
        rng = np.random.default_rng(seed)
        return (rng.standard_normal((n, 2), dtype=np.float32) * np.float32(sigma)).view(np.complex64).reshape(n)
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    return torch.view_as_complex(torch.randn(n, 2, device=device, generator=g, dtype=torch.float32) * float(sigma))


def phases(bits, ppm=0.0, cfo=0.0):
    """float64 phase (mod 2 pi) of the baseband CPFSK of a burst's bits at the wideband rate (as sw.make_wideband: +-8 kHz, the mobile's
    bit clock ppm fast, its carrier cfo Hz off)"""
    sym = synth.manchester(bits).astype(np.float64) * 2.0 - 1.0
    f = synth.symbol_waveform(sym, SPS_WIDE, ppm) * 8e3 + cfo
    return np.mod(np.cumsum(f) * (2.0 * np.pi / FS), 2.0 * np.pi)


def add(x, ph, k, off, phase, amp=1.0):
    """x[off : off + len(ph)] += amp * exp(j (ph + phase)) shifted to FFT bin k; what falls outside [0, len(x)) is dropped.
    x: numpy complex64, or a torch complex64 tensor (then `ph` is a float32 tensor on its device)."""
    n = x.shape[0]
    lo, hi = max(off, 0), min(off + ph.shape[0], n)
    if hi <= lo:
        return
    if isinstance(x, np.ndarray):
        tone = ((k * np.arange(lo, hi)) % M) * (2.0 * np.pi / M)              # bin k's carrier is periodic in M samples
        x[lo:hi] += (amp * np.exp(1j * (ph[lo - off:hi - off] + tone + phase))).astype(np.complex64)
    else:
        import torch
        tone = ((k * torch.arange(lo, hi, device=x.device)) % M).to(torch.float32) * float(2.0 * np.pi / M)
        arg = ph[lo - off:hi - off] + tone + float(phase)
        x[lo:hi] += torch.polar(torch.full_like(arg, float(amp)), arg)


def _on(device, ph):
    if device is None:
        return ph
    import torch
    return torch.from_numpy(ph.astype(np.float32)).to(device)


def plant_preambles(n, plants, seed, floor_db=30.0, device=None, nbits=48):
    """complex64 [n] (numpy; a torch tensor on `device` if given): noise, plus ONE waveform -- a random burst cut to its first `nbits`
    bits -- added at every (FFT bin, sample offset) of `plants`, each with its own random start phase"""
    rng = np.random.default_rng(seed)
    _, _, _, _, words = synth.random_message(rng)
    wave = _on(device, phases(synth.burst_bits(words, dcc=int(rng.integers(0, 4)), rng=rng)[:nbits]))
    x = noise(n, seed, floor_db, device)
    for k, off in plants:
        add(x, wave, int(k), int(off), float(rng.uniform(0, 2 * np.pi)))
    return x


FRONT_ROW, FRONT_FRAMES = 5, {768: 7300, 512: 11000}


def front_block(D, lead, seed=31):
    """a stream that starts `lead` symbols INTO the trigger of a whole burst on row FRONT_ROW (the trigger's first symbol is burst
    symbol 8): (x, the burst's MIN)"""
    x, mins = plant_bursts(FRONT_FRAMES[D] * D, [(row_bin(FRONT_ROW), -(8 + lead) * SPS_WIDE, 0.0, 0.0, 30.0)], seed + lead)
    return x, mins[0]


def plant_bursts(n, plants, seed, floor_db=30.0, device=None):
    """complex64 [n] (numpy; a torch tensor on `device` if given): noise, plus one WHOLE burst (a random message each) per (FFT bin, sample offset, ppm, carrier offset in Hz,
    carrier-to-noise in dB) of `plants`; returns (x, [MIN of each plant])"""
    rng = np.random.default_rng(seed)
    x = noise(n, seed, floor_db, device)
    mins = []
    for k, off, ppm, cfo, cn in plants:
        _, min10, _, _, words = synth.random_message(rng)
        wave = _on(device, phases(synth.burst_bits(words, dcc=int(rng.integers(0, 4)), rng=rng), float(ppm), float(cfo)))
        add(x, wave, int(k), int(off), float(rng.uniform(0, 2 * np.pi)), 10.0 ** ((cn - floor_db) / 20.0))
        mins.append(min10)
    return x, mins


# ------------------------------------------------------------- streams of several turns of the bit ring (sustained_stream tests)
def ring_samples(max_samples, sps):
    """R of include/amps_recc.h (amps_recc_debug_slicer_bits): the smallest power of two >= max_samples_per_push + sps * 3586 + 1024"""
    need = max_samples + sps * (trackref.CAPTURE_SYMS + 2 * trackref.TRIGGER_SYMS + 64) + 1024
    r = 1
    while r < need:
        r <<= 1
    return r


def largest_block(R, sps):
    """the largest max_samples_per_push, a multiple of 64, for which ring_samples still gives R"""
    m = (R - sps * (trackref.CAPTURE_SYMS + 2 * trackref.TRIGGER_SYMS + 64) - 1024) // 64 * 64
    assert m > 0 and ring_samples(m, sps) == R and ring_samples(m + 64, sps) == 2 * R
    return m


def capture_lead(sps):
    """samples in front of n_c that a capture reads: the trigger (block 0 of the timing rule) and the most the timing can move"""
    return sps * (trackref.TRIGGER_SYMS - 1) + trackref.TRACK_BLOCKS


def span_done(sps, track=True):
    """a capture is taken in the first push after which n_c + span_done < produced (trackref.captures)"""
    return tail_frames(sps, track) - 1


def window_holds(nc, sps, at):
    """the capture window [n_c - capture_lead, n_c + span_done] contains the ring position `at`"""
    return nc - capture_lead(sps) <= at <= nc + span_done(sps)


def aim(D, row, frame, phase=3):
    """(FFT bin, sample offset) at which a burst or a preamble is planted on `row` for its trigger run to start at `frame` (RUN_START;
    the offset's sub-frame phase is far from RUN_JUMP): n_c is the run's centre, `frame` or one more"""
    assert frame >= RUN_START[D] and phase < RUN_JUMP[D] - 32
    return row_bin(row), (frame - RUN_START[D]) * D + phase


SUSTAINED_R, SUSTAINED_FRAMES = 16384, 51200
REALTIME_SAMPLES = 614400                                 # 20 ms of the wideband stream: 800 frames at D = 768, 1200 at D = 512
SWEEP_PUSH = {768: 10, 512: 9}                            # the sweep straddles the end of this push (counted from 1) of the real-time blocks
TIGHT_PUSH = {768: 3, 512: 6}                             # one capture just misses the end of this push of the tightest ring's blocks
# (bit clock in ppm, carrier offset in Hz, C/N in dB): four of the mobiles of tests/test_gpu_wideband_second_statement.py (IMPAIRED)
CLEAN, MOBILES = (0, 0, 30), [(500, 0, 30), (-500, 2000, 20), (100, -2000, 30), (700, 0, 25)]
WRAP_ROWS = {1: (0, (1023 - FIRST) % M, 100, 600, 37), 2: ((0 - FIRST) % M, 777, 150, 650, 41), 3: (200, 700)}
SWEEP_ROWS, HOLD_ROWS, UNFINISHED_ROW, TIGHT_ROW = list(range(400, 416, 2)), list(range(500, 510, 2)), 250, 300


def sustained_plan(D, frames=SUSTAINED_FRAMES, R=SUSTAINED_R):
    """What the sustained-stream tests plant in `frames` frames that turn a ring of R samples several times (or, shortened, once), as
    a dictionary:
      bursts     [(tag, row, (bin, offset, ppm, cfo, C/N))] of the whole bursts, in the order plant_bursts takes them:
                 "wrap k ..."  per wrap k R that the stream holds with its tails, bursts whose capture window contains k R -- n_c aimed
                               40 samples behind it (block 0 of the timing rule and the trigger read across the ring's end), 32 in
                               front of it (the last 64-sample word), its middle and (twice) its end on k R; only the last two where the
                               stream ends too early for the others' tails
                 "sweep i"     eight bursts a frame apart (sweep_plants) whose n_c + span_done straddle E, the samples produced after
                               push SWEEP_PUSH of 20 ms blocks
                 "tight"       n_c + span_done aimed AT the end of push TIGHT_PUSH of the tightest ring's blocks (not below it: not
                               taken yet): taken a whole block later, the capture that needs the most of the ring.  At D = 768 the
                               block is longer than a burst, so its trigger is found in that very push
                 "unfinished"  begins so late that its tail is never received
      preambles  [(bin, offset)]: on each of HOLD_ROWS two, the second one the hold-off + j frames behind the first, j = -2 .. 2; the
                 first run start lies in front of R, the second behind it
      E, tight_E, tight_block, block (frames of a 20 ms block)
    The tags say what is aimed at; the tests establish what was hit from the second statement on the bits."""
    sps = SPS_WIDE // D
    span, hold = span_done(sps), sps * HOLD_SYMBOLS
    block = REALTIME_SAMPLES // D
    assert block * D == REALTIME_SAMPLES and block % 64
    bursts = []
    mob = iter(MOBILES * 2)
    for k in sorted(WRAP_ROWS):
        at = k * R
        full = [("behind", 40, CLEAN), ("last word", -32, CLEAN), ("middle", -sps * 1700, None), ("end", 300 - span, CLEAN), ("late end", 1500 - span, None)]
        if at + 41 + span + 64 >= frames:
            full = full[3:]
        if at + full[-1][1] + 1 + span + 64 >= frames:
            continue
        assert len(full) == len(WRAP_ROWS[k])
        for (what, dt, imp), row in zip(full, WRAP_ROWS[k]):
            bursts.append((f"wrap {k} {what}", row, aim(D, row, at + dt) + (imp or next(mob))))
    E = SWEEP_PUSH[D] * block // 64 * 64
    for i, (b, off) in enumerate(sweep_plants(D, SWEEP_ROWS, E - span - 4)):
        bursts.append((f"sweep {i}", SWEEP_ROWS[i], (b, off) + CLEAN))
    tight_block = largest_block(R, sps)
    tight_E = TIGHT_PUSH[D] * tight_block
    bursts.append(("tight", TIGHT_ROW, aim(D, TIGHT_ROW, tight_E - span) + CLEAN))
    bursts.append(("unfinished", UNFINISHED_ROW, aim(D, UNFINISHED_ROW, frames - 3000) + CLEAN))
    preambles = []
    for j, row in zip(range(-2, 3), HOLD_ROWS):
        b, off = aim(D, row, R - hold + 300)
        preambles += [(b, off), (b, off + (hold + j) * D)]
    assert frames % 64 == 0 and tight_E + 64 <= frames
    return dict(D=D, sps=sps, R=R, frames=frames, block=block, bursts=bursts, preambles=preambles, E=E, tight_E=tight_E, tight_block=tight_block)


def sustained_stream(plan, seed=211, device=None):
    """(x complex64 [frames * D], [MIN of each burst of the plan]): the bursts on a 30 dB floor, the preambles added on top"""
    n = plan["frames"] * plan["D"]
    x, mins = plant_bursts(n, [p for _, _, p in plan["bursts"]], seed, device=device)
    rng = np.random.default_rng(seed + 1)
    _, _, _, _, words = synth.random_message(rng)
    wave = _on(device, phases(synth.burst_bits(words, dcc=int(rng.integers(0, 4)), rng=rng)[:48]))
    for k, off in plan["preambles"]:
        add(x, wave, int(k), int(off), float(rng.uniform(0, 2 * np.pi)))
    return x, mins


def sustained_facts(bits, plan, mins, tol, n_done):
    """What the second statement says of the planted rows of bits[ROWS][>= n_done] -- the conditions the sustained-stream tests assert:
      nc         {tag: [n_c of the row's captures]}
      min_ok     {tag: exactly one capture, and it decodes to the planted MIN} (no capture at all for "unfinished")
      wraps      {k: tags whose capture window contains k R}
      sweep      [n_c + span_done - E] of the sweep rows
      tight      [n_c + span_done - tight_E] of the "tight" row
      held       [captures on each hold-off row],  hold_runs [its run starts],  gaps [second run start - first - hold-off]"""
    sps, R = plan["sps"], plan["R"]
    f = dict(nc={}, min_ok={}, wraps={}, sweep=[], tight=[], held=[], gaps=[], hold_runs=[])
    for (tag, row, _), min10 in zip(plan["bursts"], mins):
        got = expected(bits[row][:n_done], sps, tol, True, n_done)
        f["nc"][tag] = [nc for nc, _, _ in got]
        f["min_ok"][tag] = got == [] if tag == "unfinished" else len(got) == 1 and got[0][2]["min"] == min10
        for nc, _, _ in got:
            for k in range(1, n_done // R + 1):
                if window_holds(nc, sps, k * R):
                    f["wraps"].setdefault(k, []).append(tag)
            if tag.startswith("sweep"):
                f["sweep"].append(nc + span_done(sps) - plan["E"])
            if tag == "tight":
                f["tight"].append(nc + span_done(sps) - plan["tight_E"])
    for row in HOLD_ROWS:
        runs = run_starts(matches_all_rows(bits[row][:n_done], sps, tol)[0], sps)
        f["held"].append(len(expected(bits[row][:n_done], sps, tol, True, n_done)))
        f["gaps"].append([b[0] - a[0] - sps * HOLD_SYMBOLS for a, b in zip(runs, runs[1:])])
        f["hold_runs"].append([s for s, _ in runs])
    return f


IQ_BLOCK, IQ_LIVE = 4096, 4


def iq_sustained_stream(sps, seed=5):
    """The IQ seam's stream of a little over three turns of its ring (handle created for blocks of IQ_BLOCK samples):
    (iq complex64 [IQ_LIVE][3 R + IQ_BLOCK], R, offsets) with synth.fsk_modulate bursts at explicit offsets (`offsets`: per channel).
      channel 0  n_c aimed 40 samples behind R, and a second whole burst that begins 20 symbols behind the first one's end: inside its
                 hold-off, the trigger behind it (accepted)
      channel 1  n_c aimed 32 samples in front of 2 R
      channel 2  the capture's end on 3 R
      channel 3  a burst cut to 1000 bits whose capture holds R, a whole burst 100 symbols behind its end (its trigger inside the
                 hold-off: dropped, many pushes after the first was found), and one whose capture's end lies on 3 R"""
    R = ring_samples(IQ_BLOCK, sps)
    n, span = 3 * R + IQ_BLOCK, span_done(sps)
    rng = np.random.default_rng(seed)

    def burst(nbits=None):
        _, _, _, _, words = synth.random_message(rng)
        return synth.burst_bits(words, dcc=int(rng.integers(0, 4)), rng=rng)[:nbits]

    at = lambda nc: nc - 82 * sps + 1                          # a burst's 41 preamble bits end at its n_c
    plan = [[(at(R + 40), burst()), (at(R + 40) + 3476 * sps, burst())],
            [(at(2 * R - 32), burst())],
            [(at(3 * R - span + 300), burst())],
            [(at(R - 1700 * sps), burst(1000)), (at(R - 1700 * sps) + 2100 * sps, burst()), (at(3 * R - span + 1500), burst())]]
    iq = np.stack([synth.fsk_modulate(n, b, sps=sps, fs=20e3 * sps, snr_db=30.0, rng=rng) for b in plan])
    return iq, R, [[off for off, _ in b] for b in plan]


def iq_sustained_facts(bits, sps, R, offsets, n_done, tol=0):
    """the second statement on bits[IQ_LIVE][>= n_done] of iq_sustained_stream: nc [per channel, the captures' n_c], runs [per channel,
    the trigger run starts], wraps [per channel, the k whose k R lies in one of its capture windows]"""
    f = dict(nc=[], runs=[], wraps=[])
    for c in range(IQ_LIVE):
        g = np.asarray(bits[c][:n_done])
        f["nc"].append([nc for nc, _ in trackref.captures(g, sps, tol, True, n_done)])
        f["runs"].append([s for s, _ in run_starts(matches_all_rows(g, sps, tol)[0], sps)])
        f["wraps"].append(sorted({k for nc in f["nc"][c] for k in range(1, 4) if window_holds(nc, sps, k * R)}))
    return f


def assert_iq_sustained_facts(f, sps, R, offsets):
    """the conditions of the IQ seam's sustained stream (see iq_sustained_stream), asserted from iq_sustained_facts"""
    hold, lead = sps * HOLD_SYMBOLS, capture_lead(sps)
    assert [len(n) for n in f["nc"]] == [2, 1, 1, 2], f["nc"]
    assert all(f["wraps"]), f["wraps"]                          # on every live channel a capture window holds a multiple of R
    assert {k for w in f["wraps"] for k in w} == {1, 2, 3}
    assert 0 <= f["nc"][0][0] - R < lead                        # block 0 of the timing rule and the trigger read across the ring's end
    assert -64 <= f["nc"][1][0] - 2 * R < 0                     # n_c in the last word in front of 2 R
    # channel 0: the second burst BEGINS inside the first one's hold-off, its trigger lies behind it: accepted
    assert offsets[0][1] < f["nc"][0][0] + hold <= f["runs"][0][1] and len(f["runs"][0]) == 2
    # channel 3: a run start inside the hold-off of the first capture is dropped; the next one is accepted
    inside = [s for s in f["runs"][3] if f["nc"][3][0] < s < f["nc"][3][0] + hold]
    assert len(inside) >= 1 and not set(inside) & set(f["nc"][3]) and f["nc"][3][1] > f["nc"][3][0] + hold
