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
