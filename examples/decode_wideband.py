"""decode_wideband.py -- the headline path in twenty lines: one 30.72 Msps complex stream in, decoded RECC seizure bursts of the whole
AMPS band out (BASELINE configs[3]; replaces 832 x [freq_xlating_fir_filter_ccc -> quadrature_demod -> clock_recovery_mm -> binary_slicer
-> amps.recc -> amps.recc_decode] of grc/recctest.grc).  Needs an MI355X: the library has no CPU path.

    python examples/decode_wideband.py            # 12 mobiles on random channels, the stream pushed in ragged blocks
    python examples/decode_wideband.py --sc16     # the same stream as a 16-bit converter delivers it: interleaved int16 I/Q, pushed as it is
    python examples/decode_wideband.py --channels 128   # one SDR's worth: a 3.84 Msps stream (or 256: 7.68, 512: 15.36) through the bank of
                                                        # that many branches, every bin a channel.  Bin channels / 2 sits on +- fs / 2, where a
                                                        # real radio's anti-alias filter rolls off: expect less of a mobile there than here
    python examples/decode_wideband.py --channels 128 --sc8   # ... as a HackRF delivers it: interleaved int8 I/Q at a full scale of 100, pushed
                                                              # as it is (2 bytes per sample); meaningful with --channels below 1024
    python examples/decode_wideband.py --channels 500 [--sc8] # a radio on a 100 MHz clock: a 5 Msps stream (or 1000: 10, 2000: 20, 2500: 25 Msps)
                                                              # through the bank of that many branches of 10 kHz, a channel on every third bin
    python examples/decode_wideband.py --channels 128 --tuner-error 9000              # a radio whose crystal is 11 ppm off at 835 MHz: every
                                                                                      # mobile 9 kHz above its bin's centre; nothing decodes
    python examples/decode_wideband.py --channels 128 --tuner-error 9000 --shift 9000 # ... corrected inside the filter bank (--channels below
                                                                                      # 1024): amps_recc_set_wideband_shift, all twelve again
    python examples/decode_wideband.py --channels 500 --tuner-error 2000 --afc        # the handle measures what is left: the first half of the
                                                                                      # stream runs uncorrected with the unit-amplitude carrier
                                                                                      # offset on, the median burst_offset of what it decoded
                                                                                      # becomes the shift, the stream goes on; nothing is reset.
                                                                                      # --afc refines: it needs bursts that still decode, about
                                                                                      # +-3 kHz of error.  A coarse search beyond that (try
                                                                                      # shifts 5 kHz apart until bursts appear) is the caller's
    python examples/decode_wideband.py --rate 8e6 [--sc8]     # a HackRF at its recommended 8 Msps, a rate that is no bank's: the first entry
                                                              # of capi.wideband_resample_plan(8e6) that keeps the whole delivered band (one
                                                              # that resamples up: 5/2 into the 2000 bank) is printed and set, and the stream
                                                              # is pushed as it arrives; the handle takes the channels of the band the resampler
                                                              # keeps flat, the bank's bins beyond the delivered band hold only its images
    python examples/decode_wideband.py --rate 4e6 --channels 500   # ... the first such entry into that bank: 4 Msps x 5/4
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gr_amps_amd import capi, synth_wideband as sw

RATE = float(sys.argv[sys.argv.index("--rate") + 1]) if "--rate" in sys.argv[1:] else 0.0          # the delivered rate where it is no bank's: a resampler in front of the bank
RESAMPLE = None
if RATE:                                          # which ratio into which bank: the first answer of the plan that resamples up, so that nothing of the band is cut off
    entries = [e for e in capi.wideband_resample_plan(RATE) if e[0] > e[1] and ("--channels" not in sys.argv[1:] or e[2] == int(sys.argv[sys.argv.index("--channels") + 1]))]
    if not entries:
        sys.exit("no bank takes %g sps through an L / M resampler that keeps the whole band (capi.wideband_resample_plan)" % RATE)
    RESAMPLE = entries[0]
    print("%g sps x %d/%d into the bank of %d branches at decimation %d: %d samples per symbol, %d taps per phase, bins of %d Hz, a channel on every %d, %d Hz usable"
          % ((RATE,) + RESAMPLE))
BANK = RESAMPLE[2] if RATE else int(sys.argv[sys.argv.index("--channels") + 1]) if "--channels" in sys.argv[1:] else 1024   # branches of the filter bank: fs = BANK x 30 kHz
GRID10 = BANK in capi.GRID10_CHANNELS             # ... or BANK x 10 kHz: bins of 10 kHz, a channel on every third one, 40 ksps per channel
BIN_HZ, STRIDE = (10e3, 3) if GRID10 else (30e3, 1)
FIRST_BIN, CHANNELS = (96, 832) if BANK == 1024 else (0, BANK // STRIDE)   # the band selection: FFT bins 96 .. 927 of the 1024-branch filter bank, or every channel of a smaller one
if RATE:                                          # the handle takes the channels inside the band the resampler keeps flat (RESAMPLE[8] Hz around the centre) and no others: the
    K = int((0.5 * RESAMPLE[8] - 15e3) // (STRIDE * BIN_HZ))   # bank's bins beyond the delivered band hold the stop band's images of the mobiles inside it, with their noise as
    FIRST_BIN, CHANNELS = (-STRIDE * K) % BANK, 2 * K + 1      # far down as they are, and an FM receiver there decodes them as well as the mobiles themselves
FS = RATE or BANK * BIN_HZ                        # of the stream as it is delivered
NSAMP = 12 * (1 << 20) * BANK // (1024 * STRIDE)  # 0.41 s of signal
if RATE:
    NSAMP = NSAMP * RESAMPLE[1] // RESAMPLE[0]    # ... in delivered samples

def _option(name, default):
    return float(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv[1:] else default


TUNER_ERROR = _option("--tuner-error", 0.0)       # the radio delivers everything this many hertz too high
SHIFT = _option("--shift", 0.0)                   # ... and the filter bank takes this many back out
AFC = "--afc" in sys.argv[1:]
if (SHIFT or AFC) and BANK == 1024:
    sys.exit("--shift and --afc need --channels below 1024: the 1024 bank has no mixer (radios that reach 30.72 Msps have a TCXO)")
BURST = 3456 * int(FS) // 20000                   # wideband samples of one burst
rng = np.random.default_rng(7)
BINS, chan_of = BANK, None
if RATE:                                          # a channel sits where it sits in hertz: the delivered band has RATE / 10 kHz bins
    BINS = int(round(RATE / 10e3))
    hz = [sw.bin_freq((FIRST_BIN + STRIDE * c) % BANK, BANK * BIN_HZ, BANK) for c in range(CHANNELS)]
    chan_of = {int(round(hz[c] / 10e3)) % BINS: c for c in range(CHANNELS)}      # delivered bin -> channel of the handle
    plan = [(int(round(hz[int(c)] / 10e3)) % BINS, int(rng.integers(4000, NSAMP - BURST - 4000))) for c in rng.choice(CHANNELS, 12, replace=False)]
else:
    plan = [((FIRST_BIN + STRIDE * int(c)) % BANK, int(rng.integers(4000, NSAMP - BURST - 4000))) for c in rng.choice(CHANNELS, 12, replace=False)]
if AFC:                                           # the shift changes at NSAMP / 2: no burst is on the air there (a burst that spans the change is not the twin's)
    plan = [(k, int(rng.integers(4000, NSAMP // 2 - BURST - 4000) if i % 2 else rng.integers(NSAMP // 2 + 4000, NSAMP - BURST - 4000))) for i, (k, _) in enumerate(plan)]
x, truth = sw.make_wideband(NSAMP, plan, seed=7, snr_db=20.0, sym_ppm=50.0, fs=FS, bins=BINS, cfo_hz=TUNER_ERROR)   # every mobile 50 ppm off the nominal bit clock

SC16 = "--sc16" in sys.argv[1:]
if SC16:                                          # full scale for the loudest sample, a power of two; no slicer decision depends on the scale
    scale = 2.0 ** np.floor(np.log2(30000.0 / max(np.abs(x.real).max(), np.abs(x.imag).max())))
    x = np.rint(np.stack([x.real, x.imag], axis=1) * scale).astype(np.int16)   # [n, 2]: 4 bytes per sample instead of 8
SC8 = "--sc8" in sys.argv[1:] and not SC16
if SC8:                                           # the loudest sample at 100 of 127
    x = np.rint(np.stack([x.real, x.imag], axis=1) * (100.0 / max(np.abs(x.real).max(), np.abs(x.imag).max()))).astype(np.int8)   # [n, 2]: 2 bytes per sample

try:
    wideband = {"channels": BANK, "first_channel": FIRST_BIN}                   # decimation: the library default (3/4 of the branches: 40 ksps per channel)
    if GRID10:
        wideband["decim"] = BANK // 4                                            # ... which the banks of 10 kHz bins want stated: 40 ksps per channel too
    if RATE:
        wideband["decim"], wideband["resample"] = RESAMPLE[3], (RATE, RESAMPLE[0], RESAMPLE[1])   # blocks arrive at RATE: set_wideband_resample
    at_bank = NSAMP * RESAMPLE[0] // RESAMPLE[1] + 1 if RATE else NSAMP                 # samples the bank sees
    rx = capi.Recc(n_channels=CHANNELS, max_samples=at_bank // (BANK // 4 if GRID10 else BANK // 2) + 72, max_bursts=256, wideband=wideband,
                   stream_offset="unit" if AFC else False)
except capi.AmpsError as e:
    sys.exit("no MI355X here (%s): the library has no CPU fallback" % e)
with rx:
    if SHIFT:
        rx.set_wideband_shift(SHIFT)
    pos, early = 0, None
    while pos < NSAMP:                            # blocks of any size: what is left of a frame waits in the handle for the next push
        n = min(int(rng.integers(100_000, 3_000_000)) * BANK // 1024, NSAMP - pos)
        if AFC and early is None:
            n = min(n, NSAMP // 2 - pos)
            if n == 0:                            # half way: steer by what has been decoded so far, then go on with the stream
                early = rx.drain()
                hz = rx.burst_offset(early)[0] if len(early) else np.zeros(0)
                if len(hz):
                    rx.set_wideband_shift(SHIFT + float(np.median(hz)))
                print("afc: %d bursts read %+.0f Hz (median); shift now %+.1f Hz" % (len(hz), float(np.median(hz)) if len(hz) else 0.0, rx.wideband_shift))
                continue
        if SC8:
            rx.push_wideband_as(x[pos:pos + n], capi.SAMPLES_SC8)
        else:
            (rx.push_wideband_short if SC16 else rx.push_wideband)(x[pos:pos + n])
        pos += n
    recs = rx.drain()
    if early is not None:
        recs = np.concatenate([early, recs])
sent = {chan_of[k] if RATE else (k - FIRST_BIN) % BANK // STRIDE: v[1] for (k, _), v in truth.items()}
print("%d bursts sent, %d decoded" % (len(sent), len(recs)))
for r in recs:
    ch, got = int(r["channel"]), r["min"].decode()
    print("  channel %3d  MIN %s  class %d  words valid %s  %s" % (ch, got, int(r["msg_class"]), "".join(str(int(v)) for v in r["valid"]),
                                                                 "ok" if sent.get(ch) == got else "MISMATCH"))
sys.exit(0 if len(recs) == len(sent) and all(sent.get(int(r["channel"])) == r["min"].decode() for r in recs) else 1)
