"""decode_subband.py -- the receiver most people can build: ONE modest SDR tuned to the middle of system A's 21 reverse control
channels (AMPS channels 313 .. 333, 834.39 .. 834.99 MHz: 630 kHz), delivering one 800 ksps complex stream; the shared translate
seam filters all 21 channels out of it in one launch (amps_recc_set_xlate_shared / amps_recc_push_raw_shared) and the fused chain
behind it decodes them.  Replaces 21 x [freq_xlating_fir_filter_ccc -> quadrature_demod -> clock_recovery_mm -> binary_slicer ->
amps.recc -> amps.recc_decode] of grc/recctest.grc.  Needs an MI355X: the library has no CPU path.

    python examples/decode_subband.py             # one mobile per control channel, the stream pushed in ragged blocks
    python examples/decode_subband.py --sc16      # the same stream as an SDR delivers it: interleaved int16, pushed as it is
                                                  # (amps_recc_push_raw_shared_as; --sc8 / --cu8 likewise take capi.SAMPLES_SC8 / _CU8)
    python examples/decode_subband.py --rtl       # an RTL-SDR at its usual 2.4 Msps, tuned between the two systems: BOTH systems' 42
                                                  # control channels (313 .. 354, 1.26 MHz) from one cu8 stream, decimated by 12
                                                  # (capi.subband_plan(2.4e6) lists the decimations a rate admits)
    python examples/decode_subband.py --rtl2048   # the same dongle at 2.048 Msps, the rate most RTL-SDR tools default to: no integer
                                                  # decimation reaches a symbol rate, so the stage resamples by 5/64 to 160 ksps, 8
                                                  # samples per symbol (Recc.set_xlate_resampled; capi.resample_plan(2.048e6))
    python examples/decode_subband.py --rssi      # with any of the above: the mobiles arrive 0, 3, 6, 9 and 12 dB down in turn, the handle
                                                  # keeps received power (Recc(stream_power=True)) and every decoded MIN is printed with
                                                  # its burst power in dB relative to the strongest (Recc.burst_power)
    python examples/decode_subband.py --cfo       # with any of the above: the tuner's crystal is 1.4 ppm off (+1200 Hz at 835 MHz) and every
                                                  # mobile a little off on its own (-300 .. +300 Hz); the handle measures carrier offsets
                                                  # (Recc(stream_offset=True)) behind a channel filter opened to 16 kHz -- behind the default
                                                  # 10 kHz one the figure is not usable -- and every decoded MIN is printed
                                                  # with the offset sent and read (Recc.burst_offset); the median is the tuner's error
    python examples/decode_subband.py --cfo-unit  # the --cfo scenario behind the DEFAULT 10 kHz filter, measured with the unit-amplitude
                                                  # statistic (Recc(stream_offset="unit")), which has the right sign there and reads within
                                                  # a few tens of Hz; a burst the narrow filter costs is reported, not counted as a failure
    python examples/decode_subband.py --afc       # steering by it: a second half-second follows with a new burst per channel; the first
                                                  # half is measured as --cfo-unit, every centre is moved by the median of its decoded
                                                  # bursts (Recc.retune_xlate: nothing is reset, the stream goes on) and the second half's
                                                  # residual median is printed -- the mobiles' own offsets are all that is left
    python examples/decode_subband.py --seizures  # with any of the above: the handle keeps seizure events (Recc(seizure_events=True)), drained
                                                  # after every push (Recc.drain_seizures), and the stream is pushed in 2 ms blocks; every
                                                  # burst is printed with found_at - position in milliseconds of stream -- how long after
                                                  # its trigger the seizure was reported: the block length at most (+ 128 samples), where
                                                  # its record takes 169 ms more
    python examples/decode_subband.py --early     # with any of the above: the handle keeps early messages (Recc(early_messages=True)); the
                                                  # stream is pushed in 2 ms blocks and the early messages and the records are drained after
                                                  # every push (Recc.drain_early, Recc.drain).  Per mobile: stream time from its trigger to
                                                  # its early message -- 24 ms per announced word and at most a block -- and to its record,
                                                  # 169 ms and at most a block; the early message's MIN is the record's
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gr_amps_amd import capi, synth

RTL2048 = "--rtl2048" in sys.argv[1:]
RTL = "--rtl" in sys.argv[1:] or RTL2048
RSSI = "--rssi" in sys.argv[1:]
AFC = "--afc" in sys.argv[1:]
SEIZURES = "--seizures" in sys.argv[1:]
EARLY = "--early" in sys.argv[1:]
CFO_UNIT = "--cfo-unit" in sys.argv[1:] or AFC
CFO = "--cfo" in sys.argv[1:] or CFO_UNIT
TUNER_HZ = 1200.0                                 # --cfo: what every channel is off by; mobile c adds (c % 5 - 2) * 150 Hz of its own
CFO_CUTOFF = 0.0 if CFO_UNIT else 16e3            # --cfo: the channel filter's cut-off (0 = the flow graph's 10 kHz: --cfo-unit, --afc, and otherwise)
HALVES = 2 if AFC else 1                          # --afc: a second stretch of NSAMP samples, one more burst per channel
INTERP, SPS = 1, 10
if RTL2048:
    RATE, INTERP, DECIM, SPS, NSAMP = 2.048e6, 5, 64, 8, 1_024_000   # 0.5 s of signal; 2.048 Msps x 5/64 = 160 ksps per channel
    assert capi.subband_plan(RATE) == [] and (INTERP, DECIM, SPS, 1531) in capi.resample_plan(RATE)   # 1531 taps per phase
    TUNED = 0.5 * (capi.reverse_channel_hz(333) + capi.reverse_channel_hz(334))
    centres = capi.control_channel_centers("AB", TUNED)
    FIRST, GAP = 10000, 13500
elif RTL:
    RATE, DECIM, NSAMP = 2.4e6, 12, 1_200_000     # 0.5 s of signal; 2.4 Msps / 12 = 200 ksps per channel
    assert (DECIM, 10, 1793) in capi.subband_plan(RATE)          # the channel filter has 1793 taps at this rate
    TUNED = 0.5 * (capi.reverse_channel_hz(333) + capi.reverse_channel_hz(334))   # between the systems: no channel on the tuner's DC
    centres = capi.control_channel_centers("AB", TUNED)          # -615 kHz .. +615 kHz in 30 kHz steps
    FIRST, GAP = 12000, 16000
else:
    RATE, DECIM, NSAMP = 800e3, 4, 400_000        # 0.5 s of signal; 800 ksps / 4 = 200 ksps per channel: 10 samples per symbol
    TUNED = capi.reverse_channel_hz(323)          # the SDR sits on the middle channel
    centres = capi.control_channel_centers("A", TUNED)   # -300 kHz .. +300 kHz in 30 kHz steps
    FIRST, GAP = 4000, 11000

try:
    rx = capi.Recc(n_channels=len(centres), sps=SPS, max_samples=NSAMP // DECIM if INTERP == 1 else NSAMP * INTERP // DECIM + 1, max_bursts=64,
                   stream_power=RSSI, stream_offset="unit" if CFO_UNIT else CFO, seizure_events=SEIZURES, early_messages=EARLY)
except capi.AmpsError as e:
    sys.exit("no MI355X here (%s): the library has no CPU fallback" % e)

rng = np.random.default_rng(7)
k = np.arange(NSAMP)
x = np.zeros(NSAMP * HALVES, np.complex128)
sent, sent_hz, sent2 = {}, {}, {}
seizures = []                                     # --seizures: the events, as they were drained behind every push
early, early_recs, recs_at = [], [], []           # --early: the early messages and the records as they were drained, and the samples processed by then
for c, fc in enumerate(centres):                  # one seizure burst per channel, at its own time
    iq, truth = synth.make_channel_block(NSAMP, 1, seed=7000 + c, sps=RATE / 20e3 if INTERP > 1 else 10 * DECIM, snr_db=40.0, first=FIRST + GAP * c,
                                          **({"cfo_hz": TUNER_HZ + 150.0 * (c % 5 - 2)} if CFO else {}))
    sent_hz[c] = TUNER_HZ + 150.0 * (c % 5 - 2)
    if RSSI:
        iq = iq * 10.0 ** (-3.0 * (c % 5) / 20.0)
    x[:NSAMP] += iq * np.exp(2j * np.pi * fc * k / RATE)
    sent[c] = truth[0][2]
    if AFC:                                       # the second half: another mobile on every channel, as far off as the first
        iq, truth = synth.make_channel_block(NSAMP, 1, seed=8000 + c, sps=RATE / 20e3 if INTERP > 1 else 10 * DECIM, snr_db=40.0, first=FIRST + GAP * c,
                                              cfo_hz=sent_hz[c])
        x[NSAMP:] += iq * np.exp(2j * np.pi * fc * (k + NSAMP) / RATE)
        sent2[c] = truth[0][2]
x = x.astype(np.complex64)
SC16 = "--sc16" in sys.argv[1:]
if SC16:                                          # what the SDR's converter does: scale to the converter's range and round; the seam reads
    x = np.rint(np.stack([x.real, x.imag], -1) * 2048.0).astype(np.int16)   # the [n, 2] int16 block in place -- no float copy on the host

if RTL:                                           # the dongle's converter: 8 bits, offset binary; 42 carriers at 4 units each stay within it
    x = np.clip(np.floor(np.stack([x.real, x.imag], -1) * 4.0 + 128.0), 0, 255).astype(np.uint8)

with rx:
    if INTERP > 1:
        rx.set_xlate_resampled(RATE, centres, INTERP, DECIM, cutoff_hz=CFO_CUTOFF if CFO else 0.0)
    else:
        rx.set_xlate_shared(RATE, centres, DECIM, cutoff_hz=CFO_CUTOFF if CFO else 0.0)
    def push_until(end, pos):                     # blocks of any size: samples short of a decimation step wait in the handle
        while pos < end:
            n = min(int(RATE * 2e-3) if SEIZURES or EARLY else int(rng.integers(10_000, 150_000)), end - pos)   # --seizures: 2 ms blocks, as a radio delivers
            if SC16 or RTL:
                rx.push_raw_shared_as(x[pos:pos + n], capi.SAMPLES_SC16 if SC16 else capi.SAMPLES_CU8)
            else:
                rx.push_raw_shared(x[pos:pos + n])
            if SEIZURES:
                seizures.append(rx.drain_seizures())
            if EARLY:
                early.append(rx.drain_early())
                early_recs.append(rx.drain())
                recs_at.extend([rx.debug_slicer_bits(0, 0)[1]] * len(early_recs[-1]))
            pos += n

    push_until(NSAMP, 0)
    recs = np.concatenate(early_recs + [rx.drain()]) if EARLY else rx.drain()
    power, nblk = rx.burst_power(recs) if RSSI else (None, None)
    read_hz, nblk_hz = rx.burst_offset(recs) if CFO else (None, None)
    if AFC:                                       # steer by the first half, then go on with the stream: nothing is reset
        applied = float(np.median(read_hz[nblk_hz > 0]))
        rx.retune_xlate(np.asarray(centres, np.float64) + applied)
        push_until(2 * NSAMP, NSAMP)
        recs2 = rx.drain()
        read2, nblk2 = rx.burst_offset(recs2)
print("%d bursts sent, %d decoded" % (len(sent), len(recs)))
for r in recs:
    ch, got = int(r["channel"]), r["min"].decode()
    print("  channel %3d (AMPS %d, %.2f MHz)  MIN %s  class %d  words valid %s  %s"
          % (ch, 313 + ch, (TUNED + centres[ch]) / 1e6, got, int(r["msg_class"]), "".join(str(int(v)) for v in r["valid"]),
             "ok" if sent.get(ch) == got else "MISMATCH"))
if SEIZURES:
    ev = np.concatenate(seizures)
    fs = 20e3 * SPS                               # the channel rate: position and found_at count its samples
    print("seizure events: %d, reported this long after the trigger (found_at - position):" % len(ev))
    for e in ev:
        rec = recs[(recs["channel"] == e["channel"]) & (recs["position"] == e["position"])]
        print("  channel %3d  position %8d  %6.2f ms  coded DCC %s  %s"
              % (int(e["channel"]), int(e["position"]), 1e3 * (int(e["found_at"]) - int(e["position"])) / fs,
                 "".join(str(int(b)) for b in e["dcc"]) if int(e["flags"]) & capi.SEIZURE_FLAG_DCC_COMPLETE else "(not in yet)",
                 "MIN %s" % rec[0]["min"].decode() if len(rec) else "(its record is in the second half)" if AFC else "NO RECORD"))
if EARLY:
    ev = np.concatenate(early)
    fs = 20e3 * SPS                               # the channel rate: position, found_at and the samples processed count its samples
    print("early messages: %d, stream time from the trigger to the message and to its record:" % len(ev))
    for e in ev:
        ch, pos = int(e["rec"]["channel"]), int(e["rec"]["position"])
        i = np.nonzero((recs["channel"] == ch) & (recs["position"] == pos))[0]
        after = "%6.2f ms" % (1e3 * (recs_at[i[0]] - pos) / fs) if len(i) and i[0] < len(recs_at) else "(not drained in the first half)"
        print("  channel %3d  position %8d  words %d  MIN %s  message after %6.2f ms, record after %s  %s"
              % (ch, pos, int(e["n_words"]), e["rec"]["min"].decode(), 1e3 * (int(e["found_at"]) - pos) / fs, after,
                 "ok" if len(i) and recs[i[0]]["min"] == e["rec"]["min"] else "NO RECORD" if not len(i) else "MISMATCH"))
if RSSI and len(recs):
    print("burst power, dB relative to the strongest (sent 0, -3, -6, -9, -12 dB in turn):")
    for r, p, nb in zip(recs, power, nblk):
        ch = int(r["channel"])
        rel = "%6.1f dB" % (10.0 * np.log10(p / power.max())) if nb else "  (not held)"
        print("  channel %3d  MIN %s  %s  over %d blocks of 256 samples (sent %d dB)" % (ch, r["min"].decode(), rel, int(nb), -3 * (ch % 5)))
if CFO and len(recs):
    print("carrier offset, Hz from the channel centre (the tuner %+.0f Hz off, every mobile up to 300 Hz on its own):" % TUNER_HZ)
    for r, hz, nb in zip(recs, read_hz, nblk_hz):
        ch = int(r["channel"])
        print("  channel %3d  MIN %s  sent %+7.1f Hz  read %s  over %d blocks of 256 samples"
              % (ch, r["min"].decode(), sent_hz[ch], "%+7.1f Hz" % hz if nb else "(not held)", int(nb)))
    print("tuner error (median of %d): %+.1f Hz" % (int(np.count_nonzero(nblk_hz)), float(np.median(read_hz[nblk_hz > 0]))))
if AFC:
    print("retuned every centre by %+.1f Hz; second half: %d bursts sent, %d decoded" % (applied, len(sent2), len(recs2)))
    for r, hz, nb in zip(recs2, read2, nblk2):
        ch = int(r["channel"])
        print("  channel %3d  MIN %s  left %+7.1f Hz  read %s  over %d blocks of 256 samples  %s"
              % (ch, r["min"].decode(), sent_hz[ch] - applied, "%+7.1f Hz" % hz if nb else "(not held)", int(nb),
                 "ok" if sent2.get(ch) == r["min"].decode() else "MISMATCH"))
    print("residual (median of %d): %+.1f Hz" % (int(np.count_nonzero(nblk2)), float(np.median(read2[nblk2 > 0]))))
    # centred again, every burst of the second half must be there
    sys.exit(0 if len(recs2) == len(sent2) and all(sent2.get(int(r["channel"])) == r["min"].decode() for r in recs2)
             and all(sent.get(int(r["channel"])) == r["min"].decode() for r in recs) else 1)
right = all(sent.get(int(r["channel"])) == r["min"].decode() for r in recs)
if CFO_UNIT and len(recs) < len(sent):            # 1.5 kHz off behind a 10 kHz filter: a burst may be lost; --afc is the remedy
    print("%d of %d bursts lost behind the default filter" % (len(sent) - len(recs), len(sent)))
sys.exit(0 if right and (CFO_UNIT or len(recs) == len(sent)) and len(recs) else 1)
