"""CPU only, no GPU: the two tables of DESIGN.md 4.7g for the carrier-offset measurement (AMPS_RECC_FLAG_STREAM_OFFSET), from the float64
model tests/streamoffsetref.py.

  (1) IQ seam: the worst |estimate - sent| of the burst estimate over synth.make_channel_block bursts, four seeds per point, offsets
      0, +700, -1500, +3000 Hz, at 10 / 6 / 3 samples per symbol and 30 / 10 / 3 dB (noise in the sampled band).
  (2) behind the channel filter: the same estimator on the CPU oracle's translate output (oracle.freq_xlating_fir with the flow graph's
      filter: gain 3, width 4.5 kHz; cut-off 10 kHz, the default, and wider ones) at 400 ksps / 2 and at 2.4 Msps / 12, offsets +-700, +-1500, +-2500 Hz, 30 and
      12 dB at the channel rate, on the very bursts tests/test_gpu_stream_offset.py sends (its seeds and centre).

A capture's position is taken from where the burst was planted: offset + 82 symbols - 1 sample (the last trigger symbol's decision
instant, tests/test_cpu_oracle.py), moved by the filter's delay in (2).  usage: python scripts/offset_estimator_cpu.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle  # noqa: E402
import streamoffsetref as sor  # noqa: E402
from gr_amps_amd import synth  # noqa: E402

OFFSETS_IQ = (0.0, 700.0, -1500.0, 3000.0)
OFFSETS_FILTER = (700.0, -700.0, 1500.0, -1500.0, 2500.0, -2500.0)
SEEDS = (9100, 9101, 9102, 9103)
FILTER_SEED = 9200                                                   # tests/test_gpu_stream_offset.py: FILTER_SEED
# name: (front-end rate, decimation, channel centre, cut-off of the channel filter; gain 3 and width 4.5 kHz throughout)
FORMS = {"400k_d2": (400e3, 2, 160e3, 10e3), "2400k_d12": (2.4e6, 12, 615e3, 10e3),
         "400k_d2_13k": (400e3, 2, 160e3, 13e3), "400k_d2_16k": (400e3, 2, 160e3, 16e3), "2400k_d12_16k": (2.4e6, 12, 615e3, 16e3)}


def capture_position(offset, sps):
    return int(offset) + 82 * int(sps) - 1


def iq_estimate(seed, sps, snr_db, cfo):
    n = 4000 + 1000 + (3374 + 300) * sps
    iq, truth = synth.make_channel_block(n, 1, seed=seed, sps=sps, snr_db=snr_db, first=2000, cfo_hz=cfo)
    assert len(truth) == 1
    hz, cnt = sor.burst_offset_hz(sor.blocks(iq)[0], capture_position(truth[0][0], sps), sps)
    assert cnt > 0
    return hz


def filtered_burst(form, snr_db, cfo, seed=FILTER_SEED):
    """(input stream at the front-end rate, the burst's offset in it, taps): one burst at `cfo` from the form's centre; snr_db is stated
    at the CHANNEL rate (200 ksps), so the noise per input sample is that much stronger by the decimation"""
    fs, decim, fc, _ = FORMS[form]
    sps_in = 10 * decim
    n = 4000 * decim + (3374 + 300) * sps_in
    iq, truth = synth.make_channel_block(n, 1, seed=seed, sps=sps_in, snr_db=snr_db - 10.0 * np.log10(decim), first=2000 * decim, cfo_hz=cfo)
    assert len(truth) == 1
    x = (iq * np.exp(2j * np.pi * fc * np.arange(n) / fs)).astype(np.complex64)
    return x, truth[0][0]


def filtered_position(form, offset_in, ntaps):
    decim = FORMS[form][1]
    return (int(offset_in) + (ntaps - 1) // 2) // decim + 82 * 10 - 1


def filter_estimate(form, snr_db, cfo):
    fs, decim, fc, cutoff = FORMS[form]
    x, off = filtered_burst(form, snr_db, cfo)
    taps = oracle.firdes_low_pass(3.0, fs, cutoff, 4.5e3)
    y = oracle.freq_xlating_fir(x, taps, fc, fs, decim)
    hz, cnt = sor.burst_offset_hz(sor.blocks(y)[0], filtered_position(form, off, len(taps)), 10)
    assert cnt > 0
    return hz


def example_errors():
    """examples/decode_subband.py --cfo in its plain form (21 centres of an 800 ksps stream, / 4, cut-off 16 kHz), the same seeds and
    offsets: [(channel, sent, estimate)] from the oracle's filter on each centre"""
    from gr_amps_amd import capi
    rate, decim, nsamp, first, gap = 800e3, 4, 400_000, 4000, 11000
    centres = capi.control_channel_centers("A", capi.reverse_channel_hz(323))
    k = np.arange(nsamp)
    x = np.zeros(nsamp, np.complex128)
    planted = []
    for c, fc in enumerate(centres):
        f = 1200.0 + 150.0 * (c % 5 - 2)
        iq, truth = synth.make_channel_block(nsamp, 1, seed=7000 + c, sps=10 * decim, snr_db=40.0, first=first + gap * c, cfo_hz=f)
        x += iq * np.exp(2j * np.pi * fc * k / rate)
        planted.append((truth[0][0], f))
    x = x.astype(np.complex64)
    taps = oracle.firdes_low_pass(3.0, rate, 16e3, 4.5e3)
    out = []
    for c, fc in enumerate(centres):
        y = oracle.freq_xlating_fir(x, taps, fc, rate, decim)
        pos = (planted[c][0] + (len(taps) - 1) // 2) // decim + 82 * 10 - 1
        hz, cnt = sor.burst_offset_hz(sor.blocks(y)[0], pos, 10)
        assert cnt > 0
        out.append((c, planted[c][1], hz))
    return out


def main():
    print("(1) IQ seam, worst |estimate - sent| in Hz over %d seeds x offsets %s" % (len(SEEDS), OFFSETS_IQ))
    print("| samples per symbol | 30 dB | 10 dB | 3 dB |\n|---|---|---|---|")
    for sps in (10, 6, 3):
        row = []
        for snr in (30.0, 10.0, 3.0):
            row.append(max(abs(iq_estimate(s, sps, snr, f) - f) for s in SEEDS for f in OFFSETS_IQ))
        print("| %d | %.0f Hz | %.0f Hz | %.0f Hz |" % (sps, *row))
        sys.stdout.flush()
    print("\n(2) behind the channel filter: estimate in Hz (error), one burst per point")
    worst = {}
    for form in FORMS:
        print("\n%s, cut-off %g kHz\n| sent | 30 dB | 12 dB |\n|---|---|---|" % (form, FORMS[form][3] / 1e3))
        for f in OFFSETS_FILTER:
            cells = []
            for snr in (30.0, 12.0):
                hz = filter_estimate(form, snr, f)
                worst[(form, snr)] = max(worst.get((form, snr), 0.0), abs(hz - f))
                cells.append("%+.0f (%+.0f)" % (hz, hz - f))
            print("| %+.0f | %s | %s |" % (f, *cells))
            sys.stdout.flush()
    print("\nworst |error| per form and level:", {k: round(v, 1) for k, v in worst.items()})
    ex = example_errors()
    print("\n(3) examples/decode_subband.py --cfo (800 ksps / 4, 21 adjacent channels, cut-off 16 kHz, 40 dB): channel sent estimate")
    for c, f, hz in ex:
        print("  %2d %+7.1f %+7.1f (%+.1f)" % (c, f, hz, hz - f))
    print("worst |error| %.1f Hz; median estimate %+.1f Hz (the tuner is +1200 Hz off)" % (max(abs(hz - f) for _, f, hz in ex), float(np.median([hz for _, _, hz in ex]))))


if __name__ == "__main__":
    main()
