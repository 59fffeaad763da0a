"""CPU only, no GPU: the tables of DESIGN.md 4.7g for the unit-amplitude carrier-offset statistic (AMPS_RECC_FLAG_STREAM_OFFSET_UNIT),
from the float64 models tests/streamoffsetunitref.py (unit) and tests/streamoffsetref.py (the shipped, amplitude-weighted one), on
the very bursts, seeds, filters and capture positions of scripts/offset_estimator_cpu.py.

  (1) IQ seam: the worst |estimate - sent| over four seeds x four offsets, shipped -> unit, at 10 / 3 samples per symbol and 30 / 10 / 3 dB.
  (2) behind the channel filter: estimate in Hz at 30 dB / 12 dB, shipped and unit behind the default 10 kHz cut-off at 400 ksps / 2,
      unit at 2.4 Msps / 12 (10 kHz) and at 400 ksps / 2 behind 16 kHz.
  (3) the point the tests bound: 2.4 Msps / 12, default filter, +1500 Hz, 30 dB.
  (4) examples/decode_subband.py --cfo-unit and --afc in their plain form (21 adjacent channels of an 800 ksps stream, / 4, the default
      filter, bursts overlapping in time, 40 dB): every channel's estimate, the median, and after moving every centre by it the second
      half's estimates and residual median.

usage: python scripts/offset_unit_estimator_cpu.py > profiles/stream_offset_unit/estimator_cpu.txt
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import offset_estimator_cpu as oe  # noqa: E402
import oracle  # noqa: E402
import streamoffsetref as sor  # noqa: E402
import streamoffsetunitref as sur  # noqa: E402
from gr_amps_amd import synth  # noqa: E402

OFFSETS_TABLE = (700.0, -1500.0, 2500.0, -2500.0)
MODELS = {"amp": sor, "unit": sur}


def iq_estimates(seed, sps, snr_db, cfo):
    """{statistic: estimate in Hz} of one synthetic burst on the IQ seam"""
    n = 4000 + 1000 + (3374 + 300) * sps
    iq, truth = synth.make_channel_block(n, 1, seed=seed, sps=sps, snr_db=snr_db, first=2000, cfo_hz=cfo)
    assert len(truth) == 1
    pos = oe.capture_position(truth[0][0], sps)
    return {k: m.burst_offset_hz(m.blocks(iq)[0], pos, sps)[0] for k, m in MODELS.items()}


def filter_estimates(form, snr_db, cfo):
    """{statistic: estimate in Hz} of one burst behind the form's channel filter (the CPU oracle's translate output)"""
    fs, decim, fc, cutoff = oe.FORMS[form]
    x, off = oe.filtered_burst(form, snr_db, cfo)
    taps = oracle.firdes_low_pass(3.0, fs, cutoff, 4.5e3)
    y = oracle.freq_xlating_fir(x, taps, fc, fs, decim)
    pos = oe.filtered_position(form, off, len(taps))
    return {k: m.burst_offset_hz(m.blocks(y)[0], pos, 10)[0] for k, m in MODELS.items()}


def example_halves():
    """[(channel, offset from the centre in use, estimate)] of the first half, the median applied, and the same list of the second half"""
    import numpy as np
    from gr_amps_amd import capi
    rate, decim, nsamp, first, gap, tuner = 800e3, 4, 400_000, 4000, 11000, 1200.0
    centres = capi.control_channel_centers("A", capi.reverse_channel_hz(323))
    k = np.arange(nsamp)
    x = np.zeros(2 * nsamp, np.complex128)
    starts = {}
    for c, fc in enumerate(centres):
        f = tuner + 150.0 * (c % 5 - 2)
        for half in (0, 1):
            iq, truth = synth.make_channel_block(nsamp, 1, seed=7000 + 1000 * half + c, sps=10 * decim, snr_db=40.0, first=first + gap * c, cfo_hz=f)
            x[half * nsamp:(half + 1) * nsamp] += iq * np.exp(2j * np.pi * fc * (k + half * nsamp) / rate)
            starts[(half, c)] = (truth[0][0] + half * nsamp, f)
    x = x.astype(np.complex64)
    taps = oracle.firdes_low_pass(3.0, rate, 10e3, 4.5e3)

    def half_estimates(half, shift):
        out = []
        for c, fc in enumerate(centres):
            y = oracle.freq_xlating_fir(x, taps, fc + shift, rate, decim)
            start, f = starts[(half, c)]
            pos = (start + (len(taps) - 1) // 2) // decim + 82 * 10 - 1
            hz, cnt = sur.burst_offset_hz(sur.blocks(y)[0], pos, 10)
            assert cnt > 0
            out.append((c, f - shift, hz))
        return out

    one = half_estimates(0, 0.0)
    applied = float(np.median([hz for _, _, hz in one]))
    return one, applied, half_estimates(1, applied)


def main():
    print("(1) IQ seam, worst |estimate - sent| in Hz over %d seeds x offsets %s: shipped -> unit" % (len(oe.SEEDS), oe.OFFSETS_IQ))
    print("| samples per symbol | 30 dB | 10 dB | 3 dB |\n|---|---|---|---|")
    for sps in (10, 3):
        row = []
        for snr in (30.0, 10.0, 3.0):
            worst = {"amp": 0.0, "unit": 0.0}
            for s in oe.SEEDS:
                for f in oe.OFFSETS_IQ:
                    for k, hz in iq_estimates(s, sps, snr, f).items():
                        worst[k] = max(worst[k], abs(hz - f))
            row.append("%.0f -> %.0f Hz" % (worst["amp"], worst["unit"]))
        print("| %d | %s | %s | %s |" % (sps, *row))
        sys.stdout.flush()
    print("\n(2) behind the channel filter: estimate in Hz at 30 dB / 12 dB, one burst per point (seed %d)" % oe.FILTER_SEED)
    print("| sent | 400k_d2 10 kHz: amp | same, unit | 2400k_d12 10 kHz: unit | 400k_d2 16 kHz: unit |\n|---|---|---|---|---|")
    worst = {}
    for f in OFFSETS_TABLE:
        cells = []
        for form, stat in (("400k_d2", "amp"), ("400k_d2", "unit"), ("2400k_d12", "unit"), ("400k_d2_16k", "unit")):
            hz = [filter_estimates(form, snr, f)[stat] for snr in (30.0, 12.0)]
            worst[(form, stat)] = max([worst.get((form, stat), 0.0)] + [abs(v - f) for v in hz])
            cells.append("%+.0f / %+.0f" % tuple(hz))
        print("| %+.0f | %s |" % (f, " | ".join(cells)))
        sys.stdout.flush()
    print("\nworst |error| per form and statistic:", {k: round(v, 1) for k, v in worst.items()})
    est = filter_estimates("2400k_d12", 30.0, 1500.0)
    print("\n(3) 2.4 Msps / 12, default 10 kHz filter, +1500 Hz, 30 dB: shipped %+.1f Hz, unit %+.1f Hz (error %+.1f)" % (est["amp"], est["unit"], est["unit"] - 1500.0))
    sys.stdout.flush()
    import numpy as np
    one, applied, two = example_halves()
    print("\n(4) examples/decode_subband.py --cfo-unit / --afc (800 ksps / 4, 21 adjacent channels, default 10 kHz filter, 40 dB), unit statistic")
    for title, rows in (("first half: channel sent estimate", one), ("second half, every centre moved by %+.1f Hz: channel left estimate" % applied, two)):
        print(title)
        for c, f, hz in rows:
            print("  %2d %+7.1f %+7.1f (%+.1f)" % (c, f, hz, hz - f))
        print("worst |error| %.1f Hz; median estimate %+.1f Hz" % (max(abs(hz - f) for _, f, hz in rows), float(np.median([hz for _, _, hz in rows]))))


if __name__ == "__main__":
    main()
