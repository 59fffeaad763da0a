"""Regenerates tests/golden/wideband_frames.npz and tests/golden/wideband_records.npz -- the frozen vectors of the wideband seam, every
filter bank in every geometry (same status as make_golden.py ... make_golden_r04.py: they pin the float64 MODELS over time and travel to
the GPU box; they are not reference-derived).  tests/widebandgolden.py holds the geometries, the models and the comparisons;
tests/test_cpu_wideband_golden.py keeps the models on these files, tests/test_gpu_wideband_golden.py the device.

wideband_frames.npz: one sc8 input per bank size (int8 [128 D_max + 37, 2]) and one at 3.2 Msps for the resampled path; per geometry the
float64 bank's rows64 [8][128] (six keyed rows, two noise-only rows on either side of the wrap), norm [128], 16 points of the
definition's double sum, and the float64 slicer bits of all four specs with the mask of where a binary32 slicer may leave them; for
(128, 96) and (500, 125) the variant shifted by +6543.21 Hz with the per-frame weight of the mixer's bound; for the resampled path
three windows of the float64 resampler's output and the rows of the float64 chain.
wideband_records.npz: per burst block of the suite its SHA-256 and the records of oracle.fused_push_all on the float64 bank's rows.

The inputs are COMMITTED, not regenerated: a run reads them back from wideband_frames.npz, so that neither numpy's generator nor libm
can move them, and rewrites both files byte for byte.  `--new-inputs` draws them afresh (SEEDS: chosen so that no row's mask exceeds
the cap of tests/test_gpu_wideband_bits.py, which the script asserts; a row that fails wants another input, never another cap).
Run from the repo root:  python tests/golden/make_golden_wideband.py"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from gr_amps_amd import synth, synth_wideband as sw  # noqa: E402
import wbresampleref as wr  # noqa: E402
import widebandgolden as wg  # noqa: E402

SEEDS = {1024: 2, 512: 1, 256: 1, 128: 3, 2500: 1, 2000: 1, 1000: 1, 500: 2, "resample": 1}    # the first seed of 1, 2, ... that meets the cap
FULL_SCALE = 120.0
SNR_DB = 30.0                  # inside one channel's 60 kHz, as synth_wideband.make_wideband states it


def make_input(n, fs, carriers_hz, seed):
    """int8 [n, 2]: noise 30 dB below the carriers, a Manchester-keyed +-8 kHz FSK carrier (random bits, its own symbol timing and phase)
    at every frequency of carriers_hz, the loudest component at FULL_SCALE, then the format's extreme codes in both components"""
    rng = np.random.default_rng(seed)
    sigma = 10.0 ** (-SNR_DB / 20.0) / np.sqrt(2.0) * np.sqrt(fs / 60e3)
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)) * sigma
    sps_w = int(round(fs / 20e3))
    assert sps_w * 20e3 == fs
    t = np.arange(n)
    for f0 in carriers_hz:
        bits = rng.integers(0, 2, n // (2 * sps_w) + 2)
        sym = synth.manchester(bits).astype(np.float64) * 2.0 - 1.0
        off = int(rng.integers(0, 2 * sps_w))
        f = synth.symbol_waveform(sym, sps_w)[off:off + n] * 8e3
        ph = 2.0 * np.pi * np.cumsum(f) / fs + rng.uniform(0, 2 * np.pi)
        x += np.exp(1j * (ph + 2.0 * np.pi * f0 * t / fs))
    peak = max(np.abs(x.real).max(), np.abs(x.imag).max())
    q = np.rint(np.stack([x.real, x.imag], axis=1) * (FULL_SCALE / peak)).astype(np.int8)
    for i, pair in ((5, (-128, 127)), (6, (127, -128)), (n // 2, (-128, -128)), (n // 2 + 1, (127, 127)), (n - 3, (127, -128))):
        q[i] = pair
    return q


def new_inputs():
    inputs = {}
    for M in wg.SIZES:
        fs = wg.fs_of(M)
        hz = [sw.bin_freq(int(k), fs, M) for k in wg.row_bins(M, wg.keyed_rows(M))]
        inputs[M] = make_input(wg.input_len(M), fs, hz, SEEDS[M])
    b = wr.BURSTS["3.2M"]
    return inputs, make_input(wg.rs_input_len(), b.rate, [b.row_hz(r) for r in b.rows], SEEDS["resample"])


def committed_inputs():
    fx = wg.load_frames()
    return {M: fx["input_M%d" % M] for M in wg.SIZES}, fx["input_resample"]


def save_npz(path, arrays):
    """np.savez_compressed with fixed member times: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    fresh = "--new-inputs" in sys.argv[1:] or not os.path.exists(wg.FRAMES_NPZ)
    inputs, rs_input = new_inputs() if fresh else committed_inputs()
    for M in wg.SIZES:
        assert inputs[M].shape == (wg.input_len(M), 2) and inputs[M].dtype == np.int8
        assert inputs[M].min() == -128 and inputs[M].max() == 127
    frames = wg.compute_frames(inputs, rs_input)
    wg.assert_frames_consistent(frames)
    frames.update({"input_M%d" % M: inputs[M] for M in wg.SIZES})
    frames["input_resample"] = rs_input
    save_npz(wg.FRAMES_NPZ, frames)
    records = wg.compute_records()
    for name in wg.RECORD_CASES:
        assert len(wg.frozen_records(records, name)) >= 3, name
    save_npz(wg.RECORDS_NPZ, records)
    for path in (wg.FRAMES_NPZ, wg.RECORDS_NPZ):
        assert os.path.getsize(path) <= 1 << 20, (path, os.path.getsize(path))
        print(os.path.relpath(path, ROOT), os.path.getsize(path), "bytes")
    print({k: (v.shape, str(v.dtype)) for k, v in frames.items() if k.startswith(("M128_D96", "resample", "input"))})
    print({name: len(wg.frozen_records(records, name)) for name in wg.RECORD_CASES})


if __name__ == "__main__":
    main()
