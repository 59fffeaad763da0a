"""-m gpu: the wideband seam held to committed vectors (tests/golden/wideband_frames.npz, wideband_records.npz) -- every filter bank in
every geometry, the shifted banks, the resampled path, and whole bursts.  The expected values were computed once on the CPU in float64
(tests/golden/make_golden_wideband.py), part of them by the definition's double sum and not by fold and FFT, and
tests/test_cpu_wideband_golden.py keeps the models on them: a model and its kernel cannot drift together.  The comparisons are those of
tests/widebandgolden.py, which the CPU test shows to fail on a model with one thing wrong.  Every case is one handle or a few and one
or two pushes."""
import numpy as np
import pytest

import slicerbound as sb
from oracle import channelizer as cz
from gr_amps_amd import capi

import wbresampleref as wr
import widebandgolden as wg

pytestmark = pytest.mark.gpu
GEO = pytest.mark.parametrize("M,D", wg.GEOMETRIES, ids=wg.IDS)
SC8 = capi.SAMPLES_SC8
MAX_FRAMES = 192 + 64 + 72                       # the input is 192 frames at D = M / 2; a flush of 64 more; what the handle holds back

_cache = {}


def _frames():
    if "frames" not in _cache:
        _cache["frames"] = wg.load_frames()
    return _cache["frames"]


def _records():
    if "records" not in _cache:
        _cache["records"] = wg.load_records()
    return _cache["records"]


def _handle(M, D, C, first, max_frames=MAX_FRAMES, resample=None, **kw):
    wb = {"channels": M, "decim": D, "first_channel": first}
    if resample:
        wb["resample"] = resample
    return capi.Recc(n_channels=C, max_samples=max_frames, max_bursts=64, wideband=wb, **kw)


def _bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _both_taps(r, q):
    """the bank's rows of the sc8 block read in place and of its fc32 conversion: bit-identical, every value finite"""
    a = r.debug_channelize_as(q, SC8)
    r.reset()
    b = r.debug_channelize(capi.convert_samples(q, SC8))
    assert a.shape == b.shape and a.shape[1] >= wg.NFR and np.array_equal(_bits32(a), _bits32(b))
    assert np.isfinite(a.view(np.float32)).all()
    return a


# ---- 1. rows
@GEO
def test_rows_meet_the_frozen_float64_rows(gpu, M, D):
    """|y32 - rows64| <= FFT_C 2^-24 log2(M) norm[frame] on the eight frozen rows of all 128 frames, the bound of the banks' own per-bin
    tests with the frozen norm; on the shifted variants plus DELTA x the frozen weight, as tests/test_gpu_wideband_shift.py states it.
    Measured worst fractions of the bound (profiles/wideband_golden/golden.txt): 1024: 0.187 (D = 768), 0.198 (512); 512: 0.268 (256),
    0.235 (384); 256: 0.285, 0.305; 128: 0.377, 0.341; 2500: 0.124, 2000: 0.109, 1000: 0.133, 500: 0.161; shifted 128 / 96: 0.117,
    500: 0.103.  The float64 model rounded to complex64 reads 0.2 at the most, a model with one thing wrong far above 1
    (tests/test_cpu_wideband_golden.py)."""
    fx = _frames()
    q = fx["input_M%d" % M]
    first, C = wg.band(M)
    rows = wg.frozen_rows(M)
    with _handle(M, D, C, first) as r:
        assert r.sps == wg.sps_of(M, D)
        got = _both_taps(r, q)
        assert got.shape[0] == C
        worst = wg.check_rows(got[rows, :wg.NFR], fx, wg.key(M, D), M)
        print(f"\nM={M} D={D}: worst |y32 - rows64| / bound = {worst:.3f}")
        if (M, D) in wg.SHIFTED:
            r.reset()
            r.set_wideband_shift(wg.SHIFT_HZ)
            shifted = _both_taps(r, q)
            worst = wg.check_rows(shifted[rows, :wg.NFR], fx, wg.key(M, D, True), M)
            print(f"M={M} D={D} shifted by {wg.SHIFT_HZ:+.2f} Hz: worst |y32 - rows64| / bound = {worst:.3f}")
            assert not np.array_equal(_bits32(shifted), _bits32(got))


# ---- 2. bits
@GEO
def test_slicer_bits_are_the_frozen_bits(gpu, M, D):
    """the input, then 64 D zeros; the bits of the frozen rows under all four specs against the frozen float64 bits: none differs
    outside the frozen mask, at most EXPLAINED_FRAC of all bits inside it.  The mask is the committed one, made before any device
    existed from the project's own bound on the bank's error; it is never recomputed from what the device gave.  On the 1024 bank the
    fused form, and the two-kernel form (AMPS_RECC_FLAG_UNFUSED_WIDEBAND) too.  Measured: no bit differs anywhere, in any geometry
    or form (no position of the committed masks is set on these rows, so none could)."""
    fx = _frames()
    q = fx["input_M%d" % M]
    first, C = wg.band(M)
    rows = wg.frozen_rows(M)
    flush = np.zeros((64 * D, 2), np.int8)
    for form in ([{}, {"unfused_wideband": True}] if M == 1024 else [{}]):
        got = []
        for spec in wg.SPECS:
            with _handle(M, D, C, first, slicer=spec, **form) as r:
                r.push_wideband_as(q, SC8)
                r.push_wideband_as(flush, SC8)
                bits, produced = r.debug_slicer_bits(0, wg.NFR)
            assert produced == ((len(q) + len(flush)) // D) & ~63 and bits.shape == (C, wg.NFR)
            got.append(bits[rows])
        got = np.array(got)
        inside = wg.check_bits(got, fx, wg.key(M, D))
        print(f"\nM={M} D={D} {'two-kernel' if form else 'default'} form: {inside} of {got.size} bits differ inside the frozen mask, none outside")


# ---- 3. the resampled path
def test_resampler_and_the_bank_behind_it(gpu):
    """3.2 Msps x 6/5 into M = 128, D = 96.  The tap (debug_wideband_resample) on the three frozen windows, per component within the
    bound of test_gpu_wideband_resample.py::test_tap_meets_float64 (wbresampleref.bound), b.

    The bank behind it against the frozen rows of the float64 chain.  The device's bank reads y32 = y64 + d with |d[n]| <= sqrt(2) b.
    The bank is linear: bin k of frame m of the float64 bank moves by sum_i h[i] d[n0 + i] e^{...}, at most e = sqrt(2) b sum |h|.  The
    device's bank is within FFT_C 2^-24 log2(M) ||Y(y32)(m)|| of the float64 bank on y32, and ||Y(y32)(m)|| <= ||Y64(m)|| + sqrt(M) e.
    So |y32 - rows64| <= FFT_C 2^-24 log2(M) norm[m] + e (1 + FFT_C 2^-24 log2(M) sqrt(M)) (widebandgolden.resample_rows_extra).
    That derivation is sound but not tight: b is a worst case over 56 taps at full scale, and e comes to about a hundred times the FFT
    term (the CPU test shows it is still a thousand times below the rows, so a wrong index fails it).  The case is therefore ALSO held
    to the unshifted bound on the resampler's own device output: the device's rows against the float64 bank on
    debug_wideband_resample's samples, every row and frame, with no extra term.  Measured: the tap 0.023 of b, the rows 0.0021 of the
    derived bound and 0.316 of the unshifted one."""
    fx = _frames()
    rate, L, Mr, M, D = wg.RESAMPLE
    q = fx["input_resample"]
    b = wr.BURSTS["3.2M"]
    with _handle(M, D, b.C, wg.RS_FIRST, resample=(rate, L, Mr)) as r:
        y = r.debug_wideband_resample(q, SC8)
        assert y.shape == (wr.nout(len(q), L, Mr),)
        ratio = wg.check_resample(y, fx)
        r.reset()
        got = _both_taps(r, q)
    assert got.shape == (b.C, wg.NFR)
    worst = wg.check_rows(got[wg.RS_ROWS], fx, "resample", M, wg.resample_rows_extra(fx))
    want = cz.channelize(y, P=b.P, M=M, D=D, taps=b.bank_taps())[:, :wg.NFR]
    unit = sb.U32 * np.log2(M) * np.sqrt((np.abs(want) ** 2).sum(0))
    bins = [b.row_bin(c) for c in range(b.C)]
    own = (np.abs(got - want[bins]) / (sb.FFT_C * unit)).max()
    print(f"\nresampler: worst error / bound per component = {ratio:.3f}; rows against the frozen chain / derived bound = {worst:.4f}; "
          f"rows against the float64 bank on the tap's own output / unshifted bound = {own:.3f}")
    assert own <= 1.0, own


# ---- 4. records
@pytest.mark.parametrize("name", wg.RECORD_CASES)
def test_records_are_the_frozen_records(gpu, name):
    """the suite's burst block, regenerated and held to its committed SHA-256 first; pushed in two uneven pieces and the flush; the
    records' identity fields equal the frozen ones of the float64 chain exactly, their number too, and every position lies fewer than
    sps channel-rate samples from the frozen one: the same symbol, whichever of the sps sampling phases either side took.  Measured:
    every position of all fifteen blocks equals the frozen one."""
    rx = _records()
    case = wg.record_case(name)
    x = case["block"]()
    assert wg.block_sha(x) == str(rx[name + "_sha256"][0]), "the burst block moved: its generator, not a kernel"
    M, D, sps = case["M"], case["D"], case["sps"]
    n = len(x)
    cut = (n // 3) // D * D + 100
    flush = np.zeros(80 * D, np.complex64)
    bank_samples = (lambda m: m) if not case["resample"] else (lambda m: wr.nout(m, case["resample"][1], case["resample"][2]))
    with _handle(M, D, case["C"], case["first"], max_frames=bank_samples(n + len(flush)) // D + 72, resample=case["resample"]) as r:
        assert r.sps == sps
        for piece in (x[:cut], x[cut:], flush):
            r.push_wideband(piece)
        got = r.drain()
    dpos = wg.check_records(got, rx, name, sps)
    print(f"\n{name}: {len(got)} records, positions device - frozen = {dpos}")
