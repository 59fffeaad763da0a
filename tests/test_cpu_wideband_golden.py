"""The float64 models of the wideband seam held to the committed vectors (tests/golden/wideband_frames.npz, wideband_records.npz;
tests/golden/make_golden_wideband.py writes them, tests/widebandgolden.py holds what is shared), without a GPU:

  1  everything the make script computes, computed again from the committed inputs: bits, masks, records and digests byte for byte,
     rows64, the definition's points and the resampler's float64 output to 1e-10 of the frame norm -- a float64 FFT's own error is of
     order 2^-53 log2 M, the binary32 bound the device gets about 2^-24 log2 M, so 1e-10 is four orders below anything a kernel-scale
     change produces and five above float64 noise.  This is the test that fails when somebody edits a model;
  2  the conditions the reference alone must meet, restated: the definition's double sum, the mask-share cap, the digests of the
     inputs and of the regenerated burst blocks;
  3  the fixture notices: the comparisons of tests/test_gpu_wideband_golden.py fed the float64 model rounded to complex64 pass, and fed
     the same with one thing wrong fail -- the evidence that the frozen vectors would catch a subtly wrong kernel."""
import functools
import hashlib

import numpy as np
import pytest

from oracle import channelizer as cz
from gr_amps_amd import capi

import wbresampleref as wr
import widebandgolden as wg
from test_gpu_wideband_bits import EXPLAINED_FRAC

GEO = pytest.mark.parametrize("M,D", wg.GEOMETRIES, ids=wg.IDS)

INPUT_SHA256 = {
    "input_M1000": "aa6006516787f2eb24196ff737fa9d08a8b51b698b8b1c9ac25f2046d419e763",
    "input_M1024": "ed7aafec1ca7ab272e1cbc3255d49d8d5fa5bc32282f459741f00e3efec18c68",
    "input_M128": "e3f91fbcda10ffb96f69098bbdd5f67404c22c3fac5991445e7c3067933392fc",
    "input_M2000": "af267a9caa01816f30ee221bb1cfaace27a4632fded93eb355c347fd71320676",
    "input_M2500": "2f5c2ba0f6c6ef4209cb051d547ae4aa95ca952233d65a9580461742d2c5fc19",
    "input_M256": "a101ca4f079b6c47976a937ea2b20151c5829acfbda70acbab222d78923013a0",
    "input_M500": "5bebd5166ffd41aa6a5e441877ff35a7bb88141e37c9543e62a3b8f410f8719c",
    "input_M512": "0e4d604b9db8fee407b127e74ca27c7292639cfca7e75ef3e96617ea433fb1d8",
    "input_resample": "c63ab478fc59238fe46e04f9e2c3c693706c84ca213152b9bdbfd5ed8631dde3",
}
BLOCK_SHA256 = {
    "M1024_D768": "127162217a8021043813a3bd15225ffadaf12c4bffc97662629cc53d88c3d08e",
    "M1024_D512": "127162217a8021043813a3bd15225ffadaf12c4bffc97662629cc53d88c3d08e",
    "M512_D256": "4ebf313709e049a4f07247667cb62a973363903093a019d7fe68cd2926d16056",
    "M512_D384": "4ebf313709e049a4f07247667cb62a973363903093a019d7fe68cd2926d16056",
    "M256_D128": "085ed92451a276ee72c2a2d94e19622a94421c82f1b54819d916439376f00994",
    "M256_D192": "085ed92451a276ee72c2a2d94e19622a94421c82f1b54819d916439376f00994",
    "M128_D64": "2058aa4fc1bda2c47178eb0f0d1e8e16d8f99fbf6cb77a51f59f311e2df4539e",
    "M128_D96": "586fcb18466431887003a3e1cbf69bbe0e8bed441914d0ba9ff2c3338a1399bb",
    "M2500_D625": "613d3028645b4de3ea8201f64d22ed964b8cdd66a0005bf16d6786ddbc25cd4e",
    "M2000_D500": "7f6b2046e14fab4940c4987aa42823a29b82cebf2214f3a591de793391553a98",
    "M1000_D250": "0e546eabafbfd79dcd95d10798ffb76466322e2c0e69719b19cd60033a57c50c",
    "M500_D125": "b35a49bd53f0723527534904e66010ca186c761bb0d40ee2222c5470b9fa1e38",
    "M500_D125_cfo1500": "c49989c16fdd90c41197d46b445477e19bee73a9a961f9785460fb80994d7933",
    "M2500_D625_cfo1500": "96e4cd37336351b621625e92cb8184e91c8bc23cce84a80a984eddc53609d7c3",
    "resample_3.2M": "f194b488eccd667ff5063655bdc2967afbfdb046b08150350634930c25cb687f",
}


@functools.lru_cache(maxsize=None)
def _frames():
    fx = wg.load_frames()
    for v in fx.values():
        v.setflags(write=False)
    return fx


@functools.lru_cache(maxsize=None)
def _records():
    return wg.load_records()


@functools.lru_cache(maxsize=None)
def _recomputed():
    fx = _frames()
    return wg.compute_frames({M: fx["input_M%d" % M] for M in wg.SIZES}, fx["input_resample"])


def _input(M):
    return capi.convert_samples(_frames()["input_M%d" % M], wg.SC8)


# ---- 1. models against fixtures
def test_inputs_are_the_committed_ones():
    fx = _frames()
    assert sorted(k for k in fx if k.startswith("input")) == sorted(INPUT_SHA256)
    for k, want in INPUT_SHA256.items():
        assert fx[k].dtype == np.int8 and hashlib.sha256(fx[k].tobytes()).hexdigest() == want, k
    for M in wg.SIZES:
        q = fx["input_M%d" % M]
        assert q.shape == (wg.NFR * wg.d_max(M) + wg.TAIL, 2)
        assert (q[:, 0].min(), q[:, 0].max(), q[:, 1].min(), q[:, 1].max()) == (-128, 127, -128, 127)      # the extreme codes, both components
    assert wr.nout(len(fx["input_resample"]), 6, 5) >= wg.NFR * 96 + wg.TAIL


def test_models_reproduce_the_frame_vectors():
    fx, now = _frames(), _recomputed()
    assert sorted(now) == sorted(k for k in fx if not k.startswith("input"))
    for k, got in now.items():
        want = fx[k]
        assert got.shape == want.shape and got.dtype == want.dtype, k
        if k.endswith(("_bits", "_allowed", "_windows")):
            assert got.tobytes() == want.tobytes(), k                                  # byte for byte
        elif k.startswith("resample_y64"):
            assert np.abs(got - want).max() <= wg.MODEL_TOL * np.abs(fx["resample_y64"]).max(), k
        elif k.endswith(("_rows64", "_definition")):
            norm = fx[k.rsplit("_", 1)[0] + "_norm"]
            scale = norm[None, :] if k.endswith("_rows64") else norm[[m for _, m in wg.DEFINITION_POINTS]]
            assert (np.abs(got - want) <= wg.MODEL_TOL * scale).all(), (k, float((np.abs(got - want) / scale).max()))
        else:                                                                          # norm, weight: real and positive
            assert (np.abs(got - want) <= wg.MODEL_TOL * want).all(), k


@pytest.mark.parametrize("name", wg.RECORD_CASES)
def test_models_reproduce_the_records(name):
    rx = _records()
    case = wg.record_case(name)
    assert wg.block_sha(case["block"]()) == str(rx[name + "_sha256"][0]), "the burst block moved: its generator, not a model"
    got = wg.model_records(name)
    want = wg.frozen_records(rx, name)
    assert len(got) == len(want) == len(case["channels"])
    assert got.tobytes() == want.tobytes()                                             # byte for byte
    assert sorted(int(c) for c in want["channel"]) == sorted(case["channels"]) and want["valid"].all()


# ---- 2. the conditions, restated
def test_reference_meets_its_own_conditions():
    fx, rx = _frames(), _records()
    wg.assert_frames_consistent(fx)
    assert EXPLAINED_FRAC == 1e-3
    for M, D in wg.GEOMETRIES:
        share = wg.mask_shares(fx[wg.key(M, D) + "_allowed"])
        assert share.shape == (4, 8) and share.max() <= EXPLAINED_FRAC, (M, D, share.max())
        bits = np.unpackbits(fx[wg.key(M, D) + "_bits"], axis=-1)
        assert 0.2 < bits[:, :6].mean() < 0.8                                          # keyed rows: ones and zeros
    assert sorted(BLOCK_SHA256) == sorted(wg.RECORD_CASES)
    for name, want in BLOCK_SHA256.items():
        assert str(rx[name + "_sha256"][0]) == want, name


@GEO
def test_definition_points_cover_what_they_claim(M, D):
    """frame 0, a frame inside the history fill, the last frame; bins on both sides of the wrap; and the definition is no restatement of
    the fold: it agrees with rows64 only through the mathematics"""
    L = wg.taps(M, D).size
    frames = [m for _, m in wg.DEFINITION_POINTS]
    assert 0 in frames and wg.NFR - 1 in frames and any(0 < (m + 1) * D < L for m in frames) and len(wg.DEFINITION_POINTS) == 16
    bins = wg.row_bins(M, wg.frozen_rows(M))
    first = wg.band(M)[0]
    assert {bool(bins[r] >= first) for r, _ in wg.DEFINITION_POINTS} == {True, False}
    pts = _frames()[wg.key(M, D) + "_definition"]
    assert np.abs(pts).min() > 0


# ---- 3. the fixture notices
def _rounded(M, D, **kw):
    return wg.model_frames(_input(M), M, D, wg.frozen_rows(M), **kw)[0].astype(np.complex64)


@GEO
def test_the_rounded_model_passes(M, D):
    fx = _frames()
    k = wg.key(M, D)
    worst = wg.check_rows(_rounded(M, D), fx, k, M)
    assert worst < 0.2                                       # binary32 rounding of a value is 2^-24 of it: far inside FFT_C log2(M) of the frame norm
    rows64 = fx[k + "_rows64"]
    bits = np.array([[wg.sb.float64_bits(y, wg.sps_of(M, D), s) for y in rows64] for s in range(4)], np.uint8)
    assert wg.check_bits(bits, fx, k) == 0
    if (M, D) in wg.SHIFTED:
        assert wg.check_rows(_rounded(M, D, shift_hz=wg.SHIFT_HZ), fx, wg.key(M, D, True), M) < 0.2
        with pytest.raises(AssertionError):                  # the shift does something
            wg.check_rows(_rounded(M, D), fx, wg.key(M, D, True), M)


def test_bank_model_is_the_oracles_and_the_prototype_is_symmetric():
    """wg.bank_model with no knob turned is oracle.channelizer.channelize to the last bit.  The prototypes are exactly symmetric, so
    `taps reversed` is no wrong model: it cannot fail and is not in wg.wrong_models."""
    for M, D in ((128, 96), (500, 125)):
        h = wg.taps(M, D)
        x = _input(M)[:40 * D]
        assert np.array_equal(wg.bank_model(x, h, M, D), cz.channelize(x, P=h.size // M, M=M, D=D, taps=h))
    for M, D in wg.GEOMETRIES:
        h = wg.taps(M, D)
        assert np.array_equal(h, h[::-1]), (M, D)
        assert "reversed" not in wg.wrong_models(M, D)


@pytest.mark.parametrize("what", ["cutoff", "roll", "bin", "frame_phase", "conj", "stride"])
def test_a_wrong_bank_model_fails_the_comparison(what):
    """cut-off 15 -> 14.5 kHz (13 -> 12.5 behind D = M / 2), the roll by n0 + 1, row c read from bin first + stride c + 1, the roll of the
    frame before, the conjugate, and on the 10 kHz grid stride 1: each fails check_rows, on every geometry it applies to"""
    fx = _frames()
    caught, applies = [], []
    for (M, D), gid in zip(wg.GEOMETRIES, wg.IDS):
        wrong = wg.wrong_models(M, D)
        if what not in wrong:
            continue
        h, knobs, bin_off, stride = wrong[what]
        applies.append(gid)
        got = _rounded(M, D, h=h, bin_off=bin_off, stride=stride, **knobs)
        try:
            wg.check_rows(got, fx, wg.key(M, D), M)
        except AssertionError:
            caught.append(gid)
    assert applies == (wg.IDS[-4:] if what == "stride" else wg.IDS)
    assert caught == applies, sorted(set(applies) - set(caught))


def test_a_wrong_resampler_phase_fails_the_comparison():
    """phase p + 1 for p in the resampler, and then the bank's rows behind it"""
    fx = _frames()
    rate, L, Mr, M, D = wg.RESAMPLE
    x = capi.convert_samples(fx["input_resample"], wg.SC8)
    g = wg.rs_prototype()
    y = wr.upfirdn(x, g, L, Mr)
    extra = wg.resample_rows_extra(fx)
    h = wr.BURSTS["3.2M"].bank_taps()
    assert wg.check_resample(y.astype(np.complex64), fx) < 0.1
    assert wg.check_rows(wg.model_frames(y, M, D, wg.RS_ROWS, first=wg.RS_FIRST, h=h)[0].astype(np.complex64), fx, "resample", M, extra) < 0.1
    # the wrong resampler, by the definition's sum with the phase off by one, at every output
    bad = wg.rs_definition(x, g, L, Mr, range(len(y)), phase_off=1)
    with pytest.raises(AssertionError):
        wg.check_resample(bad.astype(np.complex64), fx)
    with pytest.raises(AssertionError):
        wg.check_rows(wg.model_frames(bad, M, D, wg.RS_ROWS, first=wg.RS_FIRST, h=h)[0].astype(np.complex64), fx, "resample", M, extra)
    # the extra term is small beside the rows it guards: a wrong model is of the order of the rows themselves
    assert extra < 1e-3 * np.abs(fx["resample_rows64"][:6, 64:]).mean()


def test_a_flipped_bit_and_a_moved_record_fail_the_comparison():
    fx, rx = _frames(), _records()
    k = wg.key(500, 125)
    bits = np.unpackbits(fx[k + "_bits"], axis=-1)
    assert wg.check_bits(bits, fx, k) == 0
    bits[2, 3, 77] ^= 1
    with pytest.raises(AssertionError):
        wg.check_bits(bits, fx, k)
    name = "M500_D125_cfo1500"
    rec = wg.frozen_records(rx, name).copy()
    assert wg.check_records(rec, rx, name, 2) == [0] * 6
    rec["position"][2] += 1                                   # another sampling phase of the same symbol
    assert wg.check_records(rec, rx, name, 2) == [0, 0, 1, 0, 0, 0]
    rec["position"][2] += 1                                   # the next symbol
    with pytest.raises(AssertionError):
        wg.check_records(rec, rx, name, 2)
    rec = wg.frozen_records(rx, name).copy()
    rec["word_raw"][4, 1, 7] ^= 1
    with pytest.raises(AssertionError):
        wg.check_records(rec, rx, name, 2)
    with pytest.raises(AssertionError):
        wg.check_records(wg.frozen_records(rx, name)[:5], rx, name, 2)
