"""The CPU model of the slicers (oracle.Fused) on degenerate sample values (tests/valuecases.py), no GPU.

  * on the integer-valued classes V1, V2, V4 the model equals the independent float64 statement tests/valueref.py with 0 differing
    bits, taps compared as uint32 (so -0 != +0), for every spec and every supported samples-per-symbol -- which also shows that
    valueref's statements are exact on their stated domain;
  * the kernels' own spec D word logic (exact_slice_word, built for the host behind amps_recc_debug_exact_slice) gives valueref's bits
    on the sign words of those classes;
  * on V3 (zero runs) and V5 (power-of-two scales) the model does not depend on the push schedule, and spec D is the sign of the
    float64 libm boxcar of tests/test_cpu_exact_slicer.py wherever that sum is more than 1e-4 rad from zero."""
import ctypes as C

import numpy as np
import pytest

import oracle
import valuecases as vc
import valueref as vr
from test_cpu_exact_slicer import TOL_RAD, _boxcar_of_libm_atan2

ALL_SPS = [2, 3, 4, 5, 6, 8, 10, 12]
SCHEDULES = [[64], [1, 63, 777, 4096, 10000], [2047, 2049]]       # those of test_cpu_exact_slicer.py


def _model(x, sps, sid, blocks=None):
    f = oracle.Fused(0, sps, slicer=sid)
    recs, off, k = [], 0, 0
    while off < len(x):
        m = len(x) - off if blocks is None else min(blocks[k % len(blocks)], len(x) - off)
        recs.append(f.push(x[off:off + m]))
        off += m
        k += 1
    return f.taps(), np.concatenate(recs)


@pytest.fixture(scope="module")
def exact_rows():
    rows = {(cls, name): row for cls in vc.EXACT_CLASSES for name, row in vc.classes(10)[cls].items()}
    for row in rows.values():
        row.setflags(write=False)
    return rows


def test_the_inputs_are_what_they_claim():
    x = vc.lattice()
    re, im = vr.cosine_product(x, 1), vr.sine_product(x, 1)
    v = x.view(np.float32)
    assert set(np.unique(v)) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    negz = (v == 0) & np.signbit(v)
    assert 0.03 < negz.sum() / (v == 0).sum() < 0.07
    assert 0.03 < (x == 0).mean() < 0.05                              # 1 / 25 of the samples are exactly zero
    assert 0.15 < (im == 0).mean() < 0.30                             # 129 of the 625 value pairs: a fifth of the conj-products have no imaginary part
    assert (np.signbit(im) & (im == 0)).any() and (~np.signbit(im) & (im == 0)).any()
    y = vc.axis_walk()
    re, im = vr.cosine_product(y, 1)[1:], vr.sine_product(y, 1)[1:]
    assert ((re == 0) ^ (im == 0)).all()                              # every step is exactly 0, +-pi/2 or pi
    for sign in (False, True):                                        # atan2(+0, -1) = +pi and atan2(-0, -1) = -pi both occur
        assert ((re < 0) & (im == 0) & (np.signbit(im) == sign)).sum() > 100
    for sps in (3, 10):
        for kw in ({}, {"negative": True}, {"leading": True}):
            z, runs = vc.zero_runs(sps, **kw)
            assert [L for _, L in runs][-15:] == vc.run_lengths(sps)
            for i, (s, L) in enumerate(runs[-15:]):
                size = (vc.LANE, vc.WORD, vc.TILE)[i % 3]
                assert (s + max(1, L // 2)) % size == 0 and s < s + max(1, L // 2) <= s + L      # the boundary lies in or at the end of the run
                assert (z[s:s + L] == 0).all() and z[s - 1] != 0 and z[s + L] != 0
                assert np.signbit(z[s:s + L].view(np.float32)).all() == bool(kw.get("negative"))
            assert (runs[0][0] == 0) == bool(kw.get("leading"))
    for name, row in vc.constants().items():
        assert (vr.sine_product(row, 1) == 0).all() and (vr.sine_product(row, 10) == 0).all(), name
    d = vr.sine_product(vc.constants()["negzero_sines"], 1)
    assert (d == 0).all() and np.signbit(d).all()                     # ... and on this one every sine is -0: spec C's sum is -0, its bit 0
    assert not vr.spec_c(vc.constants()["negzero_sines"], 10)[2][10:].any()
    s = vc.scales(10)
    assert sorted(s) == sorted(vc.SCALES) and np.abs(s[59]).max() < 2.0 ** 60
    tiny = float(np.finfo(np.float32).tiny)
    for k, most in ((-63, 0.9), (-75, 1.0)):                          # the products of two samples are subnormal or zero there
        v = s[k].view(np.float32).astype(np.float64)
        assert (np.abs(v[2:] * v[:-2]) < tiny).mean() >= most and (v * v).max() < 2 * tiny, k
    assert (np.abs(s[-50].view(np.float32).astype(np.float64)) ** 2).max() < 4 * 2.0 ** -100     # ... and at the floor of mx at 2^-50


@pytest.mark.parametrize("sid", [1, 2, 3])
@pytest.mark.parametrize("sps", ALL_SPS)
def test_model_equals_the_float64_statement(exact_rows, sps, sid):
    for key, x in exact_rows.items():
        (d, S, g), _ = _model(x, sps, sid)
        wd, wS, wg = vr.taps32(x, sps, sid)
        assert len(g) == len(x)
        assert int((g != wg).sum()) == 0, (key, np.nonzero(g != wg)[0][:8])
        assert np.array_equal(vr.u32(S), wS), (key, np.nonzero(vr.u32(S) != wS)[0][:8])
        assert np.array_equal(vr.u32(d), wd), (key, np.nonzero(vr.u32(d) != wd)[0][:8])
    # the signed zeros decide bits here: with -0 read as "not negative" the lattice's spec B / C / D bits would differ
    x = exact_rows[("V1", "lattice")]
    d, S, g = vr.SPEC[sid](x, sps)
    z = d if sid == 2 else S                              # spec C: a boxcar sum is -0 only if every term is; its ties are +0
    assert ((z == 0) & np.signbit(z)).sum() > 20 and ((z == 0) & ~np.signbit(z)).sum() > 20
    assert (S == 0).sum() > (20 if sps <= 4 or sid != 2 else 0)


@pytest.mark.parametrize("sps", ALL_SPS)
def test_model_spec_a_on_exact_values(exact_rows, sps):
    for key, x in exact_rows.items():
        (d, S, g), _ = _model(x, sps, 0)
        seen = vr.check_spec_a(x, sps, d, S, g)
        if key[0] == "V2":
            assert seen["plus_pi"] > 100 and seen["minus_pi"] > 100 and seen["minus_zero"] > 100, seen
        if key[0] == "V1":
            assert seen["zero_sample"] > 300, seen


@pytest.mark.parametrize("sps", ALL_SPS)
def test_kernel_word_logic_on_exact_values(exact_rows, sps):
    """exact_slice_word<sps> as the streaming kernel uses it: every 32-sample window, oldest sample at bit 0, bits > sps exact"""
    from gr_amps_amd import capi
    L = capi.load()
    weights = (1 << np.arange(32, dtype=np.uint64))
    for key, x in exact_rows.items():
        x = x[:2048]
        xi = x.view(np.float32)[1::2]
        it, ic, g = vr.spec_d(x, sps)
        signs = [np.signbit(xi), np.signbit(it), np.signbit(ic)]
        out = (C.c_uint32 * 3)()
        for w0 in range(0, len(x) - 32, 32 - sps - 1):                # windows overlap so that every sample is an exact bit of one
            words = (C.c_uint32 * 3)(*[int((s[w0:w0 + 32].astype(np.uint64) * weights).sum()) for s in signs])
            assert L.amps_recc_debug_exact_slice(0, sps, words, out) == 0
            got = (out[0] >> np.arange(32)) & 1
            lo = sps + 1
            assert np.array_equal(got[lo:], g[w0 + lo:w0 + 32]), (key, w0)


V35_SPS = [3, 10]


def _v35_rows(sps):
    rows = {("V3", name): vc.zero_runs(sps, **kw) for name, kw in (("plus", {}), ("minus", {"negative": True}), ("leading", {"leading": True}))}
    rows.update({("V5", k): (row, []) for k, row in vc.scales(sps).items()})
    return rows


@pytest.mark.parametrize("sid", [0, 1, 2, 3])
@pytest.mark.parametrize("sps", V35_SPS)
def test_model_is_push_invariant_on_zero_runs_and_scales(sps, sid):
    for key, (x, _) in _v35_rows(sps).items():
        (d, S, g), recs = _model(x, sps, sid)
        assert len(g) == len(x)
        for blocks in SCHEDULES:
            (d2, S2, g2), recs2 = _model(x, sps, sid, blocks)
            n = len(g2)
            assert n >= len(x) - 64 and np.array_equal(g2, g[:n]), (key, blocks)
            assert np.array_equal(vr.u32(d2), vr.u32(d[:n])) and np.array_equal(vr.u32(S2), vr.u32(S[:n])), (key, blocks)
            assert recs2.tobytes() == recs.tobytes()


@pytest.mark.parametrize("sps", V35_SPS)
def test_spec_d_is_the_sign_of_the_libm_boxcar_on_zero_runs_and_scales(sps):
    """The float64 sum is scale-free; spec D's binary32 products are not once they leave the normal range (k = -75, -63: the
    products are subnormal or zero, and the header's arithmetic -- not libm -- defines the bits there), so the statement is made
    at the scales whose products are normal.  Within sps of a zero run S is exactly 0 and the header's tie rule decides."""
    for key, (x, runs) in _v35_rows(sps).items():
        if key[0] == "V5" and key[1] < -50:
            continue
        g = _model(x, sps, 3)[0][2]
        S = _boxcar_of_libm_atan2(x, sps)
        want = (S >= 0).astype(np.uint8)
        keep = ~vc.near_runs(runs, sps, len(x))
        keep[:sps] = False
        diff = np.nonzero((g != want) & keep)[0]
        assert len(diff) <= 2 and (np.abs(S[diff]) <= TOL_RAD).all(), (key, len(diff), np.abs(S[diff]).max() if len(diff) else 0)
        assert keep.mean() > 0.5
