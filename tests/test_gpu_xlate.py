"""Translate seam: the channel filter of grc/recctest.grc -- freq_xlating_fir_filter_ccc with the
firdes.low_pass taps (grc/recctest.grc:889-937, :115-155) -- on the GPU, in front of the fused IQ seam, so that the
flow graph's 400 ksps ".raw" captures can be pushed as they are.

Float stage: compared with the oracle's restatement of the GNU Radio block (composite complex taps + rotator, fp32) and
with the exact formula in float64, tolerance stated below.  Downstream of it the comparison is word-level and bit-exact."""
import errno

import numpy as np
import pytest

import oracle
from gr_amps_amd import capi, synth

pytestmark = pytest.mark.gpu

# |y_gpu - y_exact| for unit-amplitude input through taps of DC gain 3: the kernel mixes in fp32 (phase exact to 2^-24
# turn) and accumulates 299 fp32 fma; the oracle's composite-tap/rotator arithmetic differs from the exact result by
# about as much.  Both bounds are absolute, on samples of magnitude <= 3.
TOL_EXACT = 2.0e-5
TOL_ORACLE = 6.0e-5


def _raw400(seed, n=2 * 400000, nb=12, fc=160e3):
    iq400, truth = synth.make_channel_block(n, nb, seed=seed, sps=20, spacing=(3456 + 74 + 4096 + 600) * 20)
    k = np.arange(iq400.size)
    return (iq400 * np.exp(2j * np.pi * fc * k / 400e3)).astype(np.complex64), truth


def _exact(x, taps, fc, fs, decim):
    n = np.arange(x.size)
    z = x.astype(np.complex128) * np.exp(-2j * np.pi * fc * n / fs)
    full = np.convolve(z, np.asarray(taps, np.float64))[: x.size]
    return full[::decim][: x.size // decim]


@pytest.mark.parametrize("fc", [160e3, -160e3, 37.5e3])
def test_xlate_matches_reference_block(gpu, fc):
    rng = np.random.default_rng(7)
    n = 50000
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64) * np.float32(0.5)
    taps = oracle.firdes_low_pass(3, 400e3, 10e3, 4.5e3)
    assert len(taps) == 299
    with capi.Recc(n_channels=1, sps=10, max_samples=n, max_bursts=4) as r:
        r.set_xlate(rate_hz=400e3, center_hz=fc, decim=2)
        y = r.debug_xlate(x[None, :])[0]
    assert y.size == n // 2
    e = _exact(x, taps, fc, 400e3, 2)
    assert np.abs(y - e).max() <= TOL_EXACT, np.abs(y - e).max()
    ref = oracle.freq_xlating_fir(x, taps, fc, 400e3, 2)
    assert np.abs(y - ref).max() <= TOL_ORACLE, np.abs(y - ref).max()


@pytest.mark.parametrize("decim,sps", [(1, 10), (4, 5)])
def test_xlate_other_decimations(gpu, decim, sps):
    rng = np.random.default_rng(8)
    n = 30001
    fs = 20e3 * sps * decim
    x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    with capi.Recc(n_channels=2, sps=sps, max_samples=n, max_bursts=4) as r:
        r.set_xlate(rate_hz=fs, center_hz=0.11 * fs, decim=decim, gain=1.0, cutoff_hz=12e3, width_hz=6e3)
        y = r.debug_xlate(np.stack([x, x[::-1]]))
    taps = oracle.firdes_low_pass(1.0, fs, 12e3, 6e3)
    assert np.abs(y[0] - _exact(x, taps, 0.11 * fs, fs, decim)).max() <= TOL_EXACT
    assert np.abs(y[1] - _exact(x[::-1], taps, 0.11 * fs, fs, decim)).max() <= TOL_EXACT


@pytest.mark.parametrize("nch", [1, 3])
@pytest.mark.parametrize("blocks", [[1, 2, 3, 298, 299, 300, 4097], [2047, 2049, 1, 1, 1], [7777] * 5])
def test_xlate_streaming_is_bitwise(gpu, blocks, nch):
    """Pushing in ragged blocks (odd sizes leave a sample waiting for the decimator) gives the same bits as one push:
    the mixer phase is a function of the absolute sample index, the carry holds the filter history.  With three rows of
    different noise every row keeps a carry of its own: each equals what a one-channel handle makes of that row alone."""
    n = sum(blocks)
    x = np.stack([np.random.default_rng(9 + c).standard_normal((2, n)) for c in range(nch)])
    x = (x[:, 0] + 1j * x[:, 1]).astype(np.complex64)
    with capi.Recc(n_channels=nch, sps=10, max_samples=n, max_bursts=4) as r:
        r.set_xlate(rate_hz=400e3, center_hz=-160e3, decim=2)
        whole = r.debug_xlate(x)
        r.reset()
        parts, o = [], 0
        for b in blocks:
            parts.append(r.debug_xlate(x[:, o:o + b]))
            o += b
    got = np.concatenate(parts, axis=1)
    assert got.shape == whole.shape == (nch, n // 2)
    assert np.array_equal(got.view(np.uint32), whole.view(np.uint32))
    for c in range(nch) if nch > 1 else ():
        with capi.Recc(n_channels=1, sps=10, max_samples=n, max_bursts=4) as r:
            r.set_xlate(rate_hz=400e3, center_hz=-160e3, decim=2)
            alone = r.debug_xlate(x[c:c + 1])[0]
        assert np.array_equal(whole[c].view(np.uint32), alone.view(np.uint32)), c


def test_raw400_words_equal_reference_cpu_chain(gpu):
    """The whole recctest.grc chain from the 400 ksps capture: oracle = restated G1..G4 + R2..R8 (chain_iq400); product =
    push_raw (GPU channel filter + fused seam).  The two channel filters agree to ~1e-5, the words must agree exactly."""
    n_ref = n_gpu = 0
    for seed in range(3):
        iq400, truth = _raw400(700 + seed)
        ref = oracle.chain_iq400(iq400, 160e3, chunk=4096)
        with capi.Recc(n_channels=1, sps=10, max_samples=iq400.size // 2, max_bursts=64) as r:
            r.set_xlate(rate_hz=400e3, center_hz=160e3, decim=2)
            for part in np.array_split(iq400, 5):          # ragged pushes
                r.push_raw(part[None, :])
            got = r.drain()
        assert len(got) == len(truth)
        by_min = {g["min"]: g for g in got}
        for rr in ref:
            assert rr["min"] in by_min, "reference decoded a burst the GPU path missed"
            g = by_min[rr["min"]]
            assert np.array_equal(rr["word_raw"], g["word_raw"])
            assert np.array_equal(rr["word_dec"], g["word_dec"])
            assert np.array_equal(rr["valid"], g["valid"]) and np.array_equal(rr["dcc"], g["dcc"])
            for f in ("msg_class", "a_MIN1", "b_MIN2", "esn", "dialed", "min"):
                assert rr[f] == g[f], f
        n_ref += len(ref)
        n_gpu += len(got)
    # The restated chain's Mueller & Mueller loop has to lock inside the four dotting bits the precursor has to spare: at 30 dB it
    # decodes ~99.8 % of the bursts (scripts/slicer_sensitivity.py, 1000 bursts per point); every one of them was compared above.
    print("reference chain decoded %d of the %d bursts the GPU path decoded" % (n_ref, n_gpu))
    assert n_ref >= n_gpu - 1, (n_ref, n_gpu)


def test_xlate_argument_errors(gpu):
    with capi.Recc(n_channels=1, sps=10, max_samples=4096, max_bursts=4) as r:
        with pytest.raises(capi.AmpsError):
            r.push_raw(np.zeros((1, 16), np.complex64))                  # stage not configured
        with pytest.raises(capi.AmpsError):
            r.set_xlate(rate_hz=400e3, center_hz=160e3, decim=4)         # 100 ksps != 10 samples/symbol
        with pytest.raises(capi.AmpsError):
            r.set_xlate(rate_hz=400e3, center_hz=160e3, decim=3)
        with pytest.raises(capi.AmpsError) as e:
            r.set_xlate(rate_hz=400e3, center_hz=float("nan"), decim=2)  # a centre that is no number
        assert e.value.code == -errno.EINVAL
        r.set_xlate(rate_hz=400e3, center_hz=160e3, decim=2)
        with pytest.raises(capi.AmpsError):
            r.push_raw(np.zeros((1, 2 * 4096 + 2), np.complex64))        # more than decim * max_samples


def test_a_wider_channel_filter_keeps_mobiles_that_are_off_their_carrier(gpu):
    """VERDICT r05 item 8 (carrier offset on the IQ seam): a mobile 2 kHz off its carrier loses half its bursts at 12 dB C/N behind the
    flow graph's channel filter -- cut-off 10 kHz, grc/recctest.grc:115-155: it cuts into a signal it no longer centres; the restated
    reference chain loses four fifths there -- and none behind a 14 kHz filter of the same length on the same seam
    (amps_recc_xlate_cfg_t.cutoff_hz; 500 bursts per point: profiles/r06/cfo_filter_width.txt).  Without an offset the two filters
    decode the same bursts."""
    nb, n400 = 96, 80000
    snr400 = 12.0 - 10.0 * np.log10(400.0 / 30.0)

    def blocks(cfo):
        raw, truth = [], []
        for i in range(nb):
            x, t = synth.make_channel_block(n400, 1, seed=881000 + i, sps=20, snr_db=snr400, first=4000, cfo_hz=cfo)
            raw.append((x * np.exp(2j * np.pi * 0.4 * np.arange(x.size))).astype(np.complex64))
            truth.append((t[0][2], [bytes(np.asarray(w, np.uint8)) for w in t[0][5]]))
        return np.stack(raw), truth

    def good(raw, truth, cutoff):
        with capi.Recc(n_channels=nb, sps=10, max_samples=n400 // 2 + 64, max_bursts=4 * nb) as r:
            r.set_xlate(rate_hz=400e3, center_hz=160e3, decim=2, cutoff_hz=cutoff)
            r.push_raw(raw)
            r.push_raw(np.zeros((nb, 2048), np.complex64))
            recs = r.drain()
        ok = set()
        for g in recs:
            min10, sent = truth[int(g["channel"])]
            if g["min"].decode() == min10 and all(bool(g["valid"][w]) and bytes(g["word_dec"][w]) == sent[w] for w in range(len(sent))):
                ok.add(int(g["channel"]))
        return len(ok)

    raw, truth = blocks(2000.0)
    narrow, wide = good(raw, truth, 0.0), good(raw, truth, 14e3)
    print("2 kHz off the carrier at 12 dB: %d of %d bursts behind the 10 kHz filter, %d behind the 14 kHz one" % (narrow, nb, wide))
    assert wide >= nb - 2 and narrow <= (3 * nb) // 4
    raw, truth = blocks(0.0)
    narrow0, wide0 = good(raw, truth, 0.0), good(raw, truth, 14e3)
    assert narrow0 >= nb - 1 and wide0 >= nb - 1
