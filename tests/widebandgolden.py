"""What tests/golden/make_golden_wideband.py, tests/test_cpu_wideband_golden.py and tests/test_gpu_wideband_golden.py share: the twelve
geometries of the wideband seam's filter banks with the band, rows and taps the frozen vectors use, the float64 side of
tests/golden/wideband_frames.npz and tests/golden/wideband_records.npz (models and the definition's own double sum), and the
comparisons that hold a device, or a wrong model, to the committed values.  Nothing here regenerates an input: the sc8 inputs are read
from the fixture, and the burst blocks are the ones the suite already builds, pinned by their SHA-256."""
import functools
import hashlib
import os

import numpy as np

import oracle
from oracle import channelizer as cz
from gr_amps_amd import capi, synth_wideband as sw

import grid10block as gb
import narrowblock as nb
import shiftblock as shb
import slicerbound as sb
import wbresampleref as wr
from test_gpu_wideband_bits import EXPLAINED_FRAC

HERE = os.path.dirname(os.path.abspath(__file__))
FRAMES_NPZ = os.path.join(HERE, "golden", "wideband_frames.npz")
RECORDS_NPZ = os.path.join(HERE, "golden", "wideband_records.npz")

NFR = 128                      # frames frozen per geometry
TAIL = 37                      # samples behind the last whole frame at the larger decimation
SC8 = capi.SAMPLES_SC8
SPECS = ("atan", "product", "sine", "exact")          # slicer specs A, B, C, D = 0 .. 3
MODEL_TOL = 1e-10              # float64 model against committed value, in units of the frame norm (far above 2^-53 log2 M, far below 2^-24)
SHIFT_HZ = 6543.21             # the shift of tests/test_gpu_wideband_shift.py

# ---- the geometries
WIDE = [(1024, 768), (1024, 512)]
GEOMETRIES = WIDE + list(nb.GEOMETRIES) + [(M, gb.decim(M)) for M in gb.SIZES]
IDS = ["M%d-D%d" % g for g in GEOMETRIES]
SIZES = sorted({M for M, _ in GEOMETRIES}, reverse=True)                  # the eight bank sizes: one committed input each
SHIFTED = [(128, 96), (500, 125)]                                         # one two-kernel geometry per family carries a shifted variant
RESAMPLE = (3.2e6, 6, 5, 128, 96)                                         # rate, L, M, bank, decimation of the resampled path


def key(M, D, shifted=False):
    return "M%d_D%d%s" % (M, D, "_shift" if shifted else "")


def grid(M):
    return M in gb.SIZES


def bank(M):
    """(bin width, bins from one row to the next, taps per branch)"""
    return wr.BANKS[M][:3]


def fs_of(M):
    return M * bank(M)[0]


def d_max(M):
    return max(D for m, D in GEOMETRIES if m == M)


def input_len(M):
    return NFR * d_max(M) + TAIL


def sps_of(M, D):
    return 2 if grid(M) else 3 * M // (2 * D)


def taps(M, D):
    if grid(M):
        return gb.taps(M)
    return cz.design_taps(8, 1024, cz.cutoff_for_decim(D)) if M == 1024 else nb.taps(M, D)


def band(M):
    """(first bin, channels) of the handle the frame vectors are made for: the first bin is M - 8, so the rows wrap past bin M - 1"""
    return M - 8, (832 if M == 1024 else M // bank(M)[1])


def row_bins(M, rows, first=None):
    first = band(M)[0] if first is None else first
    return (first + bank(M)[1] * np.asarray(rows)) % M


def keyed_rows(M):
    C = band(M)[1]
    return [0, 1, C // 2 - 1, C // 2, C - 1, C // 4]


def frozen_rows(M):
    """the six keyed rows, then the two noise-only rows on either side of the wrap: the last row before bin M - 1 is passed and the first behind it"""
    first, C = band(M)
    w = -(-(M - first) // bank(M)[1])
    rows = keyed_rows(M) + [w - 1, w]
    assert len(set(rows)) == 8 and row_bins(M, w - 1) > row_bins(M, w) and max(rows) < C
    return rows


# (index into frozen_rows, frame): frame 0, frames inside the history fill (11 frames at the least), the last frame; rows 0, 1 and the
# seventh lie before the wrap, the others behind it
DEFINITION_POINTS = [(0, 0), (7, 0), (6, 0), (2, 0), (1, 5), (3, 5), (6, 7), (7, 3),
                     (0, 127), (7, 127), (4, 127), (5, 127), (2, 64), (3, 65), (4, 31), (5, 100)]


# ---- the resampled path
RS_ROWS = list(wr.BURSTS["3.2M"].rows) + [20, 100]       # the six rows of the suite's 3.2 Msps block keyed, two noise-only ones
RS_FIRST = 0
RS_WINDOWS = (0, wr.TILE - 32, None)                       # first outputs of the three frozen windows of 64; None = the last 64


def rs_input_len():
    rate, L, Mr, M, D = RESAMPLE
    want = NFR * D + TAIL
    n = -(-want * Mr // L)
    assert wr.nout(n, L, Mr) >= want
    return n


def rs_windows(nout):
    return [nout - 64 if w is None else w for w in RS_WINDOWS]


def rs_prototype():
    rate, L, Mr, M, D = RESAMPLE
    return wr.prototype64(rate, L, M)


def rs_definition(x, g, L, Mr, ks, phase_off=0):
    """y[k] = sum_i g[L i + p] x[q - i], k Mr = L q + p, the double sum written out at the outputs ks; phase_off = 1 is the wrong model
    that takes phase p + 1 for p"""
    x = np.asarray(x, np.complex128)
    out = np.zeros(len(ks), np.complex128)
    for j, k in enumerate(ks):
        q, p = divmod(int(k) * Mr, L)
        p = (p + phase_off) % L
        for i in range(-(-len(g) // L)):
            if L * i + p < len(g) and 0 <= q - i < len(x):
                out[j] += g[L * i + p] * x[q - i]
    return out


# ---- the bank: the model, the definition, and the model with one thing wrong
def definition_point(x, h, M, D, k, m):
    """y[k][m] = sum_{i < L} h[i] x[n0 + i] exp(-2 pi i k (n0 + i) / M), n0 = (m + 1) D - L, x = 0 before the stream: the double sum,
    the phase reduced in integers; no fold, no FFT"""
    h = np.asarray(h, np.float64)
    L = h.size
    n0 = (m + 1) * D - L
    i = np.arange(max(0, -n0), L)
    n = n0 + i
    ph = (int(k) * n) % M
    return np.sum(h[i] * np.asarray(x, np.complex128)[n] * np.exp(-2j * np.pi * ph / M))


def bank_model(x, h, M, D, roll_off=0, frame_phase=0, conj=False):
    """oracle.channelizer.channelize restated with the knobs the wrong models turn: roll_off is added to the roll, frame_phase to the
    frame whose n0 sets the roll; all M bins, complex128 [M][frames].  With no knob turned it is cz.channelize."""
    h = np.asarray(h, np.float64)
    L = h.size
    x = np.asarray(x, np.complex128)
    nfr = x.size // D
    xp = np.concatenate([np.zeros(L - D, np.complex128), x[:nfr * D]])
    out = np.empty((nfr, M), np.complex128)
    for m in range(nfr):
        seg = xp[m * D:m * D + L] * h
        n0 = (m + 1 + frame_phase) * D - L
        out[m] = np.fft.fft(np.roll(seg.reshape(-1, M).sum(0), (n0 + roll_off) % M))
    out = np.ascontiguousarray(out.T)
    return np.conj(out) if conj else out


def wrong_models(M, D):
    """name -> (taps, keyword arguments of bank_model, offset added to every row's bin, stride) of the model with one thing wrong"""
    bin_hz, stride, P = bank(M)
    h = taps(M, D)
    cut = 13e3 if (not grid(M) and 2 * D == M) else 15e3
    out = {"cutoff": (cz.design_taps(P, M, cut - 0.5e3, chan_hz=bin_hz), {}, 0, stride),
           "roll": (h, {"roll_off": 1}, 0, stride),
           "bin": (h, {}, 1, stride),
           "frame_phase": (h, {"frame_phase": -1}, 0, stride),
           "conj": (h, {"conj": True}, 0, stride)}
    if grid(M):
        out["stride"] = (h, {}, 0, 1)
    return out


def model_frames(x, M, D, rows, first=None, shift_hz=None, h=None, bin_off=0, stride=None, **knobs):
    """(rows64 complex128 [R][NFR], norm float64 [NFR]) of the float64 bank on x (complex, from sample 0)"""
    h = taps(M, D) if h is None else h
    if shift_hz is not None:
        x = shb.mix64(x, shb.step_of(shift_hz, fs_of(M)))
    full = bank_model(x, h, M, D, **knobs) if knobs else cz.channelize(x, P=h.size // M, M=M, D=D, taps=h)
    first = band(M)[0] if first is None else first
    bins = (first + (bank(M)[1] if stride is None else stride) * np.asarray(rows) + bin_off) % M
    return np.ascontiguousarray(full[bins, :NFR]), np.sqrt((np.abs(full[:, :NFR]) ** 2).sum(0))


def eps_of(M, norm):
    """the project's own bound on what a row of the device may differ by: FFT_C 2^-24 log2(M) max over the frames of ||Y64(frame)||"""
    return sb.FFT_C * sb.U32 * np.log2(M) * float(np.max(norm))


def start_allowed(y64, eps, sps, spec):
    """bool [sps]: slicerbound.allowed restated for the frames before the first full window, n < sps.  There sb.allowed lets the zeros
    before the stream move like any sample (delta = pi for them, |S| = 0 <= anything at n = 0), which marks the first sps positions of
    specs A and C as free on every row whatever the input.  But those zeros are exact on the device too: the step (spec A) or product
    (spec C) against them is exactly 0, so S[0] = 0 and the bit 1 with no freedom, and S[n], 0 < n < sps, is the sum of the steps or
    products k = 1 .. n alone, each of which moves by what sb.allowed gives a step between two real samples.  A subset of sb.allowed."""
    y = np.asarray(y64[:sps], np.complex128)
    a = np.abs(y)
    S = sb.statistic(y, sps, spec)
    ok = np.zeros(sps, bool)
    if spec in (1, 3):
        return ok                                                  # defined as ones
    for n in range(1, sps):
        k = np.arange(1, n + 1)
        if spec == 0:
            delta = np.where(a > eps, np.arcsin(np.minimum(eps / np.maximum(a, 1e-300), 1.0)), np.pi)
            r = delta[k] + delta[k - 1]
            step = np.angle(y[k] * np.conj(y[k - 1]))
            ok[n] = abs(S[n]) <= r.sum() + sb.TOL_RAD + sps * sb.ATAN_STEP_RAD or bool((np.pi - np.abs(step) <= r + sb.TOL_RAD).any())
        else:
            per = eps * (a[k] + a[k - 1]) + eps * eps + 4.0 * sb.U32 * (a[k] + eps) * (a[k - 1] + eps)
            ok[n] = abs(S[n]) <= per.sum()
    return ok


def model_bits(rows64, eps, sps):
    """(bits, allowed), both packed uint8 [4][R][NFR / 8]: slicerbound's float64 statement and where a binary32 slicer may leave it
    (sb.allowed; before the first full window start_allowed, its restatement without freedom for the zeros before the stream)"""
    bits = np.array([[sb.float64_bits(y, sps, s) for y in rows64] for s in range(4)], np.uint8)
    ok = np.array([[sb.allowed(y, eps, sps, s) for y in rows64] for s in range(4)], bool)
    for s in range(4):
        for r, y in enumerate(rows64):
            first = start_allowed(y, eps, sps, s)
            assert not (first & ~ok[s, r, :sps]).any()
            ok[s, r, :sps] = first
    return np.packbits(bits, axis=-1), np.packbits(ok, axis=-1)


def mask_shares(allowed_packed):
    """float [4][R]: the share of positions of each row and spec where a difference would count as explained"""
    return np.unpackbits(allowed_packed, axis=-1).mean(axis=-1)


def compute_frames(inputs, rs_input):
    """everything tests/golden/wideband_frames.npz holds beside the inputs, from the inputs: {name: array}"""
    out = {}
    for M, D in GEOMETRIES:
        x = capi.convert_samples(inputs[M], SC8)
        rows = frozen_rows(M)
        for shifted in ([False, True] if (M, D) in SHIFTED else [False]):
            k = key(M, D, shifted)
            h = taps(M, D)
            rows64, norm = model_frames(x, M, D, rows, shift_hz=SHIFT_HZ if shifted else None)
            xm = shb.mix64(x, shb.step_of(SHIFT_HZ, fs_of(M))) if shifted else x
            out[k + "_rows64"], out[k + "_norm"] = rows64, norm
            out[k + "_definition"] = np.array([definition_point(xm, h, M, D, row_bins(M, rows[r]), m) for r, m in DEFINITION_POINTS])
            if shifted:
                out[k + "_weight"] = shb.frame_weights(x, h, D)[:NFR]
            else:
                out[k + "_bits"], out[k + "_allowed"] = model_bits(rows64, eps_of(M, norm), sps_of(M, D))
    rate, L, Mr, M, D = RESAMPLE
    x = capi.convert_samples(rs_input, SC8)
    g = rs_prototype()
    y = wr.upfirdn(x, g, L, Mr)
    wins = rs_windows(len(y))
    out["resample_windows"] = np.array(wins)
    out["resample_y64"] = np.stack([y[w:w + 64] for w in wins])
    out["resample_y64_definition"] = np.stack([rs_definition(x, g, L, Mr, range(w, w + 64)) for w in wins])
    h = wr.BURSTS["3.2M"].bank_taps()
    rows64, norm = model_frames(y, M, D, RS_ROWS, first=RS_FIRST, h=h)
    out["resample_rows64"], out["resample_norm"] = rows64, norm
    out["resample_definition"] = np.array([definition_point(y, h, M, D, row_bins(M, RS_ROWS[r], RS_FIRST), m) for r, m in DEFINITION_POINTS])
    return out


def assert_frames_consistent(fx):
    """what the reference alone must meet: rows64 equal the definition's points, the resampler's float64 output its own double sum, and
    no row's mask exceeds the cap"""
    names = [key(M, D, s) for M, D in GEOMETRIES for s in ([False, True] if (M, D) in SHIFTED else [False])] + ["resample"]
    for k in names:
        rows64, norm, pts = fx[k + "_rows64"], fx[k + "_norm"], fx[k + "_definition"]
        for (r, m), want in zip(DEFINITION_POINTS, pts):
            assert abs(rows64[r, m] - want) <= MODEL_TOL * norm[m], (k, r, m, abs(rows64[r, m] - want) / norm[m])
        if k + "_allowed" in fx:
            share = mask_shares(fx[k + "_allowed"])
            assert share.max() <= EXPLAINED_FRAC, (k, np.argwhere(share > EXPLAINED_FRAC).tolist(), share.max())
    d = np.abs(fx["resample_y64"] - fx["resample_y64_definition"]).max()
    assert d <= MODEL_TOL * np.abs(fx["resample_y64"]).max(), d


# ---- the burst blocks and their records
RECORD_FIELDS = ("channel", "msg_class", "min", "esn", "dialed", "valid", "word_raw", "word_dec")
SMOKE_FIRST, SMOKE_C = 96, 832
SMOKE_PLANTED = [(SMOKE_FIRST + 5, 120000), (SMOKE_FIRST + 400, 90000), (SMOKE_FIRST + 831, 200000)]
RECORD_CASES = (["M1024_D768", "M1024_D512"] + [key(M, D) for M, D in nb.GEOMETRIES] + [key(M, gb.decim(M)) for M in gb.SIZES]
                + ["M500_D125_cfo1500", "M2500_D625_cfo1500", "resample_3.2M"])


@functools.lru_cache(maxsize=None)
def _smoke_block():
    n = int(0.25 * sw.FS_WIDE) // 1536 * 1536
    x, truth = sw.make_wideband(n, SMOKE_PLANTED, seed=7)
    x.setflags(write=False)
    return x


def record_case(name):
    """dict(M, D, sps, first, C, channels: the handle's row of each model row, resample, block(): complex64 [n], rows(): the float64
    bank's rows of the planted channels as complex64)"""
    if name.startswith("resample"):
        b = wr.BURSTS["3.2M"]
        def rows():
            x = wr.burst_block("3.2M")[0]
            y = wr.upfirdn(x, wr.prototype64(b.rate, b.L, b.channels), b.L, b.M)
            chan = cz.channelize(y, P=b.P, M=b.channels, D=b.decim, taps=b.bank_taps())
            return np.ascontiguousarray(chan[[b.row_bin(r) for r in b.rows]]).astype(np.complex64)
        return dict(M=b.channels, D=b.decim, sps=2, first=b.first, C=b.C, channels=list(b.rows), resample=(b.rate, b.L, b.M),
                    block=lambda: wr.burst_block("3.2M")[0], rows=rows)
    M, D = (int(s[1:]) for s in name.split("_")[:2])
    cfo = 1500.0 if name.endswith("cfo1500") else 0.0
    if M == 1024:
        def rows():
            chan = cz.channelize(_smoke_block(), P=8, D=D)
            return chan[[k for k, _ in SMOKE_PLANTED]].astype(np.complex64)
        return dict(M=M, D=D, sps=1536 // D, first=SMOKE_FIRST, C=SMOKE_C, channels=[k - SMOKE_FIRST for k, _ in SMOKE_PLANTED], resample=None,
                    block=_smoke_block, rows=rows)
    if grid(M):
        return dict(M=M, D=D, sps=2, first=gb.FIRST, C=gb.max_channels(M), channels=[r for r, _ in gb.planted(M)], resample=None,
                    block=lambda: gb.burst_block(M, cfo)[0], rows=lambda: gb.model_rows(M, cfo).astype(np.complex64))
    return dict(M=M, D=D, sps=nb.sps_of(M, D), first=0, C=M, channels=[k for k, _ in nb.planted(M)], resample=None,
                block=lambda: nb.burst_block(M, D)[0], rows=lambda: nb.model_rows(M, D))


def block_sha(x):
    assert x.dtype == np.complex64
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


def model_records(name):
    """oracle.fused_push_all on the float64 bank's rows, the channel of every record the handle's row"""
    case = record_case(name)
    rec = oracle.fused_push_all(case["rows"](), sps=case["sps"])
    rec["channel"] = np.array(case["channels"], np.uint32)[rec["channel"]]
    return rec[np.lexsort((rec["position"], rec["channel"]))]


def compute_records():
    out = {}
    for name in RECORD_CASES:
        out[name + "_sha256"] = np.array([block_sha(record_case(name)["block"]())])
        out[name + "_records"] = np.ascontiguousarray(model_records(name)).view(np.uint8).reshape(-1, oracle.BURST_DTYPE.itemsize)
    return out


def frozen_records(fx, name):
    return np.ascontiguousarray(fx[name + "_records"]).view(oracle.BURST_DTYPE).reshape(-1)


# ---- the comparisons: what the GPU test holds the device to, and the CPU test a wrong model
def load_frames():
    with np.load(FRAMES_NPZ) as f:
        return {k: f[k] for k in f.files}


def load_records():
    with np.load(RECORDS_NPZ) as f:
        return {k: f[k] for k in f.files}


def rows_bound(fx, k, M, extra=0.0):
    """float64 [NFR]: FFT_C 2^-24 log2(M) ||Y64(frame)||_2, on a shifted variant plus DELTA sum |h| |x| of the frame, plus `extra`"""
    b = sb.FFT_C * sb.U32 * np.log2(M) * fx[k + "_norm"]
    if k + "_weight" in fx:
        b = b + shb.DELTA * fx[k + "_weight"]
    return b + extra


def check_rows(got, fx, k, M, extra=0.0):
    """got: complex64 [8][NFR], the frozen rows as the device (or a model) gives them.  Returns the worst |got - rows64| / bound."""
    got = np.asarray(got)
    assert got.dtype == np.complex64 and got.shape == fx[k + "_rows64"].shape, (got.dtype, got.shape)
    assert np.isfinite(got.view(np.float32)).all()
    ratio = np.abs(got.astype(np.complex128) - fx[k + "_rows64"]) / rows_bound(fx, k, M, extra)[None, :]
    assert ratio.max() <= 1.0, (k, float(ratio.max()), np.unravel_index(np.argmax(ratio), ratio.shape))
    return float(ratio.max())


def check_bits(got, fx, k):
    """got: uint8 [4][8][NFR], the slicer bits of the frozen rows under specs A .. D.  Outside the frozen mask no bit may differ; inside
    it at most EXPLAINED_FRAC of all bits.  Returns the number that differ inside."""
    got = np.asarray(got, np.uint8)
    want = np.unpackbits(fx[k + "_bits"], axis=-1)
    ok = np.unpackbits(fx[k + "_allowed"], axis=-1).astype(bool)
    assert got.shape == want.shape, got.shape
    diff = got != want
    assert not (diff & ~ok).any(), (k, np.argwhere(diff & ~ok)[:8].tolist())
    inside = int((diff & ok).sum())
    assert inside <= EXPLAINED_FRAC * got.size, (k, inside)
    return inside


def resample_bound():
    """per component, what tests/test_gpu_wideband_resample.py::test_tap_meets_float64 holds the tap to, at an sc8 block's largest value"""
    rate, L, Mr, M, D = RESAMPLE
    return wr.bound(rs_prototype(), L, 128.0)


def check_resample(y, fx):
    """y: complex64, the device's (or a model's) resampler output of the committed input.  Returns the worst error / bound per component."""
    y = np.asarray(y)
    assert y.dtype == np.complex64
    worst = 0.0
    for w, want in zip(fx["resample_windows"], fx["resample_y64"]):
        got = y[w:w + 64].astype(np.complex128)
        assert got.shape == want.shape, (w, got.shape)
        worst = max(worst, np.abs(got.real - want.real).max(), np.abs(got.imag - want.imag).max())
    assert worst <= resample_bound(), (worst, resample_bound())
    return worst / resample_bound()


def resample_rows_extra(fx):
    """what the resampler's error can add to a bin, and to the FFT bound through the frame norm (test_gpu_wideband_golden.py derives it)"""
    rate, L, Mr, M, D = RESAMPLE
    e = np.sqrt(2.0) * resample_bound() * np.abs(wr.BURSTS["3.2M"].bank_taps()).sum()
    return e + sb.FFT_C * sb.U32 * np.log2(M) * np.sqrt(M) * e


def check_records(got, fx, name, sps):
    """got: the device's records, sorted by (channel, position).  Returns the position differences (device - frozen)."""
    want = frozen_records(fx, name)
    assert len(got) == len(want), (name, len(got), len(want))
    for f in RECORD_FIELDS:
        assert np.array_equal(got[f], want[f]), (name, f)
    dpos = got["position"].astype(np.int64) - want["position"].astype(np.int64)
    assert (np.abs(dpos) < sps).all(), (name, dpos.tolist())
    return dpos.tolist()
