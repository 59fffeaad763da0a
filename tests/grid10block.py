"""What tests/test_cpu_grid10_bank.py and tests/test_gpu_grid10_bank.py share: the four sizes of the filter banks of 10 kHz bins (M = 2500,
2000, 1000, 500 branches at D = M / 4: 25, 20, 10 and 5 Msps), their prototype, the burst block both decode, the tone block of the
per-bin error test with its float64 rows, and a complex64 statement of the kernel's pass order -- each built once per process."""
import functools

import numpy as np

from oracle import channelizer as cz
from gr_amps_amd import synth_wideband as sw

SIZES = (2500, 2000, 1000, 500)
IDS = ["M%d" % M for M in SIZES]
P, BIN_HZ, STRIDE, SPS = 3, 10e3, 3, 2
FIRST = 7                     # first bin of the burst block's band: rows are bins (7 + 3 c) % M
RADICES = {2500: (5, 5, 5, 5, 4), 2000: (5, 5, 5, 16), 1000: (5, 5, 5, 8), 500: (5, 5, 5, 4)}   # the passes as the kernel runs them


def decim(M):
    return M // 4


def max_channels(M):
    return M // STRIDE


def taps(M):
    """the prototype the library designs: Kaiser beta = 8 sinc at fs = M * 10 kHz, -6 dB at 15 kHz, three taps per branch"""
    return cz.design_taps(P, M, 15e3, chan_hz=BIN_HZ)


def row_bins(M, first, C):
    return (first + STRIDE * np.arange(C)) % M


def planted(M):
    """(row, sample offset): rows 0 and 1 keyed at overlapping times, a third neighbour, both sides of +- fs / 2, the band's last row"""
    C = max_channels(M)
    return [(0, 3000), (1, 9000), (2, 20000), (C // 2 - 1, 5000), (C // 2, 7000), (C - 1, 11000)]


@functools.lru_cache(maxsize=None)
def burst_block(M, cfo_hz=0.0, first=FIRST):
    """(complex64 [n], truth keyed by (row, offset)): one burst in each of six channels of a band at fs = M * 10 kHz, 20 dB; the band's
    first bin is `first`"""
    fs, D, C = M * BIN_HZ, decim(M), max_channels(M)
    n = int(3500 * fs / 20e3 + 40000) // D * D
    bins = row_bins(M, first, C)
    x, truth = sw.make_wideband(n, [(int(bins[r]), off) for r, off in planted(M)], seed=11 + M, snr_db=20.0, fs=fs, cfo_hz=cfo_hz, bins=M)
    x.setflags(write=False)
    return x, {(r, off): truth[(int(bins[r]), off)] for r, off in planted(M)}


@functools.lru_cache(maxsize=None)
def model_rows(M, cfo_hz=0.0):
    """the float64 model's channel-rate rows of the six planted channels, complex128 [6][frames], in the order of planted(M)"""
    x, _ = burst_block(M, cfo_hz)
    bins = row_bins(M, FIRST, max_channels(M))
    chan = cz.channelize(x, M=M, D=decim(M), taps=taps(M))
    rows = np.ascontiguousarray(chan[[int(bins[r]) for r, _ in planted(M)]])
    rows.setflags(write=False)
    return rows


# ---- the per-bin error test's input
TONE_AMPS = (1.0, 0.8, 0.6, 0.9, 0.7)


def tone_rows(M):
    C = max_channels(M)
    return (0, 1, C // 2 - 1, C // 2, C - 1)


@functools.lru_cache(maxsize=None)
def tone_block(M):
    """about 300 frames: noise at 0.02 plus tones 3 kHz above the centres of the bins of rows 0, 1, C / 2 - 1, C / 2 and C - 1 of a band
    whose first bin is M - 8, so that the rows wrap past bin M - 1"""
    fs, D, C = M * BIN_HZ, decim(M), max_channels(M)
    bins = row_bins(M, M - 8, C)
    rng = np.random.default_rng(23 + M)
    n = 300 * D + 37
    t = np.arange(n)
    x = 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    for r, a in zip(tone_rows(M), TONE_AMPS):
        x += a * np.exp(2j * np.pi * (sw.bin_freq(int(bins[r]), fs, M) + 3e3) * t / fs)
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def tone_model(M):
    """float64: every bin of every frame of tone_block(M), complex128 [M][frames]"""
    y = cz.channelize(tone_block(M), M=M, D=decim(M), taps=taps(M))
    y.setflags(write=False)
    return y


# ---- the kernel's arithmetic in complex64: the fold as a multiply and two multiply-adds per branch, then the Stockham passes of
# RADICES[M] with the butterflies of recc_chz_narrow.hip.h (chz_dft) and a float32 twiddle table rounded from double
def twiddles32(M):
    w = np.exp(-2j * np.pi * np.arange(M) / M).astype(np.complex64)
    w[0], w[M // 4], w[M // 2], w[3 * M // 4] = 1, -1j, -1, 1j
    return w


def _mi(a):
    return (a.imag - 1j * a.real).astype(np.complex64)        # a * (-i)


def _dft4(a0, a1, a2, a3):
    v0, v1, v2, d = a0 + a2, a0 - a2, a1 + a3, a1 - a3
    return [v0 + v2, v1 + _mi(d), v0 - v2, v1 - _mi(d)]


def _dft5(v):
    c1, c2, s1, s2 = (np.float32(c) for c in (0.30901699437494742, -0.80901699437494742, 0.95105651629515357, 0.58778525229247313))
    t1, t2, t3, t4 = v[1] + v[4], v[2] + v[3], v[1] - v[4], v[2] - v[3]
    m1, m2 = v[0] + c1 * t1 + c2 * t2, v[0] + c2 * t1 + c1 * t2
    n1, n2 = s1 * t3 + s2 * t4, s2 * t3 - s1 * t4
    return [v[0] + t1 + t2, m1 + _mi(n1), m2 + _mi(n2), m2 - _mi(n2), m1 - _mi(n1)]


def _dft8(v):
    r2 = np.float32(0.70710678118654752)
    e, o = _dft4(v[0], v[2], v[4], v[6]), _dft4(v[1], v[3], v[5], v[7])
    o[1] = o[1] * np.complex64(r2 - 1j * r2)
    o[2] = _mi(o[2])
    o[3] = o[3] * np.complex64(-r2 - 1j * r2)
    return [e[k] + o[k] for k in range(4)] + [e[k] - o[k] for k in range(4)]


def _dft16(u):
    w16 = np.exp(-2j * np.pi * np.arange(16) / 16).astype(np.complex64)
    v = [_dft4(u[b], u[4 + b], u[8 + b], u[12 + b]) for b in range(4)]
    for b in range(1, 4):
        for c in range(1, 4):
            v[b][c] = _mi(v[b][c]) if b * c == 4 else v[b][c] * w16[b * c]
    out = [None] * 16
    for c in range(4):
        X = _dft4(v[0][c], v[1][c], v[2][c], v[3][c])
        for d in range(4):
            out[c + 4 * d] = X[d]
    return out


_DFT = {4: lambda v: _dft4(*v), 5: _dft5, 8: _dft8, 16: _dft16}


def bank_c64(x, M):
    """complex64 [M][frames]: the bank of M branches on x (from sample 0), operation by operation in binary32 in the kernel's order"""
    D, L = decim(M), P * M
    h = taps(M).astype(np.float32)
    x = np.asarray(x, np.complex64)
    nfr = x.size // D
    xp = np.concatenate([np.zeros(L - D, np.complex64), x[:nfr * D]])
    idx = np.arange(nfr)[:, None] * D + np.arange(M)[None, :]
    acc = xp[idx] * h[:M]
    for p in range(1, P):
        acc = (acc + xp[idx + p * M] * h[p * M:(p + 1) * M]).astype(np.complex64)
    u = np.empty_like(acc)
    for f in range(nfr):
        u[f] = np.roll(acc[f], ((f + 1) * D) % M)
    tw, NS = twiddles32(M), 1
    for R in RADICES[M]:
        BPF = M // R
        j = np.arange(BPF)
        k = j % NS
        v = [u[:, j + r * BPF] for r in range(R)]
        if NS > 1:
            v = [v[0]] + [(v[r] * tw[r * k * (M // (NS * R))]).astype(np.complex64) for r in range(1, R)]
        X = _DFT[R](v)
        j0 = (j // NS) * NS * R + k
        out = np.empty_like(u)
        for r in range(R):
            out[:, j0 + r * NS] = X[r]
        u, NS = out, NS * R
    assert NS == M and u.dtype == np.complex64
    return np.ascontiguousarray(u.T)
