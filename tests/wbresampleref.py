"""What tests/test_cpu_wideband_resample.py and tests/test_gpu_wideband_resample.py share: the wideband seam's L / M resampler
(include/amps_recc.h, amps_recc_set_wideband_resample) in float64 -- the default filter, the prototype, scipy's upfirdn cut to the
definition's output count, the definition's own double sum -- and the two burst blocks both decode, each built once per process."""
import functools

import numpy as np
import scipy.signal

import oracle
from oracle import channelizer as cz
from gr_amps_amd import synth_wideband as sw

import xlateresampleref as rr

# the bank sizes: branches -> (bin width, bins from one channel to the next, taps per branch, decimations in table order)
BANKS = {1024: (30e3, 1, 8, (768, 512)), 512: (30e3, 1, 8, (384, 256)), 256: (30e3, 1, 8, (192, 128)), 128: (30e3, 1, 8, (96, 64)),
         2500: (10e3, 3, 3, (625,)), 2000: (10e3, 3, 3, (500,)), 1000: (10e3, 3, 3, (250,)), 500: (10e3, 3, 3, (125,))}
# (rate, L, M, target bank): the six ratios of the tap tests
RATIOS = [(4e6, 5, 4, 500), (3.2e6, 6, 5, 128), (2.4e6, 8, 5, 128), (2.5e6, 2, 1, 500), (7.68e6, 1, 2, 128), (3e6, 5, 3, 500)]
RATIO_IDS = ["%gM_%d_%d" % (r / 1e6, L, M) for r, L, M, _ in RATIOS]
TILE = 1024                    # outputs of one workgroup of wb_resample_kernel


def bank_rate(channels):
    return channels * BANKS[channels][0]


def nout(n, L, M):
    """outputs delivered after n inputs: ceil(L n / M)"""
    return -(-L * n // M)


def default_filter(rate, channels):
    """(cutoff_hz, width_hz) the configuration fills in for zeros: width = f_low / 16, cutoff = f_low / 2 - width / 2"""
    f_low = min(rate, bank_rate(channels))
    width = f_low / 16.0
    return 0.5 * f_low - 0.5 * width, width


def prototype_ntaps(rate, L, width):
    n = int(74.0 * L * rate / (22.0 * width))
    return n + 1 - (n & 1)


def prototype64(rate, L, channels, cutoff=0.0, width=0.0):
    """g = firdes.low_pass(L, L rate, cutoff, width) (Blackman) in float64, never rounded"""
    dc, dw = default_filter(rate, channels)
    cutoff, width = cutoff or dc, width or dw
    fs = L * rate
    n = prototype_ntaps(rate, L, width)
    i = np.arange(n, dtype=np.float64)
    k = i - (n - 1) // 2
    win = 0.42 - 0.5 * np.cos(2.0 * np.pi * i / (n - 1)) + 0.08 * np.cos(4.0 * np.pi * i / (n - 1))
    w0 = 2.0 * np.pi * cutoff / fs
    with np.errstate(invalid="ignore", divide="ignore"):
        t = np.where(k == 0, w0 / np.pi, np.sin(k * w0) / (k * np.pi)) * win
    return t * L / t.sum()


def prototype32(rate, L, channels, cutoff=0.0, width=0.0):
    """the same through the oracle's firdes.low_pass, rounded to float32 as the library rounds its own: what the kernel holds"""
    dc, dw = default_filter(rate, channels)
    return oracle.firdes_low_pass(float(L), L * rate, cutoff or dc, width or dw)


def ntp_of(g, L):
    return rr.phases(np.asarray(g, np.float64), L).shape[1]


def upfirdn(x, g, L, M):
    """float64: scipy's polyphase resampler cut to the ceil(L N / M) outputs the definition delivers"""
    y = scipy.signal.upfirdn(np.asarray(g, np.float64), np.asarray(x, np.complex128), up=L, down=M)
    return y[:nout(len(x), L, M)]


def definition(x, g, L, M):
    """float64: y[k] = sum_i h_p[i] x[q - i] with k M = L q + p, written out"""
    g = np.asarray(g, np.float64)
    x = np.asarray(x, np.complex128)
    y = np.zeros(nout(len(x), L, M), np.complex128)
    for k in range(len(y)):
        q, p = divmod(k * M, L)
        for i in range(-(-len(g) // L)):
            if L * i + p < len(g) and 0 <= q - i < len(x):
                y[k] += g[L * i + p] * x[q - i]
    return y


def bound(g, L, xmax):
    """per component: (ntp + 2) 2^-24 max_p sum_i |h_p[i]| max|x| -- one rounding of each tap and ntp fma roundings of a real dot product
    whose partial sums are bounded by sum |h| |x|"""
    h = rr.phases(np.asarray(g, np.float64), L)
    return (h.shape[1] + 2) * 2.0 ** -24 * np.abs(h).sum(axis=1).max() * xmax


def ragged(n, seed):
    """n cut into ragged pieces, a piece of one sample and one of two among them"""
    rng = np.random.default_rng(seed)
    cuts, left = [1, 2], n - 3
    while left > 0:
        m = int(min(left, rng.integers(1, max(2, n // 3))))
        cuts.append(m)
        left -= m
    assert sum(cuts) == n and all(c > 0 for c in cuts)
    return cuts


# ---- the two burst blocks: six bursts at 20 dB each, channels out to the edge of the band the default filter keeps flat
class Burst:
    def __init__(self, rate, L, M, channels, decim, first, rows, seed):
        self.rate, self.L, self.M, self.channels, self.decim, self.first, self.rows, self.seed = rate, L, M, channels, decim, first, rows, seed
        self.bin_hz, self.stride, self.P, _ = BANKS[channels]
        self.C = channels // self.stride                   # the band's channels: row r is bin (first + stride r) % channels
        self.offsets = (3000, 9000, 20000, 5000, 7000, 11000)

    def row_bin(self, r):
        return (self.first + self.stride * r) % self.channels

    def row_hz(self, r):
        return sw.bin_freq(self.row_bin(r), bank_rate(self.channels), self.channels)

    def bank_taps(self):
        return cz.design_taps(self.P, self.channels, 15e3, chan_hz=self.bin_hz)      # two samples per symbol: -6 dB at 15 kHz


BURSTS = {"4M": Burst(4e6, 5, 4, 500, 125, 7, (0, 1, 56, 110, 120, 165), 41),
          "3.2M": Burst(3.2e6, 6, 5, 128, 96, 0, (0, 1, 40, 46, 82, 127), 32)}
# the 4 Msps block once more with its band from bin 0, where the command-line tool's band starts (tests/test_gpu_wideband_resample_tools.py)
TOOL_BURSTS = {"4M@0": Burst(4e6, 5, 4, 500, 125, 0, (0, 1, 56, 110, 120, 165), 43)}


@functools.lru_cache(maxsize=None)
def burst_block(name):
    """(complex64 [n] at the delivered rate, truth keyed by row): the delivered band has rate / 10 kHz bins, and a channel sits where it
    sits in hertz"""
    b = BURSTS.get(name) or TOOL_BURSTS[name]
    bins = int(round(b.rate / 10e3))
    n = int(3500 * b.rate / 20e3 + 40000)
    planted = []
    for r, off in zip(b.rows, b.offsets):
        k = int(round(b.row_hz(r) / 10e3))
        assert abs(k * 10e3 - b.row_hz(r)) < 1e-6 and abs(b.row_hz(r)) <= 0.5 * b.rate * (1 - 1 / 8.0)
        planted.append((k % bins, off))
    x, truth = sw.make_wideband(n, planted, seed=b.seed, snr_db=20.0, fs=b.rate, bins=bins)
    x.setflags(write=False)
    return x, {r: truth[p] for r, p in zip(b.rows, planted)}


@functools.lru_cache(maxsize=None)
def burst_model(name):
    """the float64 chain's records of the six rows: upfirdn -> oracle.channelizer.channelize -> oracle.fused_push_all(sps = 2); the
    record's channel is the index into the burst's rows"""
    b = BURSTS[name]
    x, _ = burst_block(name)
    y = upfirdn(x, prototype64(b.rate, b.L, b.channels), b.L, b.M)
    chan = cz.channelize(y, P=b.P, M=b.channels, D=b.decim, taps=b.bank_taps())
    rows = np.ascontiguousarray(chan[[b.row_bin(r) for r in b.rows]]).astype(np.complex64)
    return oracle.fused_push_all(rows, sps=2)
