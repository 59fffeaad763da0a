"""What tests/test_cpu_narrow_bank.py and tests/test_gpu_narrow_bank.py share: the six geometries of the narrow filter banks (M = 512,
256, 128 branches at D = M / 2 and 3 M / 4), their prototype, and the burst block both decode -- each built once per process."""
import functools

import numpy as np

from oracle import channelizer as cz
from gr_amps_amd import synth_wideband as sw

GEOMETRIES = [(M, D) for M in (512, 256, 128) for D in (M // 2, 3 * M // 4)]
IDS = ["M%d-D%d" % g for g in GEOMETRIES]


def sps_of(M, D):
    return 3 * M // (2 * D)


def taps(M, D):
    """the prototype the library designs: Kaiser beta = 8 sinc, -6 dB at 13 kHz behind D = M / 2, at 15 kHz behind D = 3 M / 4"""
    return cz.design_taps(8, M, 13e3 if 2 * D == M else 15e3)


def planted(M):
    """(bin, sample offset): both band edges, both sides of +- fs / 2, and two neighbours"""
    return [(0, 3000), (1, 9000), (M // 2 - 1, 5000), (M // 2, 7000), (M - 1, 11000), (5, 20000)]


@functools.lru_cache(maxsize=None)
def burst_block(M, D, cfo_hz=0.0):
    """(complex64 [n], truth): one burst in each of six channels of a band of M bins at fs = M * 30 kHz, 20 dB"""
    fs = M * 30e3
    n = int(3500 * fs / 20e3 + 40000) // D * D
    x, truth = sw.make_wideband(n, planted(M), seed=7 + M, snr_db=20.0, fs=fs, cfo_hz=cfo_hz, bins=M)
    x.setflags(write=False)
    return x, truth


@functools.lru_cache(maxsize=None)
def model_rows(M, D):
    """the float64 model's channel-rate rows of the six planted bins, as complex64 [6][frames], in the order of planted(M)"""
    x, _ = burst_block(M, D)
    chan = cz.channelize(x, P=8, M=M, D=D, taps=taps(M, D))
    rows = chan[[k for k, _ in planted(M)]].astype(np.complex64)
    rows.setflags(write=False)
    return rows
