"""What tests/test_cpu_wideband_formats.py and tests/test_gpu_wideband_formats.py share: the 8-bit quantisers of the wideband seam's
integer formats and the burst blocks of tests/narrowblock.py behind them, each built once per process and left unchanged."""
import functools

import numpy as np

from gr_amps_amd import capi

import narrowblock as nb

SC8, CU8 = capi.SAMPLES_SC8, capi.SAMPLES_CU8
FORMAT_IDS = {SC8: "sc8", CU8: "cu8"}


def quantise(x, format, full_scale=100.0):
    """complex [n] -> [n, 2] of the format's dtype with the loudest component at `full_scale`: sc8 = rint(v), cu8 = the nearest half-odd
    level (floor(v) + 0.5) plus 127.5.  Both are within half a step of v; nothing clips at a full scale <= 127."""
    peak = max(np.abs(x.real).max(), np.abs(x.imag).max())
    v = np.stack([x.real, x.imag], axis=1).astype(np.float64) * (full_scale / peak)
    if format == SC8:
        q = np.rint(v)
        assert np.abs(q).max() <= 127
        return q.astype(np.int8)
    assert format == CU8
    q = np.floor(v) + 128.0                                   # (floor(v) + 0.5) + 127.5
    assert q.min() >= 0 and q.max() <= 255
    return q.astype(np.uint8)


def silence(n, format):
    """[n, 2] of the format's dtype that converts to (nearly) nothing: sc8 zeros; cu8 has no zero -- the code pairs (127, 128), (128, 127)
    alternating, -+0.5, which is what `recctest wide` appends to a .cu8 file"""
    if format == SC8:
        return np.zeros((n, 2), np.int8)
    q = np.empty((n, 2), np.uint8)
    q[0::2] = (127, 128)
    q[1::2] = (128, 127)
    return q


@functools.lru_cache(maxsize=None)
def burst_block_as(M, D, format, full_scale=100.0):
    """(q [n, 2] in `format`, xf complex64 [n] = capi.convert_samples(q, format), truth) of nb.burst_block(M, D)"""
    x, truth = nb.burst_block(M, D)
    q = quantise(x, format, full_scale)
    xf = capi.convert_samples(q, format)
    q.setflags(write=False)
    xf.setflags(write=False)
    return q, xf, truth
