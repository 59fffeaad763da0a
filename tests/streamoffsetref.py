"""float64 model of the IQ and translate seams' carrier-offset measurement (include/amps_recc.h: AMPS_RECC_FLAG_STREAM_OFFSET) -- TEST
INFRASTRUCTURE ONLY.

Block j of a row is A[j] = 2^-8 * sum of y[s] conj(y[s - 1]) over the channel-rate samples s in [256 j, 256 j + 256), s absolute
(origin counted), with a ZERO in front of the stream's first sample.  A record's burst sum is the sum of the blocks that lie wholly
inside its capture [position, position + 3374 * sps) -- the blocks of burst power (streampowerref.burst_window) -- and its offset is
the sum's argument times fs / 2 pi, fs = 20000 * sps."""
import math

import numpy as np

from streampowerref import CAPTURE_SYMS, STRIDE, burst_window, first_block  # noqa: F401  (one window arithmetic for both models)


def _products(y):
    y = np.atleast_2d(np.asarray(y)).astype(np.complex128)
    prev = np.concatenate([np.zeros((y.shape[0], 1), np.complex128), y[:, :-1]], axis=1)   # y[origin - 1] = 0
    return y, prev


def _fold(p, origin):
    j0 = first_block(origin)
    skip = j0 * STRIDE - int(origin)                                 # samples in front of the first whole block
    nblk = max(0, (p.shape[1] - skip) // STRIDE)
    return p[:, skip:skip + nblk * STRIDE].reshape(p.shape[0], nblk, STRIDE).mean(axis=2)


def blocks(y, origin=0):
    """y: complex [rows][n] (or [n]) channel-rate stream from its first sample, which is absolute sample `origin`.  Returns complex128
    [rows][nblk]: column i is block j = first_block(origin) + i, for every block that lies wholly inside the n samples."""
    y, prev = _products(y)
    return _fold(y * np.conj(prev), origin)


def weights(y, origin=0):
    """2^-8 * sum |y[s]| |y[s - 1]| of the same blocks: what the fp32 error bound of a block is relative to (the terms cancel)"""
    y, prev = _products(y)
    return _fold(np.abs(y) * np.abs(prev), origin)


def burst_sum(row, pos, sps, first=0):
    """row: one channel's blocks, row[i] = block first + i.  Returns (complex sum, count) over the capture's blocks; (0j, 0) when one
    of them is not in row."""
    j0, cnt = burst_window(pos, sps)
    if j0 < first or j0 - first + cnt > len(row):
        return 0j, 0
    return complex(np.sum(np.asarray(row, np.complex128)[j0 - first:j0 - first + cnt])), cnt


def offset_hz(total, sps):
    """the argument of a (block or burst) sum as a frequency: atan2(im, re) * fs / 2 pi, fs = 20000 * sps; 0.0 for a zero sum"""
    total = complex(total)
    if total == 0:
        return 0.0
    return math.atan2(total.imag, total.real) * (20000.0 * sps) / (2.0 * math.pi)


def burst_offset_hz(row, pos, sps, first=0):
    """(offset in Hz, count) of a record's capture; (0.0, 0) when a block is not in row"""
    total, cnt = burst_sum(row, pos, sps, first=first)
    return (offset_hz(total, sps) if cnt else 0.0), cnt


def gather_sum(entries):
    """the burst sum of amps_recc_burst_autocorr restated in numpy float32: `entries` are the complex64 ring values A[j0] ... A[j0 + count
    - 1] of one row; each component alone, lane l adds 0 + e[l] + e[l + 64] + ... ascending, then the butterfly o = 32 ... 1; no
    division.  IEEE addition is what it is, so this reproduces the gather kernel bit for bit."""
    e = np.ascontiguousarray(entries, np.complex64).reshape(-1)
    out = []
    for comp in (e.real, e.imag):
        comp = np.ascontiguousarray(comp, np.float32)
        a = np.zeros(64, np.float32)
        for k in range(0, comp.size, 64):
            seg = comp[k:k + 64]
            a[:seg.size] = a[:seg.size] + seg
        idx = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            a = a + a[idx ^ o]
        assert a.dtype == np.float32
        out.append(a[0])
    return np.float32(out[0]), np.float32(out[1])
