"""float64 model of the IQ and translate seams' received power (include/amps_recc.h: AMPS_RECC_FLAG_STREAM_POWER) -- TEST
INFRASTRUCTURE ONLY.

Block j of a row is the mean of |y[s]|^2 over the channel-rate samples s in [256 j, 256 j + 256), s absolute (origin counted).  A
record's burst power is the mean of the blocks that lie wholly inside its capture [position, position + 3374 * sps)."""
import numpy as np

STRIDE = 256
CAPTURE_SYMS = 3374


def first_block(origin=0):
    """index j of column 0 of blocks(..., origin): the first block that does not begin before the origin"""
    return -(-int(origin) // STRIDE)


def blocks(y, origin=0):
    """y: complex [rows][n] (or [n]) channel-rate stream from its first sample, which is absolute sample `origin`.  Returns float64
    [rows][nblk]: column i is block j = first_block(origin) + i, for every block that lies wholly inside the n samples."""
    y = np.atleast_2d(np.asarray(y))
    p = y.real.astype(np.float64) ** 2 + y.imag.astype(np.float64) ** 2
    j0 = first_block(origin)
    skip = j0 * STRIDE - int(origin)                                 # samples in front of the first whole block
    nblk = max(0, (p.shape[1] - skip) // STRIDE)
    return p[:, skip:skip + nblk * STRIDE].reshape(p.shape[0], nblk, STRIDE).mean(axis=2)


def burst_window(pos, sps):
    """(first block, count) of a record's capture: the blocks j with pos <= 256 j and 256 (j + 1) <= pos + CAPTURE_SYMS * sps"""
    lo, hi = int(pos), int(pos) + CAPTURE_SYMS * int(sps)
    j0, j1 = -(-lo // STRIDE), hi // STRIDE - 1
    return j0, j1 - j0 + 1


def burst_mean(row, pos, sps, first=0):
    """row: one channel's blocks, row[i] = block first + i.  Returns (mean, count) over the capture's blocks; (0.0, 0) when one of them
    is not in row."""
    j0, cnt = burst_window(pos, sps)
    if j0 < first or j0 - first + cnt > len(row):
        return 0.0, 0
    return float(np.mean(np.asarray(row, np.float64)[j0 - first:j0 - first + cnt])), cnt
