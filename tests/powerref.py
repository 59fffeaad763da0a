"""float64 model of the wideband seam's received power (include/amps_recc.h: amps_recc_channel_power / amps_recc_burst_power) -- TEST
INFRASTRUCTURE ONLY.

A power snapshot is |Y_k[m]|^2 of the filter-bank frame m at every channel-rate sample index s = origin + m with s % 256 == 0, Y_k[m]
as oracle/channelizer.py:channelize defines it.  Only those frames are computed here: 1 / 256 of channelize's work."""
import numpy as np

from oracle import channelizer as cz

STRIDE = 256
CAPTURE_SYMS = 3374


def first_snapshot(origin=0):
    """index j of column 0 of snapshots(..., origin): the first snapshot at or behind the origin"""
    return -(-int(origin) // STRIDE)


def snapshots(x, D, first_bin, n_channels, origin=0, P=8, M=1024):
    """x: complex wideband stream from its first sample (channel-rate sample `origin`).  Returns float64 [C][nsnap]: column i is snapshot
    j = first_snapshot(origin) + i, the frame m = 256 j - origin, for every such frame among the len(x) // D whole frames of x."""
    h = cz.design_taps(P, M, cz.cutoff_for_decim(D))
    L = h.size
    x = np.asarray(x, np.complex128)
    nfr = x.size // D
    frames = np.arange((-int(origin)) % STRIDE, nfr, STRIDE)
    bins = (first_bin + np.arange(n_channels)) % M
    out = np.empty((n_channels, frames.size), np.float64)
    for i, m in enumerate(frames):
        n0 = (int(m) + 1) * D - L                                   # the frame covers [n0, n0 + L); samples before the stream are zeros
        seg = np.zeros(L, np.complex128)
        lo = max(n0, 0)
        seg[lo - n0:] = x[lo:n0 + L]
        u = np.roll((seg * h).reshape(-1, M).sum(0), n0 % M)
        y = np.fft.fft(u)[bins]
        out[:, i] = y.real ** 2 + y.imag ** 2
    return out


def burst_window(position, sps):
    """(first snapshot, count) of a record's capture: all j with position <= 256 j <= position + CAPTURE_SYMS * sps"""
    lo, hi = int(position), int(position) + CAPTURE_SYMS * int(sps)
    j0, j1 = -(-lo // STRIDE), hi // STRIDE
    return j0, j1 - j0 + 1


def burst_mean(P, position, sps, first=0):
    """P: one row's snapshots, P[i] = snapshot first + i.  Returns (mean, count) of the capture's snapshots; (0.0, 0) when one of them is
    not in P."""
    j0, cnt = burst_window(position, sps)
    if j0 < first or j0 - first + cnt > len(P):
        return 0.0, 0
    return float(np.mean(np.asarray(P, np.float64)[j0 - first:j0 - first + cnt])), cnt
