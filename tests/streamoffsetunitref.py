"""float64 model of the unit-amplitude carrier-offset statistic of the IQ and translate seams (include/amps_recc.h:
AMPS_RECC_FLAG_STREAM_OFFSET_UNIT) -- TEST INFRASTRUCTURE ONLY.

Block j of a row is U[j] = 2^-8 * sum of u(s) over the channel-rate samples s in [256 j, 256 j + 256), s absolute (origin counted), where
p(s) = y[s] conj(y[s - 1]) with a ZERO in front of the stream's first sample and u(s) = p(s) / |p(s)|; u(s) = (0, 0) where p(s) is zero
or not finite.  p is formed in float64 from the fp32 samples (a product of two fp32 numbers is exact in float64), so the model is the
exact value the header's error bound is stated against.  Zero and non-finite are judged as the device judges them, on p rounded to
fp32: both components zero, or either not finite.  The divisor is 2^8 whatever the number of zero terms.

Windows, burst sums and the argument as a frequency are those of the shipped statistic: streamoffsetref."""
import numpy as np

from streamoffsetref import (STRIDE, _fold, _products, burst_offset_hz, burst_sum, burst_window, first_block,  # noqa: F401
                             gather_sum, offset_hz)


def units(y):
    """complex128 [rows][n]: u(s) of every sample of the stream y (complex [rows][n] or [n], fp32 values)"""
    y, prev = _products(y)
    with np.errstate(all="ignore"):
        p = y * np.conj(prev)
        p32 = p.astype(np.complex64)
        dead = ~(np.isfinite(p32.real) & np.isfinite(p32.imag)) | ((p32.real == 0) & (p32.imag == 0))
        mag = np.hypot(p.real, p.imag)                               # no overflow or underflow of re^2 + im^2
        u = np.where(dead, 0.0, p / np.where(dead, 1.0, mag))
    return u


def blocks(y, origin=0):
    """y: the channel-rate stream from its first sample, which is absolute sample `origin`.  Returns complex128 [rows][nblk]: column i
    is block j = first_block(origin) + i, for every block that lies wholly inside the n samples."""
    return _fold(units(y), origin)


def coherence(total, count):
    """|sum of U over a burst's blocks| / their number: in [0, 1], 1 for a clean carrier, near 0 for noise"""
    return abs(complex(total)) / count if count else 0.0
