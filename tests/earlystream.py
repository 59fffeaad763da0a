"""TEST INFRASTRUCTURE: the IQ-seam stream of the early-message tests (tests/test_cpu_early_messages.py rehearses on the CPU model what
tests/test_gpu_early_messages.py asserts on the device): four messages whose carrier really ends behind their last word
(synth.burst_bits(pad_words=False)) -- a page response (2 words), a registration (3), an origination with seven dialled digits (4) and
an origination with 25 digits (7 words, which never has an event) -- on three live channels at ten samples per symbol, 25 dB."""
import functools

import numpy as np

from gr_amps_amd import synth

SPS, SNR_DB, PUSH = 10, 25.0, 2000
HOLD = SPS * (3374 + 74)
# (live channel, sample offset, kind, dialled digits): the 7-word message follows the page response on its channel, behind the hold-off
PLAN = ((0, 3000, "page_response", ""), (1, 5000, "registration", ""), (2, 7000, "origination", "5551234"),
        (0, 3000 + HOLD + 4000, "origination", "1234567890123456789012345"))
WORDS = (2, 3, 4, 7)
N = (PLAN[3][1] + 82 * SPS + SPS * 3375 + 36 + 2 * PUSH) // PUSH * PUSH


def live_rows(nch):
    """the rows of an nch-channel handle that carry the three live channels: the first, the middle, the last"""
    return (0, nch // 2, nch - 1)


def messages(seed=77):
    rng = np.random.default_rng(seed)
    out = []
    for ch, off, kind, dialed in PLAN:
        min10 = "".join(str(int(d)) for d in rng.integers(0, 10, 10))
        words = synth.make_message(kind, min10, int(rng.integers(0, 2 ** 32)), dialed)
        out.append((ch, off, words, synth.burst_bits(words, dcc=int(rng.integers(0, 4)), pad_words=False)))
    assert tuple(len(w) for _, _, w, _ in out) == WORDS
    return out


@functools.lru_cache(maxsize=None)
def iq_stream(nch=3, ppm=0.0):
    """complex64 [nch][N], read-only: the live channels on live_rows(nch), noise on the others"""
    rng = np.random.default_rng(4000 + nch)
    rows = live_rows(nch)
    iq = np.empty((nch, N), np.complex64)
    for r in range(nch):
        plan = [(off, bits) for ch, off, _, bits in messages() if r in rows and rows.index(r) == ch]
        iq[r] = synth.fsk_modulate(N, plan, sps=SPS, fs=20e3 * SPS, snr_db=SNR_DB, rng=rng, sym_ppm=float(ppm))
    iq.setflags(write=False)
    return iq


def parts(iq, push=PUSH):
    return [np.ascontiguousarray(iq[:, o:o + push]) for o in range(0, iq.shape[1], push)]


def boundaries(n=N, push=PUSH):
    """samples processed after each push of `push` samples: whole 64-sample words of what has arrived"""
    return [min(o + push, n) // 64 * 64 for o in range(0, n, push)]
