"""TEST INFRASTRUCTURE: a second statement of the SEIZURE EVENTS (include/amps_recc_seizure.h, amps_recc_drain_seizures) of one row of slicer
bits, given the list of push boundaries -- the samples processed after each push, multiples of 64.  Written from the header's prose
in numpy; it restates the hold-off walk of tests/trackref.py (captures) instead of calling it, imports no kernel code and nothing of
the C model, and runs on bits that somebody else made: the device's own (Recc.debug_slicer_bits) or the CPU model's.

  * M[n]: the 74 trigger symbols, one every sps samples and the last one AT n, differ from the bits in at most tol places (what lies in
    front of the stream reads 1).  A RUN of matching phases starts where a match has no match among the 2 sps samples before it; its
    centre is the symbol timing n_c.
  * Only run starts with start // 64 + 1 < n_k // 64 have been looked at after boundary n_k.  A start inside the hold-off of the last
    ACCEPTED one (n_c + 3448 sps) is dropped.
  * The PENDING capture after boundary n_k is the accepted n_c with n_c + span >= n_k: its tail has not been received (span = 3375 sps,
    + 36 where the capture tracks the bit clock).
  * Push k reports the pending capture of its boundary if it is not the one reported last: (channel, position = n_c, found_at = n_k),
    and the coded DCC at delay 0 -- s_i = bit n_c + sps (i + 1), dcc[j] = !s_2j, dcc_bad = pairs with s_2j == s_2j+1 -- iff
    n_c + 14 sps < n_k; otherwise zeros and the flag clear."""
import numpy as np

CAPTURE_SYMS, TRIGGER_SYMS, TRACK_BLOCKS, WORD = 3374, 74, 36, 64
DCC_COMPLETE = 1
EVENT_DTYPE = np.dtype([("push", "<i4"), ("channel", "<u4"), ("flags", "<u4"), ("position", "<u8"), ("dcc", "u1", (7,)), ("dcc_bad", "u1"),
                        ("found_at", "<u8")])
FIELDS = ("channel", "flags", "position", "dcc", "dcc_bad", "found_at")


def _trigger():
    bits = ([1, 0] * 15 + [1, 1, 1, 0, 0, 0, 1, 0, 0, 1, 0])[-TRIGGER_SYMS // 2:]
    return np.array([s for b in bits for s in ((0, 1) if b else (1, 0))], np.uint8)      # Manchester: 1 -> (0, 1), 0 -> (1, 0)


def matches(g, sps, tol=0):
    """M[rows][n] of bits g[rows][n] (or one row)"""
    g = np.atleast_2d(np.asarray(g, np.uint8))
    t, n = _trigger(), g.shape[1]
    gp = np.concatenate([np.ones((g.shape[0], sps * (TRIGGER_SYMS - 1)), np.uint8), g], axis=1)
    wrong = np.zeros(g.shape, np.int16)
    for k in range(TRIGGER_SYMS):
        wrong += gp[:, k * sps:k * sps + n] != t[k]
    return wrong <= tol


def accepted(m_row, sps):
    """[(run start, n_c)] of the accepted triggers of one row of matches(), in stream order: the hold-off walk"""
    d = 2 * sps
    out, next_allowed = [], 0
    for p in np.nonzero(m_row)[0]:
        p = int(p)
        if m_row[max(p - d, 0):p].any() or p < next_allowed:
            continue                                                        # not a run's start, or inside the last accepted burst
        nc = p + int(np.nonzero(m_row[p:p + d])[0][-1]) // 2
        next_allowed = nc + sps * (CAPTURE_SYMS + TRIGGER_SYMS)
        out.append((p, nc))
    return out


def span_done(sps, track=True):
    return sps * (CAPTURE_SYMS + 1) + (TRACK_BLOCKS if track else 0)


def pending(acc, sps, n_k, track=True):
    """the pending capture after boundary n_k, or None"""
    seen = [nc for p, nc in acc if p // WORD + 1 < n_k // WORD]
    waiting = [nc for nc in seen if nc + span_done(sps, track) >= n_k]
    assert len(waiting) <= 1                                                # the hold-off is longer than a capture
    return waiting[0] if waiting else None


def row_events(g, sps, boundaries, channel=0, tol=0, track=True, m_row=None):
    """the events of one row of bits, in order, as an EVENT_DTYPE array (`push`: the index into `boundaries` of the push that reports)"""
    g = np.asarray(g, np.uint8)
    acc = accepted(matches(g, sps, tol)[0] if m_row is None else m_row, sps)
    out, reported = [], None
    for k, n_k in enumerate(boundaries):
        assert n_k % WORD == 0 and n_k <= len(g)
        p = pending(acc, sps, n_k, track)
        if p is None or p == reported:
            continue
        reported = p
        e = np.zeros((), EVENT_DTYPE)
        e["push"], e["channel"], e["position"], e["found_at"] = k, channel, p, n_k
        if p + 14 * sps < n_k:
            s = g[p + sps * np.arange(1, 15)]
            e["flags"], e["dcc"], e["dcc_bad"] = DCC_COMPLETE, 1 - s[0::2], int((s[0::2] == s[1::2]).sum())
        out.append(e)
    return np.array(out, EVENT_DTYPE)


def events(bits, sps, boundaries, tol=0, track=True, origin=0):
    """the events of all rows bits[rows][>= boundaries[-1]] in the order the list holds them, (found_at, channel); bit i of a row is
    the stream's sample origin + i, and the boundaries count from the origin too"""
    bits = np.atleast_2d(np.asarray(bits, np.uint8))[:, :boundaries[-1]]
    m = matches(bits, sps, tol)
    per = [row_events(bits[r], sps, boundaries, r, tol, track, m[r]) for r in np.nonzero(m.any(axis=1))[0]]
    ev = np.concatenate(per) if per else np.zeros(0, EVENT_DTYPE)
    ev = ev[np.lexsort((ev["channel"], ev["push"]))]
    ev["position"] += origin
    ev["found_at"] += origin
    return ev


def assert_equal(got, want, what=""):
    """every field of the drained events `got` (capi.SEIZURE_DTYPE) equals the statement's"""
    assert len(got) == len(want), (what, len(got), len(want), got[:4], want[:4])
    for f in FIELDS:
        differs = (np.asarray(got[f]) != np.asarray(want[f])).reshape(len(want), -1 if len(want) else 1).any(axis=1)
        bad = np.nonzero(differs)[0]
        assert bad.size == 0, (what, f, got[bad[:4]], want[bad[:4]])
