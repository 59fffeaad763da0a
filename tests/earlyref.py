"""TEST INFRASTRUCTURE: a second statement of the EARLY MESSAGES (include/amps_recc_early.h, amps_recc_drain_early) of one row of slicer
bits, given the list of push boundaries -- the samples processed after each push, multiples of 64.  Written from the header's prose in
numpy on tests/trackref.py (the capture's timing rule, restated here block by block so that it can stop early and say its delays),
tests/refdecode.py (the decode, both modes) and tests/seizureref.py (which capture is pending after a boundary).  It imports no kernel
code, nothing of the C model and nothing of the binding, and runs on bits that somebody else made: the device's own
(Recc.debug_slicer_bits) or the CPU model's.

  * After boundary n_k a row's PENDING capture p (seizureref.pending) is looked at.  T(n) = p + sps (15 + 480 n) + K, K = 36 where the
    capture tracks and 0 with fixed timing.
  * Once T(1) < n_k: walk(blocks 0 .. 5), decode, word A says n_words = NAWC + 1; invalid, or 7 and more: never an event.
  * First boundary with T(n_words) < n_k: the event.  Its record is the decode of the walk over 1 + 5 n_words blocks with the symbols of
    the other words set to the pair (1, 0) -- bit 0, no Manchester violation -- and valid = 0, first_valid_rep = 5 for those words."""
import numpy as np

import refdecode
import seizureref
import trackref

CAPTURE_SYMS, TRIGGER_SYMS, TRACK_BLOCKS = trackref.CAPTURE_SYMS, trackref.TRIGGER_SYMS, trackref.TRACK_BLOCKS
WORD_BITS, REPEATS, WORDS = trackref.WORD_BITS, trackref.REPEATS, trackref.WORDS
MAX_WORDS = WORDS - 1                               # a seven-word message has no event

# the layout of amps_recc_burst_t (include/amps_recc.h, 728 bytes) and of amps_recc_early_t (include/amps_recc_early.h, 744), stated again
RECORD_DTYPE = np.dtype([
    ("channel", "<u4"), ("flags", "<u4"), ("position", "<u8"), ("dcc", "u1", (7,)), ("dcc_bad", "u1"),
    ("manch_bad", "<u2", (7,)), ("valid", "u1", (7,)), ("first_valid_rep", "u1", (7,)), ("word_raw", "u1", (7, 48)), ("word_dec", "u1", (7, 36)),
    ("a_F", "u1"), ("a_NAWC", "u1"), ("a_T", "u1"), ("a_S", "u1"), ("a_E", "u1"), ("a_ER", "u1"), ("a_SCM", "u1"), ("_pad0", "u1"), ("a_MIN1", "<u4"),
    ("b_F", "u1"), ("b_NAWC", "u1"), ("b_MSG_TYPE", "u1"), ("b_ORDQ", "u1"), ("b_ORDER", "u1"), ("b_LT", "u1"), ("b_EP", "u1"), ("b_SCM4", "u1"),
    ("b_MPCI", "u1"), ("b_SDCC1", "u1"), ("b_SDCC2", "u1"), ("_pad1", "u1"), ("b_MIN2", "<u2"), ("_pad2", "<u2"),
    ("esn", "<u4"), ("has_esn", "u1"), ("msg_class", "u1"), ("n_called_words", "u1"), ("_pad3", "u1"), ("min", "S12"), ("dialed", "S36"), ("_pad4", "<u4")])
EVENT_DTYPE = np.dtype([("rec", RECORD_DTYPE), ("found_at", "<u8"), ("n_words", "<u4"), ("_pad", "<u4")])
assert RECORD_DTYPE.itemsize == 728 and EVENT_DTYPE.itemsize == 744
FLAG_NAWC_MISMATCH, FLAG_BAD_DIGIT, FLAG_DCC_INVALID = 2, 4, 8
# what the relation to the record promises for the words w < n_words, and for the whole event
PER_WORD = ("manch_bad", "valid", "first_valid_rep", "word_raw", "word_dec")
WORD_A = ("a_F", "a_NAWC", "a_T", "a_S", "a_E", "a_ER", "a_SCM", "a_MIN1")


def due(p, sps, n, track=True):
    """T(n): the first n words of capture p are in once T(n) < samples processed"""
    return p + sps * (15 + 2 * WORD_BITS * REPEATS * n) + (TRACK_BLOCKS if track else 0)


def _bit(g, n):
    n = np.asarray(n)
    return np.where(n < 0, 1, g[np.maximum(n, 0)])  # what lies in front of the stream reads 1; an index behind g is an IndexError


def walk(g, nc, sps, track=True, nblocks=TRACK_BLOCKS):
    """The capture's timing walk (trackref.capture's rule) over its first `nblocks` blocks: (symbols of those blocks, 14 + 96 (nblocks - 1)
    of them, the delay each block was TAKEN at).  Block 0 is the trigger's 37 bits in front of the capture, block 1 the coded DCC with
    repeat 0 of word A, every other block one repeat.  From three samples per symbol on a block's mid-bit transitions move everything
    BEHIND it; at two a block chooses its OWN delay among the one before and its two neighbours by its Manchester violations."""
    g = np.asarray(g, np.uint8)
    sizes = ([TRIGGER_SYMS // 2, 7 + WORD_BITS] + [WORD_BITS] * (WORDS * REPEATS - 1))[:nblocks]
    sym = np.zeros(2 * sum(sizes[1:]), np.uint8)
    delays, delay, first = [], 0, -(TRIGGER_SYMS // 2)
    for nb in sizes:
        k = np.arange(first, first + nb)
        if track and sps == 2:
            t3 = nc + sps * (2 * k[None, :] + 1) + delay + np.array([0, -1, 1])[:, None]
            viol = (_bit(g, t3) == _bit(g, t3 + sps)).sum(1)
            delay += (0, -1, 1)[int(np.argmin(viol))]               # the first minimum in the order (d, d - 1, d + 1)
        delays.append(delay)
        t = nc + sps * (2 * k + 1) + delay
        a, b = _bit(g, t), _bit(g, t + sps)
        keep = k >= 0
        sym[2 * k[keep]], sym[2 * k[keep] + 1] = a[keep], b[keep]
        if track and sps > 2:
            between = _bit(g, t[:, None] + np.arange(1, sps)[None, :])
            late = 2 * (between == a[:, None]).sum(1) - (sps - 1)     # twice how late the mid-bit transition came: integers
            pair = a != b
            f, r = late[pair & (a == 1)], late[pair & (a == 0)]
            if len(f) and len(r):
                lhs, rhs = int(f.sum()) * len(r) + int(r.sum()) * len(f), 2 * len(f) * len(r)   # mean(f) / 2 + mean(r) / 2 against +-1
                delay += 1 if lhs > rhs else -1 if lhs < -rhs else 0
        first += nb
    return sym, delays


def prefix_symbols(g, nc, sps, track, n):
    """the 3374 symbols the event's record is decoded from: the walk over the first n words, the pair (1, 0) everywhere behind"""
    sym, _ = walk(g, nc, sps, track, 1 + REPEATS * n)
    assert len(sym) == 14 + 2 * WORD_BITS * REPEATS * n
    rest = np.tile(np.array([1, 0], np.uint8), (CAPTURE_SYMS - len(sym)) // 2)
    return np.concatenate([sym, rest])


def record_of(dec, channel=0, position=0):
    """a refdecode dictionary as the 728 bytes of amps_recc_burst_t"""
    r = np.zeros((), RECORD_DTYPE)
    r["channel"], r["position"] = channel, position
    r["flags"] = FLAG_NAWC_MISMATCH * bool(dec["nawc_mismatch"]) + FLAG_BAD_DIGIT * bool(dec["bad_digit"]) + FLAG_DCC_INVALID * bool(dec["dcc_invalid"])
    r["dcc"], r["dcc_bad"], r["manch_bad"] = dec["dcc"], dec["dcc_bad"], dec["manch_bad"]
    r["valid"], r["first_valid_rep"] = [int(v) for v in dec["valid"]], dec["first_valid_rep"]
    r["word_raw"], r["word_dec"] = dec["word_raw"], dec["word_dec"]
    for k, v in dec["a"].items():
        r["a_" + k] = v
    for k, v in dec["b"].items():
        r["b_" + k] = v
    r["esn"], r["has_esn"], r["msg_class"], r["n_called_words"] = dec["esn"], dec["has_esn"], dec["cls"], dec["n_called_words"]
    r["min"], r["dialed"] = dec["min"].encode(), dec["dialed"].encode()
    return r


def decode(sym, majority=False):
    return refdecode.decode_majority(sym) if majority else refdecode.decode(sym)


def announced(g, p, sps, track=True, majority=False):
    """n_words of capture p from word A alone, or None where it never has an event"""
    a = decode(prefix_symbols(g, p, sps, track, 1), majority)
    n = a["a"]["NAWC"] + 1
    return n if a["valid"][0] and n <= MAX_WORDS else None


def event_record(g, p, sps, n, track=True, majority=False, channel=0):
    r = record_of(decode(prefix_symbols(g, p, sps, track, n), majority), channel, p)
    r["valid"][n:], r["first_valid_rep"][n:] = 0, REPEATS
    return r


def row_events(g, sps, boundaries, channel=0, tol=0, track=True, majority=False, m_row=None):
    """[(push, EVENT_DTYPE scalar)] of one row of bits, in order.  At boundary n_k only g[:n_k] is looked at."""
    g = np.asarray(g, np.uint8)
    acc = seizureref.accepted(seizureref.matches(g, sps, tol)[0] if m_row is None else m_row, sps)
    out, cur, words, done = [], None, 0, False
    for k, n_k in enumerate(boundaries):
        p = seizureref.pending(acc, sps, n_k, track)
        if p is None:
            continue
        if p != cur:
            cur, words, done = p, 0, False                          # words: 0 = word A not looked at, None = never
        seen = g[:n_k]
        if words == 0 and due(p, sps, 1, track) < n_k:
            words = announced(seen, p, sps, track, majority)
        if words and not done and due(p, sps, words, track) < n_k:
            e = np.zeros((), EVENT_DTYPE)
            e["rec"], e["found_at"], e["n_words"] = event_record(seen, p, sps, words, track, majority, channel), n_k, words
            out.append((k, e))
            done = True
    return out


def events(bits, sps, boundaries, tol=0, track=True, majority=False, origin=0):
    """(pushes, EVENT_DTYPE array) of all rows bits[rows][>= boundaries[-1]] in the order the list holds them, (found_at, channel); bit i
    of a row is the stream's sample origin + i, and the boundaries count from the origin too"""
    bits = np.atleast_2d(np.asarray(bits, np.uint8))[:, :boundaries[-1]]
    m = seizureref.matches(bits, sps, tol)
    per = [x for r in np.nonzero(m.any(axis=1))[0] for x in row_events(bits[r], sps, boundaries, int(r), tol, track, majority, m[r])]
    per.sort(key=lambda x: (x[0], int(x[1]["rec"]["channel"])))
    ev = np.array([e for _, e in per], EVENT_DTYPE) if per else np.zeros(0, EVENT_DTYPE)
    ev["rec"]["position"] += origin
    ev["found_at"] += origin
    return np.array([k for k, _ in per], np.int64), ev


def assert_equal(got, want, what=""):
    """every byte of the drained events equals the statement's; the first differing field is named"""
    assert len(got) == len(want), (what, len(got), len(want))
    got = np.asarray(got).view(EVENT_DTYPE) if len(got) else np.zeros(0, EVENT_DTYPE)
    for i in range(len(want)):
        if got[i].tobytes() == want[i].tobytes():
            continue
        for f in ("found_at", "n_words"):
            assert got[i][f] == want[i][f], (what, i, f, got[i][f], want[i][f])
        for f in RECORD_DTYPE.names:
            assert np.array_equal(got[i]["rec"][f], want[i]["rec"][f]), (what, i, f, got[i]["rec"][f], want[i]["rec"][f])
        raise AssertionError((what, i, "padding differs"))


def assert_relation(e, R):
    """the header's relation between an event and the record R that follows it"""
    rec, n = e["rec"], int(e["n_words"])
    assert int(rec["channel"]) == int(R["channel"]) and int(rec["position"]) == int(R["position"])
    for f in ("dcc", "dcc_bad") + WORD_A:
        assert np.array_equal(rec[f], R[f]), (f, rec[f], R[f])
    for f in PER_WORD:
        assert np.array_equal(rec[f][:n], R[f][:n]), (f, rec[f][:n], R[f][:n])
    assert not rec["valid"][n:].any() and (rec["first_valid_rep"][n:] == REPEATS).all()
    assert not rec["word_raw"][n:].any() and not rec["word_dec"][n:].any() and not rec["manch_bad"][n:].any()
