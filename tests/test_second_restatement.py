"""tests/refdecode.py (a second restatement of bursts_message, written apart from oracle/ref_chain.c) against the oracle on CPU
and against the HIP decode kernel on the GPU: random bursts steered into every message class, with bit errors (so that the
first-valid-of-five rule and the 'parse repeat 0 as received' quirk matter) and non-Manchester symbol pairs."""
import numpy as np
import pytest

import bchref
import oracle
import refdecode
from gr_amps_amd import capi


def _cw(msg36):
    m = 0
    for b in msg36:
        m = (m << 1) | int(b)
    m <<= 12
    w = m | bchref.polymod(m)
    return [(w >> (47 - i)) & 1 for i in range(48)]


def _bits(v, n):
    return [(v >> (n - 1 - i)) & 1 for i in range(n)]


def _message(rng, kind):
    """the seven words (36 message bits each) of a burst steered into the message class `kind`"""
    nawc_a = int(rng.integers(0, 8))
    T, S, E = int(rng.integers(0, 2)), int(rng.integers(0, 2)), 1
    order, ordq, mtype = 0, 0, 0
    if kind == "page":
        T = 0
    elif kind == "registration":
        T, order = 1, 0xD
        ordq, mtype = int(rng.integers(0, 8)), int(rng.integers(0, 32))
    elif kind == "origination":
        T = 1
        nawc_a = int(rng.integers(1, 5)) + (2 if S else 0)
        if rng.integers(0, 2):
            order, ordq, mtype = int(rng.integers(0, 13)), int(rng.integers(0, 8)), int(rng.integers(0, 32))
            if order or ordq or mtype:
                nawc_a = max(nawc_a, 3)
    elif kind == "bad_nawc":
        T, S = 1, int(rng.integers(0, 2))
        nawc_a = int(rng.choice([0, 5, 6, 7])) if not S else int(rng.choice([0, 1, 2, 7]))
        if nawc_a <= 2:
            order, ordq, mtype = 0, 0, 0
        else:
            order = int(rng.integers(0, 13))
    elif kind == "e_zero":
        E = 0
    elif kind == "unknown":
        T, nawc_a, order = 1, int(rng.integers(0, 3)), int(rng.choice([1, 2, 3, 7, 0xC, 0xE, 0x1F]))
    elif kind == "random":
        T, S, E = (int(x) for x in rng.integers(0, 2, 3))
        order, ordq, mtype = int(rng.integers(0, 32)), int(rng.integers(0, 8)), int(rng.integers(0, 32))
    words = []
    words.append([1] + _bits(nawc_a, 3) + [T, S, E, int(rng.integers(0, 2))] + _bits(int(rng.integers(0, 16)), 4) + _bits(int(rng.integers(0, 1 << 24)), 24))
    words.append([0] + _bits(int(rng.integers(0, 8)), 3) + _bits(mtype, 5) + _bits(ordq, 3) + _bits(order, 5) +
                 [int(x) for x in rng.integers(0, 2, 3)] + _bits(int(rng.integers(0, 4)), 2) + _bits(int(rng.integers(0, 4)), 2) +
                 _bits(int(rng.integers(0, 4)), 2) + _bits(int(rng.integers(0, 1 << 10)), 10))
    for _ in range(5):
        if rng.integers(0, 3) == 0:          # a serial-number word
            nw = int(rng.integers(0, 8)) if rng.integers(0, 4) == 0 else (nawc_a - 2) & 7
            words.append([0] + _bits(nw, 3) + _bits(int(rng.integers(0, 1 << 32)), 32))
        else:                                # a called-address word: digit codes incl. terminators and invalid codes
            codes = [int(rng.choice([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 0, 13, 15], p=[.08] * 12 + [.02, .01, .01])) for _ in range(8)]
            d = 0
            for c in codes:
                d = (d << 4) | c
            words.append([0] + _bits(int(rng.integers(0, 8)), 3) + _bits(d, 32))
    return words


def make_burst(rng, kind):
    words = _message(rng, kind)
    bits = [int(x) for x in rng.integers(0, 2, 7)]                 # DCC: seven free bits here
    for wi, w in enumerate(words):
        cw = _cw(w)
        for r in range(5):
            while True:
                rep = list(cw)
                ne = int(rng.choice([0, 0, 0, 1, 2, 3, 4])) if not (kind == "invalid_a" and wi == 0) else int(rng.integers(3, 7))
                for p in rng.choice(48, size=ne, replace=False):
                    rep[int(p)] ^= 1
                if not (kind == "invalid_a" and wi == 0) or not refdecode.bch_valid(rep):
                    break                                              # half of all 63-bit words decode: draw until this one does not
            bits += rep
    sym = np.empty(2 * len(bits), np.uint8)
    sym[0::2] = [1 - b for b in bits]                              # '0' -> (1,0), '1' -> (0,1)
    sym[1::2] = bits
    for p in rng.choice(len(sym), size=int(rng.choice([0, 0, 3, 12])), replace=False):
        sym[int(p)] ^= 1                                           # (1,1) / (0,0) pairs: decoded with the reference's bias, counted bad
    assert len(sym) == 3374
    return sym


KINDS = ["page", "registration", "origination", "bad_nawc", "e_zero", "unknown", "invalid_a", "random"]


def _bursts(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([make_burst(rng, KINDS[i % len(KINDS)]) for i in range(n)])


def _check(rec, want, i):
    assert list(rec["dcc"]) == want["dcc"] and int(rec["dcc_bad"]) == want["dcc_bad"], i
    assert list(rec["manch_bad"]) == want["manch_bad"], i
    assert [bool(v) for v in rec["valid"]] == want["valid"] and list(rec["first_valid_rep"]) == want["first_valid_rep"], i
    a, b = want["a"], want["b"]
    for k in ("F", "NAWC", "T", "S", "E", "ER", "SCM", "MIN1"):
        assert int(rec["a_" + k]) == a[k], (i, "a_" + k)
    for k in ("F", "NAWC", "MSG_TYPE", "ORDQ", "ORDER", "LT", "EP", "SCM4", "MPCI", "SDCC1", "SDCC2", "MIN2"):
        assert int(rec["b_" + k]) == b[k], (i, "b_" + k)
    assert rec["min"].decode() == want["min"], i
    assert int(rec["msg_class"]) == want["cls"], (i, int(rec["msg_class"]), want["cls"])
    assert int(rec["esn"]) == want["esn"] and int(rec["has_esn"]) == want["has_esn"], i
    assert rec["dialed"].decode() == want["dialed"] and int(rec["n_called_words"]) == want["n_called_words"], i
    assert bool(int(rec["flags"]) & 2) == want["nawc_mismatch"] and bool(int(rec["flags"]) & 4) == want["bad_digit"], i
    for w in range(7):
        assert rec["word_raw"][w].tolist() == want["word_raw"][w], (i, "word_raw", w)
        assert rec["word_dec"][w].tolist() == want["word_dec"][w], (i, "word_dec", w)
    assert bool(int(rec["flags"]) & 8) == want["dcc_invalid"], (i, "DCC_INVALID")      # never set in reference mode


def _differs(rec, want):
    try:
        _check(rec, want, 0)
    except AssertionError:
        return True
    return False


# ---------------------------------------------------------------------------------------- bursts that reach every branch (bchref only)
def _blk(pattern):
    """an error pattern over the 63-bit word (bit e = x^e, tests/bchref.py) that lies inside the 48 transmitted bits, as 48 flips in
    transmitted order"""
    assert pattern >> 48 == 0
    return bchref.bits(pattern)[15:]


def _flip(block, flips):
    return [a ^ b for a, b in zip(block, flips)]


def _rand_flips(rng, n, lo=0, hi=48):
    f = [0] * 48
    for p in rng.choice(np.arange(lo, hi), size=n, replace=False):
        f[int(p)] = 1
    return f


_PAD3 = []


def _pad_triples():
    """every pattern of three flips inside the 48 bits whose coset leader (tests/bchref.py) has a bit in positions 48..62: a decoder
    "corrects" such a word by flipping a shortening zero"""
    if not _PAD3:
        lead = bchref.coset_leaders()
        for i in range(48):
            for j in range(i):
                for k in range(j):
                    e = (1 << i) | (1 << j) | (1 << k)
                    r = bchref.polymod(e)
                    if r in lead and lead[r][1] >> 48:
                        _PAD3.append(e)
    return _PAD3


def _three_roots(p):
    """the pattern x^p + x^(p+21) + x^(p+42): S1 = 0, S3 = alpha^(3p), a cube.  Inside the 48 bits for p < 6.  For p >= 6 a code word
    is added that clears positions 48..62: the SAME syndromes, inside the 48 bits, but the three positions IT++ flips are the
    original ones, one of them among the shortening zeros"""
    t = (1 << p) | (1 << (p + 21)) | (1 << (p + 42))
    assert bchref.evaluate(t, 1) == 0 and bchref.is_cube(bchref.evaluate(t, 3))
    if p >= 6:
        m = (t >> 48) << 48
        t ^= m | bchref.polymod(m)
    return t


def _symbols(rng, dcc, reps, n_bad):
    bits = list(dcc)
    for w in reps:
        for r in w:
            assert len(r) == 48
            bits += r
    sym = np.empty(2 * len(bits), np.uint8)
    sym[0::2] = [1 - b for b in bits]
    sym[1::2] = bits
    for p in rng.choice(len(sym), size=n_bad, replace=False):
        sym[int(p)] ^= 1
    assert len(sym) == 3374
    return sym


def _invalid_flips(rng, cw, majority):
    """three to six flips after which the word does not decode (majority: or decodes into the shortening zeros)"""
    while True:
        f = _rand_flips(rng, int(rng.integers(3, 7)))
        flag, _, in_pad, _ = refdecode.bch_correct(_flip(cw, f))
        if not flag or (majority and in_pad):
            return f


CLASS_KINDS = ["page", "registration", "origination", "bad_nawc", "e_zero", "unknown", "invalid_a"]
MAJ_KINDS = ["clean", "rate .01", "rate .03", "rate .06", "rate .10", "residual 1", "residual 2", "residual 3", "residual 4",
             "agree 0", "agree 1", "agree 2", "agree 3", "agree 4", "pad_reject A", "pad_reject B", "pad_reject read", "pad_reject unread",
             "quirk3 accepted", "quirk3 rejected", "dcc1", "dcc2", "unread_invalid", "demote"]
DCC_CODES = ["0000000", "0011111", "1100011", "1111100"]


def make_majority_burst(rng, kind, msgkind, rep):
    """one burst for the majority branch.  `kind` says what is done to the repeats (or to the coded DCC), `msgkind` which message
    class the clean words would give; rep = how often this kind has been made before: it picks the DCC code word of `dcc1` / `dcc2`
    and the branch (origination, registration) of the kinds that need a word behind B to be read, so that neither depends on where
    the kind stands in MAJ_KINDS.  Every other burst draws its code word, and a distance of 0, 1 or 2 from it, from the rng."""
    needs_c = kind in ("pad_reject read", "demote")
    if needs_c:
        msgkind = ("origination", "registration")[rep % 2]
    while True:
        words = _message(rng, "e_zero" if msgkind == "invalid_a" else msgkind)
        cws = [_cw(w) for w in words]
        dcc = [int(c) for c in DCC_CODES[rep % 4 if kind in ("dcc1", "dcc2") else int(rng.integers(0, 4))]]
        clean = refdecode.decode_majority(_symbols(rng, dcc, [[cw] * 5 for cw in cws], 0))
        read, unread = clean["read"], [w for w in range(7) if w not in clean["read"]]
        if (not needs_c or len(read) > 2) and (unread or "unread" not in kind):
            break
    nd = {"dcc1": 1, "dcc2": 2}.get(kind, int(rng.choice([0, 0, 1, 2])))
    for p in rng.choice(7, size=nd, replace=False):
        dcc[int(p)] ^= 1
    reps = []
    special = {"pad_reject A": [0], "pad_reject B": [1], "pad_reject read": read[2:], "pad_reject unread": unread, "unread_invalid": unread,
               "demote": read[1:], "quirk3 accepted": range(7), "quirk3 rejected": range(7)}.get(kind)
    special = None if special is None else int(rng.choice(list(special)))
    for w, cw in enumerate(cws):
        common, nrep, light = [0] * 48, 5, 0.0
        if msgkind == "invalid_a" and w == 0:
            common, nrep = _invalid_flips(rng, cw, True), int(rng.integers(3, 6))
        elif w == special:
            nrep = int(rng.integers(3, 6))
            if kind.startswith("pad_reject"):
                common = _blk(int(rng.choice(_pad_triples())))
            elif kind == "quirk3 accepted":
                common = _blk(_three_roots(int(rng.integers(0, 6))))
            elif kind == "quirk3 rejected":
                common = _blk(_three_roots(int(rng.integers(6, 21))))
            else:
                common = _invalid_flips(rng, cw, True)
        elif kind.startswith("residual"):
            common, nrep, light = _rand_flips(rng, int(kind[-1])), int(rng.integers(3, 6)), float(rng.choice([0.0, 0.01]))
        elif kind.startswith("rate"):
            light = float(kind[4:])
        elif not kind.startswith("agree"):
            light = float(rng.choice([0.0, 0.0, 0.005]))
        planted = set(int(r) for r in rng.choice(5, size=nrep, replace=False))
        rs = [_flip(cw, common) if r in planted else list(cw) for r in range(5)]
        if kind.startswith("agree"):                            # 5 - n repeats with one flip each, all at different positions
            n = int(kind[-1])
            for r, p in zip(rng.choice(5, size=5 - n, replace=False), rng.choice(48, size=5, replace=False)):
                rs[int(r)][int(p)] ^= 1
        for r in rs:
            for p in np.nonzero(rng.random(48) < light)[0]:
                r[int(p)] ^= 1
        reps.append(rs)
    return _symbols(rng, dcc, reps, int(rng.choice([0, 0, 0, 3])))


REF_KINDS = ["first 0", "first 1", "first 2", "first 3", "first 4", "first 5", "parity_only", "straddle"]


def make_reference_burst(rng, kind, msgkind):
    """one burst for the reference branch: every word's first valid repeat is chosen (`first r`, r = 5: none), or drawn from 1..4 with
    that repeat's errors confined to the parity bits (`parity_only`) or one on either side of the message/parity boundary (`straddle`)"""
    words = _message(rng, msgkind)
    dcc = [int(x) for x in rng.integers(0, 2, 7)]
    reps = []
    for w, m in enumerate(words):
        cw = _cw(m)
        first = int(kind[-1]) if kind.startswith("first") else int(rng.integers(1, 5))
        if msgkind != "invalid_a" and w == 0 and first == 5:
            first = 4                                            # keep word A (and with it the class) unless the class is the point
        rs = []
        for r in range(5):
            if r < first:
                rs.append(_flip(cw, _invalid_flips(rng, cw, False)))
            elif r > first:
                rs.append(_flip(cw, _rand_flips(rng, int(rng.choice([0, 1, 2, 3, 4])))))
            elif kind == "parity_only":
                rs.append(_flip(cw, _rand_flips(rng, int(rng.integers(1, 3)), 36, 48)))
            elif kind == "straddle":
                rs.append(_flip(_flip(cw, _rand_flips(rng, 1, 0, 36)), _rand_flips(rng, 1, 36, 48)))
            else:
                rs.append(_flip(cw, _rand_flips(rng, int(rng.integers(0, 3)))))
        reps.append(rs)
    return _symbols(rng, dcc, reps, int(rng.choice([0, 0, 3])))


_sets = {}


def majority_set():
    """(bursts [240][3374], [decode_majority of each], [kind of each]): every kind ten times, over the seven message classes"""
    if "maj" not in _sets:
        rng = np.random.default_rng(553)
        kinds = [MAJ_KINDS[i % len(MAJ_KINDS)] for i in range(240)]
        b = np.stack([make_majority_burst(rng, k, CLASS_KINDS[i % 7], i // len(MAJ_KINDS)) for i, k in enumerate(kinds)])
        _sets["maj"] = (b, [refdecode.decode_majority(x) for x in b], kinds)
    return _sets["maj"]


def reference_set():
    """(bursts [160][3374], [decode of each]): the eight kinds of make_burst eight times, the eight of make_reference_burst twelve times"""
    if "ref" not in _sets:
        rng = np.random.default_rng(1983)
        b = [make_burst(rng, KINDS[i % len(KINDS)]) for i in range(64)]
        b += [make_reference_burst(rng, REF_KINDS[i % 8], (CLASS_KINDS + ["random"])[(i // 8 + i) % 8]) for i in range(96)]
        b = np.stack(b)
        _sets["ref"] = (b, [refdecode.decode(x) for x in b])
    return _sets["ref"]


def majority_coverage(wants):
    """what the second statement says the majority set reaches: {condition: number of bursts}"""
    n = {}

    def count(key, hit):
        n[key] = n.get(key, 0) + bool(hit)
    for d in wants:
        for c in range(7):
            count("class %d" % c, d["cls"] == c)
        count("demoted by a word the dispatch read", d["cls"] == refdecode.INVALID_WORD_A and d["valid"][0])
        count("class kept beside an invalid word the dispatch did not read", d["cls"] >= refdecode.PAGE_RESPONSE and not all(d["valid"]))
        count("pad-rejected word", "leader_pad" in d["verdict"])
        count("accepted three-root word", "three_ok" in d["verdict"])
        count("rejected three-root word", "three_pad" in d["verdict"])
        count("DCC flag set", d["dcc_invalid"])
        count("DCC flag clear at distance 1", d["dcc_distance"] == 1 and not d["dcc_invalid"])
        for code in DCC_CODES:                                   # each of the four comparisons on its own, on either side of its bound
            off = sum(int(c) != b for c, b in zip(code, d["dcc"]))
            count("DCC flag clear one bit off " + code, off == 1 and not d["dcc_invalid"])
            count("DCC flag set two bits off " + code, off == 2 and d["dcc_invalid"])
        # used_ok per branch: a word behind B that the branch read is pad-rejected (A and B are valid: the class was the branch's own)
        behind = [w for w in d["read"][2:] if d["verdict"][w] == "leader_pad"]
        demoted = d["cls"] == refdecode.INVALID_WORD_A and d["valid"][0] and d["valid"][1] and bool(behind)
        registration = d["a"]["T"] == 1 and d["b"]["ORDER"] == 0xD
        count("registration demoted by a pad-rejected word C", demoted and registration)
        count("origination demoted by a pad-rejected word behind B", demoted and not registration)
        for a in range(6):
            count("agree count %d" % a, a in d["first_valid_rep"])
    return n


def reference_coverage(wants):
    firsts = {r for d in wants for r in d["first_valid_rep"]}
    fixes = [f for d in wants for f in d["fixes"] if f]
    return firsts, sum(f[0] > 0 for f in fixes), sum(f[0] == 0 and f[1] > 0 for f in fixes), sum(f[0] > 0 and f[1] > 0 for f in fixes)


def test_oracle_equals_the_second_restatement():
    bursts = _bursts(160, 2024)
    recs = oracle.decode_bursts(bursts)
    seen = set()
    for i in range(len(bursts)):
        want = refdecode.decode(bursts[i])
        _check(recs[i], want, i)
        seen.add(want["cls"])
    assert seen == set(range(7))                                   # every branch of bursts_message was taken


def test_reference_set_reaches_every_branch_and_the_oracle_agrees():
    bursts, wants = reference_set()
    assert len(bursts) <= 192
    firsts, in_msg, parity_only, straddling = reference_coverage(wants)
    print(f"\nreference set: {len(bursts)} bursts, first_valid_rep {sorted(firsts)}, words corrected inside the message bits {in_msg}, "
          f"in the parity only {parity_only}, on both sides {straddling}")
    assert firsts == set(range(6)) and in_msg >= 30 and parity_only >= 10 and straddling >= 10
    assert {d["cls"] for d in wants} == set(range(7))
    for i, (rec, want) in enumerate(zip(oracle.decode_bursts(bursts), wants)):
        _check(rec, want, i)


def test_majority_set_reaches_every_branch_and_the_oracle_agrees():
    bursts, wants, kinds = majority_set()
    assert len(bursts) <= 256
    cover = majority_coverage(wants)
    print("\nmajority set: %d bursts; %s" % (len(bursts), ", ".join("%s: %d" % kv for kv in cover.items())))
    per_branch = [k for k in cover if "demoted by a pad-rejected" in k]     # five bursts are planted for either branch
    assert all(v >= (4 if k in per_branch else 8) for k, v in cover.items()), {k: v for k, v in cover.items() if v < 8}
    residual = {}
    for d, k in zip(wants, kinds):                                 # errors left in the voted word of the `rate` and `residual` bursts
        if k.startswith(("rate", "residual")):
            for w in range(7):
                left = "3+" if not d["valid"][w] else sum(x != y for x, y in zip(d["word_raw"][w][:36], d["word_dec"][w]))
                residual[left] = residual.get(left, 0) + 1
    print("voted words by message-bit corrections (3+: not valid):", residual)
    assert all(residual.get(k, 0) >= 8 for k in (0, 1, 2, "3+"))
    for i, (rec, want) in enumerate(zip(oracle.decode_bursts(bursts, majority=True), wants)):
        _check(rec, want, (i, kinds[i]))


MAJORITY_MISTAKES = ["no_pad_rejection", "fields_from_voted_bits", "dcc_tolerance_0", "used_ok_sees_a_and_b_only", "agree_with_corrected"]
REFERENCE_MISTAKES = ["invalid_gives_repeat_0", "parity_flips_land_in_the_message"]


@pytest.mark.parametrize("wrong", MAJORITY_MISTAKES)
def test_a_wrong_majority_statement_disagrees_with_the_oracle(wrong):
    """the burst set can tell: a copy of decode_majority with one rule wrong is caught by the comparison the tests above make"""
    bursts, wants, kinds = majority_set()
    recs = oracle.decode_bursts(bursts, majority=True)
    caught = [i for i in range(len(bursts)) if _differs(recs[i], refdecode.decode_majority(bursts[i], wrong=wrong))]
    print(f"\n{wrong}: caught on {len(caught)} bursts, kinds {sorted({kinds[i] for i in caught})}")
    assert len(caught) >= 8


@pytest.mark.parametrize("wrong", REFERENCE_MISTAKES)
def test_a_wrong_word_dec_statement_disagrees_with_the_oracle(wrong):
    bursts, wants = reference_set()
    recs = oracle.decode_bursts(bursts)
    caught = [i for i in range(len(bursts)) if _differs(recs[i], refdecode.decode(bursts[i], wrong=wrong))]
    print(f"\n{wrong}: caught on {len(caught)} bursts")
    assert len(caught) >= 8


@pytest.mark.gpu
def test_hip_decode_equals_the_second_restatement(gpu):
    bursts = _bursts(96, 77)
    with capi.Recc(n_channels=1, max_bursts=8) as r:
        recs = r.decode_bursts(bursts)
    for i in range(len(bursts)):
        _check(recs[i], refdecode.decode(bursts[i]), i)
    bursts, wants = reference_set()                                # and the bursts steered into every first valid repeat and correction
    with capi.Recc(n_channels=1, max_bursts=8) as r:
        recs = r.decode_bursts(bursts)
    for i in range(len(bursts)):
        _check(recs[i], wants[i], i)


@pytest.mark.gpu
def test_hip_majority_decode_equals_the_second_statement(gpu):
    bursts, wants, kinds = majority_set()
    channels = (np.arange(len(bursts), dtype=np.uint32) * 7) % 5
    with capi.Recc(n_channels=1, max_bursts=8, majority=True) as r:
        plain = r.decode_bursts(bursts)
        tagged = r.decode_bursts(bursts, channels)
    for i in range(len(bursts)):
        _check(plain[i], wants[i], (i, kinds[i]))
        _check(tagged[i], wants[i], (i, kinds[i], "channels"))
        assert int(tagged[i]["channel"]) == int(channels[i]) and int(plain[i]["channel"]) == 0


# ------------------------------------------------------------------------------------------- the majority branch behind the capture kernels
IQ_SAMPLES, IQ_LIVE_CHANNELS = 80000, 12


def noisy_iq_block(n_channels, seed=1117):
    """complex64 [n_channels][80 000] at ten samples per symbol: two whole bursts (random messages) in each of at most twelve channels
    spread over the handle, at 5, 6 and 7 dB carrier to noise in the sampled 200 kHz, channel by channel, and noise alone at 6 dB
    everywhere else.  THE LEVEL IS CHOSEN: this seam has no channel filter in front of its discriminator, and at 9 to 11 dB in the
    sampled band the five repeats of a word never differ (CPU model: 0 of 28 records with an agree count below 5), while 9 to 11 dB
    referred to 30 kHz (0.8 to 2.8 dB per sample) loses nearly every trigger.  At 5 to 7 dB (13.2 to 15.2 dB in 30 kHz) the CPU
    model captures about four bursts in five and the vote has work in most of them.  Returns (iq, the live channels)."""
    from gr_amps_amd import synth
    rng = np.random.default_rng(seed)
    live = sorted({int(c) for c in np.linspace(0, n_channels - 1, min(n_channels, IQ_LIVE_CHANNELS))})
    iq = np.empty((n_channels, IQ_SAMPLES), np.complex64)
    for c in range(n_channels):
        bursts = []
        if c in live:
            off = 1500 + int(rng.integers(0, 997))
            for _ in range(2):
                _, _, _, _, words = synth.random_message(rng)
                bursts.append((off, synth.burst_bits(words, dcc=int(rng.integers(0, 4)), rng=rng)))
                off += 34560 + 2800 + int(rng.integers(0, 997))
            assert off - 2800 < IQ_SAMPLES
        iq[c] = synth.fsk_modulate(IQ_SAMPLES, bursts, sps=10, fs=200e3, snr_db=5.0 + live.index(c) % 3 if c in live else 6.0, rng=rng)
    return iq, live


def check_majority_captures(recs, blobs, twin_recs, twin_blobs, what):
    """every record of the majority handle is decode_majority of its own captured symbols, every record of the twin handle without the
    flag is decode of the same symbols; returns the share of records with a word that fewer than five repeats agree on"""
    assert len(recs) == len(blobs) == len(twin_recs) == len(twin_blobs) > 0, (what, len(recs), len(twin_recs))
    assert np.array_equal(blobs, twin_blobs) and np.array_equal(recs["position"], twin_recs["position"]) and \
        np.array_equal(recs["channel"], twin_recs["channel"]), what
    voted = 0
    for i in range(len(recs)):
        want = refdecode.decode_majority(blobs[i])
        _check(recs[i], want, (what, i, "majority"))
        _check(twin_recs[i], refdecode.decode(blobs[i]), (what, i, "reference"))
        voted += min(want["first_valid_rep"]) < 5
    return voted / len(recs)


@pytest.mark.gpu
@pytest.mark.parametrize("n_channels", [4, 66], ids=["queue", "workgroup"])
def test_hip_majority_captures_equal_the_second_statement(gpu, n_channels):
    """the majority branch behind the IQ seam's capture kernels (bits straight from the ring, packed records), in the form a handle of
    4 channels takes and in the one a handle of 66 takes: one push of noisy_iq_block, a silent push as flush, one drain"""
    iq, live = noisy_iq_block(n_channels)
    quiet = np.zeros((n_channels, 4096), np.complex64)
    got = []
    for majority in (True, False):
        with capi.Recc(n_channels=n_channels, sps=10, max_samples=IQ_SAMPLES, max_bursts=64, majority=majority, keep_bursts=True) as r:
            r.push_iq(iq)
            r.push_iq(quiet)
            got.append(r.drain_bursts())
    (recs, blobs), (twin_recs, twin_blobs) = got
    assert set(recs["channel"].tolist()) <= set(live)
    share = check_majority_captures(recs, blobs, twin_recs, twin_blobs, n_channels)
    print(f"\nIQ seam, {n_channels} channels: {len(recs)} records of {2 * len(live)} bursts, {share:.2f} of them with an agree count below 5")
    assert 3 * len(recs) >= 2 * len(live)                        # a third of what was sent at the least (CPU model: 8 of 8, 22 of 24)
    assert share >= 0.5                                            # the vote was exercised


# THE LEVEL IS CHOSEN: 8 dB carrier to noise in 30 kHz, the lowest point of scripts/majority_sensitivity.py (the synthesiser's floor is
# per 60 kHz: 3 dB less).  At that script's 11 dB point the repeats of a word hardly ever differ: on the float64 filter-bank model
# (oracle/channelizer.py) one record of eight at D = 768 and none of eight at D = 512 has an agree count below 5, at 9 dB three and
# four of eight; at 8 dB all eight at either decimation, and all eight bursts are still captured.
WB_LEVEL = 8.0 - 10.0 * np.log10(2.0)
WB_SAMPLES = 10000 * 768


@pytest.fixture(scope="module")
def noisy_band(gpu):
    """(0.25 s of band on the device with eight unimpaired bursts at WB_LEVEL, noise at that level over the whole band; their rows)"""
    import bitsref
    rows = (0, bitsref.ROWS - 1, (1023 - bitsref.FIRST) % 1024, (0 - bitsref.FIRST) % 1024, 100, 600, 37, 777)
    plants = [(bitsref.row_bin(row), 60000 + 230017 * i, 0.0, 0.0, WB_LEVEL) for i, row in enumerate(rows)]
    return bitsref.plant_bursts(WB_SAMPLES, plants, seed=1201, floor_db=WB_LEVEL, device=gpu)[0], rows


@pytest.mark.gpu
def test_hip_majority_captures_equal_the_second_statement_on_the_wideband_seam(gpu, decim, noisy_band):
    """the same behind the wideband seam's resolve kernel at both decimations: 0.25 s of band, eight unimpaired bursts at 8 dB carrier
    to noise in 30 kHz (WB_LEVEL, seed 1201; noise at that level over the whole band), a silent push, one drain; majority handle and its twin"""
    import bitsref
    import torch
    from conftest import wb_cfg
    (x, rows), quiet = noisy_band, torch.zeros(64 * decim, dtype=torch.complex64, device=gpu)
    wb, sps = wb_cfg(decim, bitsref.FIRST)
    got = []
    for majority in (True, False):
        with capi.Recc(n_channels=bitsref.ROWS, sps=sps, max_samples=WB_SAMPLES // decim + 64 + 72, max_bursts=512, wideband=wb,
                       majority=majority, keep_bursts=True) as r:
            r.push_wideband(x)
            r.push_wideband(quiet)
            got.append(r.drain_bursts())
    (recs, blobs), (twin_recs, twin_blobs) = got
    share = check_majority_captures(recs, blobs, twin_recs, twin_blobs, decim)
    print(f"\nwideband seam, D = {decim}: {len(recs)} records of 8 bursts, {share:.2f} of them with an agree count below 5")
    assert set(recs["channel"].tolist()) <= set(rows) and len(recs) >= 6
    assert share >= 0.5
