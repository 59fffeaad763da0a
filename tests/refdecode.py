"""A SECOND restatement of the reference's burst decode (R3, R5-R8), written separately from oracle/ref_chain.c and sharing no
code with it or with the kernels: plain Python over lists, the BCH verdict from tests/bchref.py (brute-force coset leaders + the
documented IT++ rule).  Two restatements written apart and agreeing on every field of every message class is what this repo can
offer in place of a reference-produced vector for the control flow of bursts_message (lib/recc_decode_impl.cc:81-169).

Each function cites the reference lines it follows.  Pure Python: for the handful of bursts the tests feed it."""
import bchref

_LEAD = None


def _leaders():
    global _LEAD
    if _LEAD is None:
        _LEAD = bchref.coset_leaders()
    return _LEAD


def manchester(sym, nbits):
    """lib/utils.cc:27-59: pairs (1,0) -> 0, (0,1) -> 1, (1,1) -> 0 + bad, (0,0) -> 1 + bad"""
    out, bad = [], 0
    for i in range(nbits):
        a, b = int(sym[2 * i]), int(sym[2 * i + 1])
        if (a, b) == (1, 1):
            out.append(0); bad += 1
        elif (a, b) == (0, 0):
            out.append(1); bad += 1
        elif (a, b) == (1, 0):
            out.append(0)
        else:
            assert (a, b) == (0, 1)
            out.append(1)
    return out, bad


def bch_valid(block48):
    """lib/recc_decode_impl.cc:53-79 returns itpp::BCH(63,2,true)::decode's flag on 15 zeros + the 48 bits: true when the
    word is within two flips of a code word, or in the S1 = 0 / S3-a-cube case IT++ also accepts; positions are not checked"""
    w = bchref.from_bits([0] * 15 + [int(b) & 1 for b in block48])
    r = bchref.polymod(w)
    if r in _leaders():
        return True
    return bchref.evaluate(w, 1) == 0 and bchref.is_cube(bchref.evaluate(w, 3))


def _get(bits, off, n):
    """amps_packet.h:118-143 get8 / get32 / get64: most significant bit first"""
    v = 0
    for i in range(n):
        v = (v << 1) | (int(bits[off + i]) & 1)
    return v


def extract_min_3(val):
    """amps_packet.h:277-302, quirks included (a leading digit above 9 prints as 0)"""
    m2 = val + 111
    d3 = m2 % 10
    m2 -= 10 if d3 == 0 else d3
    d2 = (m2 % 100) // 10
    m2 -= 100 if d2 == 0 else m2 % 100
    d1 = m2 // 100
    if d1 > 9:
        d1 = 0
    return "%d%d%d" % (d1, d2, d3)


def calc_min(min1, min2):
    """amps_packet.h:354-363"""
    thous = (min1 >> 10) & 0xF
    if thous > 9:
        thous = 0
    return extract_min_3(min2) + extract_min_3((min1 >> 14) & 0x3FF) + str(thous) + extract_min_3(min1 & 0x3FF)


def digits(word):
    """recc_word_called::digits, amps_packet.h:211-273: eight 4-bit codes, 0 ends, 13..15 end with a warning"""
    d, out, bad = _get(word, 4, 32), "", False
    for _ in range(8):
        v = (d >> 28) & 0xF
        if v == 0:
            break
        if v >= 13:
            bad = True
            break
        out += "0" if v == 10 else "*" if v == 11 else "#" if v == 12 else str(v)
        d = (d << 4) & 0xFFFFFFFF
    return out, bad


INVALID_WORD_A, E_ZERO, PAGE_RESPONSE, REGISTRATION, ORIGINATION, BAD_NAWC, UNKNOWN = range(7)


def bch_correct(block48):
    """lib/recc_decode_impl.cc:53-79 with the corrections kept: (flag, the 63 bits after correction, flips among the 15 leading zeros, which rule: "leader" / "three" / None).
    The 63-bit word is 15 zeros in front of the 48 bits, in transmitted order; decoded(15, 50) of :68 are entries 15..50 of it.  The
    flips are the coset leader's (weight <= 2), or, in the S1 = 0 / S3-a-cube case IT++ also accepts, the three positions p (as
    exponents of x) with alpha^(3 p) = S3.  A word that does not decode is returned as received."""
    padded = [0] * 15 + [int(b) & 1 for b in block48]
    w = bchref.from_bits(padded)
    r = bchref.polymod(w)
    if r in _leaders():
        err, rule = _leaders()[r][1], "leader"
    elif bchref.evaluate(w, 1) == 0 and bchref.is_cube(bchref.evaluate(w, 3)):
        s3 = bchref.evaluate(w, 3)
        err = sum(1 << p for p in range(63) if bchref.EXP[(3 * p) % 63] == s3)
        assert bin(err).count("1") == 3
        rule = "three"
    else:
        return False, padded, 0, None
    flips = bchref.bits(err)
    return True, [a ^ b for a, b in zip(padded, flips)], sum(flips[:15]), rule


def _dispatch(out, W, valid_a):
    """The field parse and the branches of bursts_message, lib/recc_decode_impl.cc:108-168, on the seven words W (the parsers read
    bits 0..35 only).  Fills `out`; returns the indices of the words the dispatch read, in order."""
    A, B = W[0], W[1]
    a = {"F": A[0], "NAWC": _get(A, 1, 3), "T": A[4], "S": A[5], "E": A[6], "ER": A[7], "SCM": _get(A, 8, 4), "MIN1": _get(A, 12, 24)}
    b = {"F": B[0], "NAWC": _get(B, 1, 3), "MSG_TYPE": _get(B, 4, 5), "ORDQ": _get(B, 9, 3), "ORDER": _get(B, 12, 5), "LT": B[17],
         "EP": B[18], "SCM4": B[19], "MPCI": _get(B, 20, 2), "SDCC1": _get(B, 22, 2), "SDCC2": _get(B, 24, 2), "MIN2": _get(B, 26, 10)}
    out.update(a=a, b=b, min=calc_min(a["MIN1"], b["MIN2"]))
    read = [0, 1]
    zero_order = b["ORDER"] == 0 and b["ORDQ"] == 0 and b["MSG_TYPE"] == 0
    if not valid_a:                                                             # :108-111
        out["cls"] = INVALID_WORD_A
    elif not a["E"]:                                                            # :113-116
        out["cls"] = E_ZERO
    elif a["T"] == 0 and zero_order:                                            # :121-122
        out["cls"] = PAGE_RESPONSE
    elif a["T"] == 1 and b["ORDER"] == 0xD:                                     # :123-138
        out["cls"] = REGISTRATION
        out["has_esn"] = a["S"]
        if a["S"] and a["NAWC"] > 1:
            c = W[2]; read.append(2)
            out["esn"] = _get(c, 4, 32)
            out["nawc_mismatch"] = _get(c, 1, 3) != ((a["NAWC"] - 2) & 0xFF)
    elif a["T"] == 1 and (a["NAWC"] > 2 or zero_order):                         # :139-165
        nawc, nxt = a["NAWC"], 2
        out["has_esn"] = a["S"]
        if a["S"]:
            c = W[nxt]; read.append(nxt); nxt += 1
            out["esn"] = _get(c, 4, 32)
            nawc = (a["NAWC"] - 2) & 0xFF                                       # unsigned char arithmetic
            out["nawc_mismatch"] = _get(c, 1, 3) != nawc
        if nawc < 1 or nawc > 4:                                                # :155-158
            out["cls"] = BAD_NAWC
        else:
            out["cls"] = ORIGINATION
            while nawc > 0:
                d, bad = digits(W[nxt]); read.append(nxt); nxt += 1
                out["dialed"] += d
                out["bad_digit"] = out["bad_digit"] or bad
                out["n_called_words"] += 1
                nawc -= 1
    else:                                                                       # :166-168
        out["cls"] = UNKNOWN
    return read


def _front(burst):
    """:90-100: the coded DCC and the seven words of 240 bits, with their counts of bad Manchester pairs"""
    sym = [int(x) for x in burst]
    dcc, dcc_bad = manchester(sym[0:14], 7)                                    # :90-91
    words, errs = [], []
    for i in range(7):                                                          # :97-100
        w, e = manchester(sym[14 + 480 * i:14 + 480 * (i + 1)], 240)
        words.append(w); errs.append(e)
    out = {"dcc": dcc, "dcc_bad": dcc_bad, "manch_bad": errs, "dcc_invalid": False,
           "esn": 0, "has_esn": 0, "dialed": "", "n_called_words": 0, "nawc_mismatch": False, "bad_digit": False}
    return out, words


def decode(burst, wrong=None):
    """bursts_message, lib/recc_decode_impl.cc:81-169, on the 3374 symbol bytes of one burst.  Returns a dict of everything
    the message handlers are given (and of what the product's record exposes on the way: word_raw = repeat 0 of every word as
    received, word_dec = decwords[w][0..35] of :102, the decoder's message bits of the repeat the loop of :101-106 stopped at --
    the first valid one, corrected, or repeat 4, which include/amps_recc.h gives as received where no repeat is valid).
    `wrong` names a planted mistake (tests/test_second_restatement.py: the bursts must be able to tell); never set otherwise."""
    out, words = _front(burst)
    valid, first, dec, spill, fixes = [], [], [], [], []
    for w in range(7):                                                          # :101-108: stop at the first valid repeat
        ok, rep = False, 5
        for r in range(5):
            if bch_valid(words[w][48 * r:48 * r + 48]):
                ok, rep = True, r
                break
        valid.append(ok); first.append(rep)
        last = words[w][48 * min(rep, 4):48 * min(rep, 4) + 48]
        if wrong == "invalid_gives_repeat_0" and not ok:
            last = words[w][0:48]
        flag, fixed, in_pad, _ = bch_correct(last)
        assert flag == ok
        fixes.append((sum(fixed[15 + i] != last[i] for i in range(36)), sum(fixed[15 + i] != last[i] for i in range(36, 48)), in_pad) if ok else None)
        spill.append([i for i in range(36, 48) if ok and fixed[15 + i] != last[i]])
        dec.append(fixed[15:51])
    if wrong == "parity_flips_land_in_the_message":
        # a flip in the parity, applied as "bit i of the word's 36" without asking whether i < 36, lands in the word behind it
        for w in range(6):
            for i in spill[w]:
                dec[w + 1][i - 36] ^= 1
    out.update(valid=valid, first_valid_rep=first, word_raw=[w[0:48] for w in words], word_dec=dec,
               fixes=fixes)                                                     # fixes: (in the message, in the parity, in the zeros) per valid word: for the tests' conditions
    _dispatch(out, words, valid[0])                                             # the parsers read repeat 0 as received (:112, :117)
    return out


DCC_CODES = ([0, 0, 0, 0, 0, 0, 0], [0, 0, 1, 1, 1, 1, 1], [1, 1, 0, 0, 0, 1, 1], [1, 1, 1, 1, 1, 0, 0])


def decode_majority(burst, wrong=None):
    """The product's majority mode, from the "Decode modes" paragraph and the amps_recc_burst_t field comments of include/amps_recc.h
     alone: a 3-of-5 vote per bit position of every word; ONE decode of the voted word, valid only if it decodes
    and no flip lies in the 15 shortening positions; word_raw = the voted bits, first_valid_rep = the number of repeats equal to
    them; word_dec = the voted word's message bits, corrected where the word is valid and as voted where it is not; fields and
    dispatch from word_dec; class INVALID_WORD_A where a word that the dispatch read is invalid and the class would be
    PAGE_RESPONSE or later; dcc_invalid where the coded DCC is more than one bit from every code word.
    `wrong` names a planted mistake, as in decode()."""
    out, words = _front(burst)
    valid, agree, raw, dec, verdict = [], [], [], [], []
    for w in range(7):
        reps = [words[w][48 * r:48 * r + 48] for r in range(5)]
        voted = [1 if sum(rep[i] for rep in reps) >= 3 else 0 for i in range(48)]
        flag, fixed, in_pad, rule = bch_correct(voted)
        verdict.append("fail" if not flag else rule + ("_pad" if in_pad else "_ok"))
        ok = flag and (in_pad == 0 or wrong == "no_pad_rejection")
        msg = fixed[15:51] if ok else voted[0:36]
        against = voted if wrong != "agree_with_corrected" else (fixed[15:63] if ok else voted)
        raw.append(voted); dec.append(msg); valid.append(ok)
        agree.append(sum(rep == against for rep in reps))
    out.update(valid=valid, first_valid_rep=agree, word_raw=raw, word_dec=dec)
    read = _dispatch(out, raw if wrong == "fields_from_voted_bits" else dec, valid[0])
    if wrong == "used_ok_sees_a_and_b_only":
        read = [0, 1]
    if out["cls"] >= PAGE_RESPONSE and not all(valid[w] for w in read):
        out["cls"] = INVALID_WORD_A
    dist = min(sum(x != y for x, y in zip(out["dcc"], code)) for code in DCC_CODES)
    out["dcc_invalid"] = dist > (0 if wrong == "dcc_tolerance_0" else 1)
    out.update(dcc_distance=dist, verdict=verdict, read=read)                   # for the tests' conditions
    return out
