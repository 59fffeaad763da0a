"""Holds the oracle (oracle/ref_chain.c) and the second restatements (tests/reccwork2.py, tests/refdecode.py) to what the REFERENCE'S OWN
COMPILED CODE produced: tests/golden/reference_compiled.npz, made by tests/golden/make_reference_compiled.py from oracle/_ref/refdriver
(the reference's recc_impl.cc, recc_decode_impl.cc, amps_packet.cc and utils.cc compiled in place against the stand-in headers of
oracle/refshim/).  Every comparison is exact: integers and strings.  Only the BCH verdict inside the reference build is a stand-in
(a table decoder of this repository, held to tests/bchref.py below); the GNU Radio float blocks are not on this path.

Reads the committed file only -- except the last three tests, which need oracle/_ref/refdriver and skip where it is not built."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bchref
import oracle
import reccwork2
import refcompiled
import refdecode

HERE = os.path.dirname(os.path.abspath(__file__))
GENERATOR = os.path.join(HERE, "golden", "make_reference_compiled.py")
needs_driver = pytest.mark.skipif(not os.path.exists(oracle.REFDRIVER), reason="oracle/_ref/refdriver is not built: the reference's sources are not on this machine")


@pytest.fixture(scope="module")
def fx():
    return refcompiled.fixture()


# ------------------------------------------------------------------------------------------------ R1 / R2: recc_impl::work
def test_oracle_work_publishes_what_the_reference_published(fx):
    for i, (name, si, sched) in enumerate(fx.cases):
        got = [(c, bytes(b)) for c, b in oracle.Recc().run(fx.streams[si], sched)]
        assert got == fx.pubs[i], (name, sched)
    assert sum(len(p) for p in fx.pubs) >= 100


def test_second_restatement_of_work_publishes_what_the_reference_published(fx):
    for i, (name, si, sched) in enumerate(fx.cases):
        assert reccwork2.ReccWork2().run(fx.streams[si], sched) == fx.pubs[i], (name, sched)


def test_the_fixture_holds_the_recorded_stream_outcomes(fx):
    """SURVEY.md 8a (Q1 - Q4), now from a file anyone with the reference's sources can rebuild"""
    n = lambda name, sched: len(fx.pubs[fx.case(name, sched)])       # noqa: E731
    assert [n("q2", [c]) for c in (1000, 4096, 333, 8191)] == [3, 3, 3, 2]
    assert n("pin sym_q1_short_tail", [4096]) == 0 and n("pin sym_q1_one_more", [4096]) == 1
    assert n("first fill 63000", [4096]) == 0 and n("first fill 60000", [4096]) == 1
    assert n("first fill 62087", [4096]) == 1 and n("first fill 62088", [4096]) == 0      # 62 088 + 74 + 3374 = 65 536: one symbol short
    assert (n("q3 lost", [1000]), n("q3 ghost", [1000]), n("same call", [1000])) == (1, 2, 1)
    assert all(n("edge %d" % k, [512]) == 1 for k in range(74))


def test_trigger_is_the_one_the_reference_constructor_built(fx):
    want = fx.z["fld_out_trigger"]
    assert want.size == 74
    assert np.array_equal(oracle.trigger(), want) and reccwork2.TRIGGER == want.tobytes()


# ------------------------------------------------------------------------------------------------ R3, R5 - R8: bursts_message and the replies
def test_oracle_decode_equals_the_reference(fx):
    recs = oracle.decode_bursts(fx.bursts)
    for i in range(len(fx.bursts)):
        refcompiled.check_record(recs[i], fx.expected_record(i), i)
    assert set(fx.z["dec_class"].tolist()) == set(range(7))


def test_oracle_reply_words_equal_the_messages_the_reference_published(fx):
    recs = oracle.decode_bursts(fx.bursts)
    for i in range(len(fx.bursts)):
        assert refcompiled.reply_lines(oracle.reply_words(recs[i])) == fx.lines[i], i
    assert sum(1 for l in fx.lines if l) >= 100
    # the origination that dials 0... gets the general word 2 (order 9), every other one a voice channel
    zero = [i for i in range(len(fx.bursts)) if fx.z["dec_class"][i] == refcompiled.ORIGINATION and fx.z["dec_dialed"][i].startswith(b"0")]
    other = [i for i in range(len(fx.bursts)) if fx.z["dec_class"][i] == refcompiled.ORIGINATION and not fx.z["dec_dialed"][i].startswith(b"0")]
    assert len(zero) >= 4 and len(other) >= 12
    assert {fx.lines[i][0].split("w2=")[1][:4] for i in zero} == {"1011"} and {fx.lines[i][0].split("w2=")[1][:4] for i in other} == {"1001"}


def _second_restatement_differences(fx):
    """[(burst, field)] where tests/refdecode.py and the reference disagree"""
    out = []
    for i in range(len(fx.bursts)):
        d = refdecode.decode(fx.bursts[i])
        got = {"msg_class": d["cls"], "dcc": d["dcc"], "dcc_bad": d["dcc_bad"], "manch_bad": d["manch_bad"], "nawc_mismatch": d["nawc_mismatch"],
               "bad_digit": d["bad_digit"], "min": d["min"], "esn": d["esn"], "has_esn": int(d["has_esn"]), "dialed": d["dialed"],
               "n_called_words": d["n_called_words"]}
        got.update({"a_" + k: int(v) for k, v in d["a"].items()})
        got.update({"b_" + k: int(v) for k, v in d["b"].items()})
        out += [(i, k) for k, v in fx.expected_record(i).items() if got[k] != v]
    return out


def test_second_restatement_of_the_decode_equals_the_reference(fx):
    assert _second_restatement_differences(fx) == []


def _digits_reading_on(word):
    """digits() with one rule wrong: a code 0 is skipped, not the end"""
    d, out = refdecode._get(word, 4, 32), ""
    for p in range(8):
        v = (d >> (28 - 4 * p)) & 0xF
        if v >= 13:
            return out, True
        if v:
            out += "0" if v == 10 else "*" if v == 11 else "#" if v == 12 else str(v)
    return out, False


def _calc_min_modulo_ten(min1, min2):
    """calc_min with one rule wrong: a thousands code above 9 printed modulo ten, not as 0"""
    return refdecode.extract_min_3(min2) + refdecode.extract_min_3((min1 >> 14) & 0x3FF) + str(((min1 >> 10) & 0xF) % 10) + refdecode.extract_min_3(min1 & 0x3FF)


@pytest.mark.parametrize("name, wrong", [("digits", _digits_reading_on), ("calc_min", _calc_min_modulo_ten)])
def test_a_wrong_rule_in_the_second_restatement_disagrees_with_the_reference(fx, monkeypatch, name, wrong):
    """the fixture can tell: the restatement with one rule planted wrong differs from the reference's outputs on several bursts"""
    monkeypatch.setattr(refdecode, name, wrong)
    bursts = {i for i, _ in _second_restatement_differences(fx)}
    assert len(bursts) >= 4, sorted(bursts)


# ------------------------------------------------------------------------------------------------ words and values
def _as_bursts(a, b):
    """bursts whose words A and B carry the given 48 bits in repeat 0 (everything else zero bits): the oracle parses repeat 0 as received"""
    bits = np.zeros((len(a), 7 + 7 * 240), np.uint8)
    bits[:, 7:55], bits[:, 247:295] = a, b
    sym = np.empty((len(a), 2 * bits.shape[1]), np.uint8)
    sym[:, 0::2], sym[:, 1::2] = 1 - bits, bits
    return sym


def test_word_parsers_equal_the_reference(fx):
    a, b, c, d = (fx.words(k) for k in "abcd")
    recs = oracle.decode_bursts(_as_bursts(a, b))
    for i in range(len(a)):
        assert [int(recs[i]["a_" + k]) for k in refcompiled.A_FIELDS] == fx.z["fld_out_a"][i].tolist(), i
        assert [int(recs[i]["b_" + k]) for k in refcompiled.B_FIELDS] == fx.z["fld_out_b"][i].tolist(), i
        wa, wb = {}, {}
        refdecode._dispatch(wa, [a[i].tolist(), b[i].tolist()] + [[0] * 240] * 5, False)
        assert [wa["a"][k] for k in refcompiled.A_FIELDS] == fx.z["fld_out_a"][i].tolist(), i
        assert [wa["b"][k] for k in refcompiled.B_FIELDS] == fx.z["fld_out_b"][i].tolist(), i
    for i in range(len(c)):                                        # recc_word / recc_word_c_serial: F, NAWC, SERIAL
        w = c[i].tolist()
        assert [w[0], refdecode._get(w, 1, 3), refdecode._get(w, 4, 32)] == fx.z["fld_out_c"][i].tolist(), i
    seen = set()
    for i in range(len(d)):                                        # recc_word_called and digits(), every code in every position
        w = d[i].tolist()
        f, nawc, digits, bad = (int(x) for x in fx.z["fld_out_d"][i])
        text = fx.z["fld_out_d_digits"][i].decode()
        assert [w[0], refdecode._get(w, 1, 3), refdecode._get(w, 4, 32)] == [f, nawc, digits], i
        assert oracle.called_digits(digits) == (text, bool(bad)), i
        assert refdecode.digits(w) == (text, bool(bad)), i
        seen |= {(p, (digits >> (28 - 4 * p)) & 0xF) for p in range(8)}
    assert seen == {(p, v) for p in range(8) for v in range(16)}


def test_min_arithmetic_equals_the_reference(fx):
    z = fx.z
    assert [refdecode.extract_min_3(v) for v in range(1024)] == [s.decode() for s in z["fld_out_extract_min_3"]]
    for v in range(1024):                                          # the oracle's extract_min_3 through calc_min's first three digits
        assert oracle.calc_min(0, v)[:3] == z["fld_out_extract_min_3"][v].decode(), v
    for s, (ok, min1, min2), back in zip(z["fld_min_strings"], z["fld_out_parse_min"], z["fld_out_parse_min_back"]):
        assert ok == 1 and oracle.parse_min(s.decode()) == (int(min1), int(min2)), s
        assert oracle.calc_min(int(min1), int(min2)) == back.decode() == refdecode.calc_min(int(min1), int(min2)), s
    for (min1, min2), want in zip(z["fld_calc_min_args"], z["fld_out_calc_min"]):
        assert oracle.calc_min(int(min1), int(min2)) == want.decode() == refdecode.calc_min(int(min1), int(min2)), (min1, min2)
    assert {(int(m) >> 10) & 0xF for m, _ in z["fld_calc_min_args"]} == set(range(16))


def test_word_builders_equal_the_reference(fx):
    z = fx.z
    for (multi, dcc, min1), want in zip(z["fld_focc_word1_args"], z["fld_out_focc_word1"]):
        assert oracle.focc_word1(int(multi), int(dcc), int(min1)) == want.decode()
    for (min2, t, q, o), want in zip(z["fld_focc_word2_general_args"], z["fld_out_focc_word2_general"]):
        assert oracle.focc_word2_general(int(min2), int(t), int(q), int(o)) == want.decode()
    for (scc, min2, vmac, chan), want in zip(z["fld_focc_word2_voice_channel_args"], z["fld_out_focc_word2_voice_channel"]):
        assert oracle.focc_word2_voice_channel(int(scc), int(min2), int(vmac), int(chan)) == want.decode()
    for (pscc, t, q, o), want in zip(z["fld_fvc_word1_general_args"], z["fld_out_fvc_word1_general"]):
        assert oracle.fvc_word1_general(int(pscc), int(t), int(q), int(o)) == want.decode()


def test_manchester_decoder_equals_the_reference(fx):
    pairs = set()
    for sym, bits, bad in fx.manchester_buffers():
        got, nbad, nonbinary = oracle.manchester_decode(sym, bits.size)
        assert np.array_equal(got, bits) and nbad == bad and not nonbinary
        assert refdecode.manchester(sym, bits.size) == (bits.tolist(), bad)
        pairs |= set(zip(sym[0::2].tolist(), sym[1::2].tolist()))
    assert pairs == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_survey_kats_are_reproduced_by_the_compiled_reference(fx):
    """the nine known-answer values the survey typed into survey_kats.json are among the driver's outputs: their provenance is checkable"""
    z, k = fx.z, json.load(open(os.path.join(HERE, "golden", "survey_kats.json")))
    mins = [s.decode() for s in z["fld_min_strings"]]
    for e in k["parse_min"]:
        i = mins.index(e["min"])
        assert z["fld_out_parse_min"][i].tolist() == [1, int(e["MIN1"], 16), int(e["MIN2"], 16)]

    def built(key, args):
        rows = [i for i, r in enumerate(z["fld_" + key + "_args"]) if [int(x) for x in r] == args]
        assert rows, (key, args)
        return z["fld_out_" + key][rows[0]].decode()
    e = k["focc_word1"][0]
    assert built("focc_word1", [e["multi"], e["dcc"], int(e["MIN1"], 16)]) == e["bits"]
    e = k["focc_word2_voice_channel"][0]
    assert built("focc_word2_voice_channel", [e["scc"], int(e["MIN2"], 16), e["vmac"], e["chan"]]) == e["bits"]
    e = k["focc_word2_general"][0]
    assert built("focc_word2_general", [int(e["MIN2"], 16), e["msg_type"], e["ordq"], e["order"]]) == e["bits"]
    e = k["manchester_decode_binbuf"][0]
    sym, bits, bad = fx.manchester_buffers()[0]
    assert sym.tolist() == e["symbols"] and "".join(str(b) for b in bits) == e["bits"] and bad == e["bad"]
    bits = np.array([int(c) for c in k["trigger_bits"]], np.uint8)
    assert np.array_equal(z["fld_out_trigger"][0::2], 1 - bits) and np.array_equal(z["fld_out_trigger"][1::2], bits)
    e = k["called_digits"][0]
    rows = [i for i, r in enumerate(z["fld_out_d"]) if int(r[2]) == int(e["DIGITS"], 16)]
    assert rows and z["fld_out_d_digits"][rows[0]].decode() == e["digits"]


# ------------------------------------------------------------------------------------------------ the stand-in BCH inside the reference build
def test_stand_in_bch_equals_the_brute_force_reference_on_all_4096_syndromes(fx):
    z = fx.z
    words = np.unpackbits(z["bch_word_bits"], axis=1)[:, :63]
    msgs = np.unpackbits(z["bch_message_bits"], axis=1)[:, :51]
    lead = bchref.coset_leaders()
    seen, three = set(), 0
    for i in range(len(words)):
        w = bchref.from_bits(words[i])
        r = bchref.polymod(w)
        seen.add(r)
        if r in lead:
            ok, err = True, lead[r][1]
        elif bchref.evaluate(w, 1) == 0 and bchref.is_cube(bchref.evaluate(w, 3)):
            s3 = bchref.evaluate(w, 3)
            ok, err = True, sum(1 << p for p in range(63) if bchref.EXP[(3 * p) % 63] == s3)
            three += 1
        else:
            ok, err = False, 0
        assert bool(z["bch_ok"][i]) == ok and int(z["bch_error"][i]) == err, (i, r)
        assert msgs[i].tolist() == bchref.bits(w ^ err)[:51], i
    assert len(seen) == 4096 and three == 21 and int(z["bch_ok"].sum()) == 2017 + 21


@needs_driver
def test_reference_driver_links_nothing_of_the_oracle():
    """the dispatch comparison would be circular on the verdict if the stand-in decoder called the oracle's"""
    for exe in (oracle.REFDRIVER, oracle.REFDRIVER_SAN):
        syms = subprocess.run(["nm", "-C", exe], capture_output=True, text=True, check=True).stdout
        assert "orc_" not in syms and "recc_decode_impl" in syms


@needs_driver
def test_the_fixture_rebuilds_byte_for_byte():
    r = subprocess.run([sys.executable, GENERATOR, "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@needs_driver
def test_sanitized_driver_runs_the_whole_input_set_clean():
    """oracle/_ref/refdriver_san (AddressSanitizer + UndefinedBehaviorSanitizer, -fno-sanitize-recover=all; a stand-alone program) over
    every input of the fixture: it must end without a report and write what the plain build wrote"""
    sys.path.insert(0, os.path.dirname(GENERATOR))
    try:
        import make_reference_compiled as gen
    finally:
        sys.path.pop(0)
    inp = gen.inputs()
    san, plain = gen.run_all(inp, oracle.REFDRIVER_SAN), gen.run_all(inp, oracle.REFDRIVER)      # a report ends the program with a status: run_driver raises
    for k in ("work", "decode", "fields", "bch"):
        assert san[k] == plain[k], k
