"""Builds tests/golden/reference_compiled.npz: inputs made from seeds, and what the REFERENCE'S OWN COMPILED CODE makes of them.

oracle/_ref/refdriver (oracle/Makefile, target _ref: the reference's recc_impl.cc, recc_decode_impl.cc, amps_packet.cc and utils.cc
compiled in place against the stand-in headers of oracle/refshim/, with oracle/refdriver.cc) is run on every input; the file keeps the
inputs and the driver's outputs, nothing else.  The oracle, the second restatements and the kernels are NOT consulted for any
expected value: tests/test_cpu_reference_compiled.py and tests/test_gpu_reference_compiled.py hold them to this file.

    python tests/golden/make_reference_compiled.py            writes the file   (needs oracle/_ref/refdriver)
    python tests/golden/make_reference_compiled.py --check    rebuilds it in memory and compares every array byte for byte

Before anything is written the coverage is asserted FROM THE REFERENCE'S OUTPUTS (main(): every message class eight times or more,
the Q1 - Q4 stream outcomes SURVEY.md 8a recorded, and streams on which the reference's search rule and a naive "search everything"
rule differ).  Symbols and bits are stored packed (np.packbits)."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PATH = os.path.join(HERE, "reference_compiled.npz")
DRIVER = os.path.join(ROOT, "oracle", "_ref", "refdriver")
CAPTURE, TRIGGER_LEN = 3374, 74
TRIGGER_BITS = "1010101010101010101010101011100010010"          # tests/golden/survey_kats.json "trigger_bits"
CLASS_NAMES = ["invalid_word_a", "e_zero", "page_response", "registration", "origination", "bad_nawc", "unknown"]

# record tags of `refdriver fields` (oracle/refdriver.cc)
TAG_A, TAG_B, TAG_C, TAG_D, TAG_X3, TAG_PM, TAG_CM, TAG_W1, TAG_W2G, TAG_W2V, TAG_FVC, TAG_MD, TAG_TRIG = range(1, 14)


def trigger():
    t = np.array([int(c) for c in TRIGGER_BITS], np.uint8)
    out = np.empty(2 * t.size, np.uint8)
    out[0::2], out[1::2] = 1 - t, t                              # '0' -> (1,0), '1' -> (0,1)
    return out


# ------------------------------------------------------------------------------------------------ running the driver
def run_driver(mode, payload, driver=DRIVER, text=True):
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            f.write(payload)
        r = subprocess.run([driver, mode, src, dst], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        if r.returncode != 0:
            raise RuntimeError("%s %s: exit status %d\n%s" % (os.path.basename(driver), mode, r.returncode, r.stderr.decode()[-4000:]))
        with open(dst, "rb") as f:
            out = f.read()
    return out.decode().splitlines() if text else out


def expand(schedule, n):
    """the chunk sizes a cycled schedule cuts a stream of n symbols into (oracle.Recc.run, ReccWork2.run)"""
    sizes, off, k = [], 0, 0
    while off < n:
        c = min(int(schedule[k % len(schedule)]), n - off)
        sizes.append(c)
        off += c
        k += 1
    return sizes


def work_payload(streams, cases):
    out = []
    for si, sched in cases:
        s = streams[si]
        sizes = expand(sched, s.size)
        out.append(np.array([s.size, len(sizes)] + sizes, "<u4").tobytes() + s.tobytes())
    return b"".join(out)


def parse_work(blob):
    rec = np.dtype([("case", "<u4"), ("call", "<u4"), ("payload", "u1", (CAPTURE,))])
    assert len(blob) % rec.itemsize == 0
    return np.frombuffer(blob, rec)


# ------------------------------------------------------------------------------------------------ streams for `work`
def _burst_stream(seed, n, offs):
    from gr_amps_amd import synth
    rng = np.random.default_rng(seed)
    b = []
    for o in offs:
        _, _, _, _, w = synth.random_message(rng)
        b.append((o, synth.burst_bits(w, dcc=int(rng.integers(0, 4)), rng=rng)))
    return synth.symbol_stream(n, b, rng)


def _planted(seed, n, starts, damaged=()):
    """random symbols with the trigger at `starts` (in order: a later one overwrites an earlier one where they overlap);
    those at `damaged` have one symbol flipped"""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 2, n).astype(np.uint8)
    for p in starts:
        s[p:p + TRIGGER_LEN] = trigger()
    for p in damaged:
        s[p:p + TRIGGER_LEN] = trigger()
        s[p + int(rng.integers(0, TRIGGER_LEN))] ^= 1
    return s


def make_streams():
    """([stream], [name], [(name, stream index, schedule)])"""
    streams, names, cases = [], [], []

    def add(name, s):
        assert set(np.unique(s)) <= {0, 1}
        streams.append(np.ascontiguousarray(s, np.uint8))
        names.append(name)
        return len(streams) - 1

    pins = np.load(os.path.join(HERE, "pin_inputs.npz"))
    for key in sorted(k for k in pins.files if k.startswith("sym_")):
        cases.append(("pin " + key, add("pin " + key, pins[key]), [4096]))
    spaced = names.index("pin sym_spaced")
    # Q2: three bursts 9456 symbols apart (the stream of tests/golden/make_golden.py)
    q2 = add("q2", _burst_stream(1, 40000, [4743, 4743 + 9456, 4743 + 2 * 9456]))
    for c in (1000, 4096, 333, 8191):
        cases.append(("q2", q2, [c]))
    # Q3, chunk 1000: the burst at 500 is published in call 3, which leaves bytes 3427..3499 of the buffer stale.
    #   lost:  a real trigger over the edge of calls 3 and 4 (ten symbols before it): its head went to the front of the buffer
    #   ghost: ten symbols of trigger at 3490 and the other 64 at 4000: no trigger in the stream, one in the buffer
    s = _planted(31, 9000, [500, 3990])
    cases.append(("q3 lost", add("q3 lost", s), [1000]))
    s = _planted(32, 9000, [500])
    s[3490:3500], s[4000:4064] = trigger()[:10], trigger()[10:]
    cases.append(("q3 ghost", add("q3 ghost", s), [1000]))
    # a trigger that is complete in the call that completes a capture (call 3: the burst at 400 ends at 3848, the trigger at 3900)
    cases.append(("same call", add("same call", _planted(33, 9000, [400, 3900])), [1000]))
    # overlapping triggers, a trigger inside a capture, a trigger damaged in one symbol
    s = _planted(34, 16000, [300, 308, 2000, 5000, 5040, 9000], damaged=[12000])
    ov = add("overlap damaged", s)
    for c in ([333], [4096], [75, 3449]):
        cases.append(("overlap damaged", ov, c))
    # the capture ends 3374 and 3375 symbols behind the trigger (strictly more than 3374 are needed)
    for extra in (0, 1):
        s = _planted(35, 700 + TRIGGER_LEN + CAPTURE + extra, [700])
        si = add("tail %d" % (CAPTURE + extra), s)
        for c in ([333], [4096]):
            cases.append(("tail %d" % (CAPTURE + extra), si, c))
    # the trigger's first symbol at each of the 74 offsets against a chunk edge (chunk 512, edge at 1024)
    for k in range(TRIGGER_LEN):
        p = 1024 - (TRIGGER_LEN - 1) + k
        cases.append(("edge %d" % k, add("edge %d" % k, _planted(1000 + k, 4700, [p])), [512]))
    # first fill of the 65 536-symbol buffer (Q4).  62 087 / 62 088: the capture's 3375th symbol is the buffer's last / the first
    # one that does not fit any more (62 088 + 74 + 3374 = 65 536)
    for p in (60000, 61439, 61440, 62087, 62088, 63000, 64500, 65462):
        cases.append(("first fill %d" % p, add("first fill %d" % p, _planted(2000 + p, 73728, [p])), [4096]))
    # schedules
    small = add("small", _planted(36, 4200, [300]))
    for c in (1, 73, 74, 75, 333, 3374, 3375, 3448, 3449):
        cases.append(("small", small, [c]))
    for c in (73, 3374, 3375, 3448, 3449):
        cases.append(("q2", q2, [c]))
    rng = np.random.default_rng(37)
    for c in ([8191], [61439], [61439, 1, 73, 74, 75, 333, 3374, 3375, 3448, 3449, 8191], [int(x) for x in rng.integers(1, 9000, 23)]):
        cases.append(("pin sym_spaced", spaced, c))
    return streams, names, cases


def naive_count(s):
    """what a rule that searches everything would publish: every trigger not inside a capture, if 3375 symbols follow it"""
    raw, t, n, at = bytes(s), bytes(trigger()), 0, 0
    while True:
        p = raw.find(t, at)
        if p < 0 or len(raw) - p - TRIGGER_LEN <= CAPTURE:
            return n
        n += 1
        at = p + TRIGGER_LEN + CAPTURE


# ------------------------------------------------------------------------------------------------ bursts for `decode`
def steered_bursts():
    """forty bursts steered at what only the reply code and the dispatch's arithmetic see; every word clean, five equal repeats"""
    import test_second_restatement as t2
    rng = np.random.default_rng(4040)
    bits = t2._bits

    def rnd(n):
        return int(rng.integers(0, 1 << n))

    def word_a(nawc, T, S, min1=None):
        return [1] + bits(nawc, 3) + [T, S, 1, 0] + bits(rnd(4), 4) + bits(rnd(24) if min1 is None else min1, 24)

    def word_b(order=0, ordq=0, mtype=0):
        return [0] + bits(rnd(3), 3) + bits(mtype, 5) + bits(ordq, 3) + bits(order, 5) + bits(rnd(3), 3) + bits(rnd(6), 6) + bits(rnd(10), 10)

    def word_c(nawc):
        return [0] + bits(nawc, 3) + bits(rnd(32), 32)

    def word_d(codes):
        d = 0
        for c in codes:
            d = (d << 4) | c
        return [0] + bits(rnd(3), 3) + bits(d, 32)

    def filler():
        return word_d([int(rng.integers(1, 13)) for _ in range(8)])

    def burst(words):
        words = words + [filler() for _ in range(7 - len(words))]
        return t2._symbols(rng, [int(x) for x in rng.integers(0, 2, 7)], [[t2._cw(w)] * 5 for w in words], 0)

    out = []
    for first in [10] + list(range(1, 10)) + [11, 12]:           # originations whose first digit is 0, 1 - 9, *, #
        out.append(burst([word_a(1, 1, 0), word_b(), word_d([first] + [int(rng.integers(1, 13)) for _ in range(7)])]))
    out.append(burst([word_a(1, 1, 0), word_b(), word_d([0] * 8)]))                      # no digit at all
    out.append(burst([word_a(1, 1, 0), word_b(), word_d([13, 1, 2, 3, 4, 5, 6, 7])]))    # none, and a bad code
    for thous in range(10, 16):                                    # thousands-digit codes 10 - 15
        out.append(burst([word_a(1, 0, 0, (rnd(10) << 14) | (thous << 10) | rnd(10)), word_b()]))
    for nawc, cn in ((0, 6), (1, 7), (0, 0), (1, 1)):              # S = 1 with NAWC 0 and 1: NAWC - 2 in unsigned char; word C says (NAWC - 2) mod 8, or NAWC
        out.append(burst([word_a(nawc, 1, 1), word_b(), word_c(cn)]))                    # the origination branch
        out.append(burst([word_a(nawc, 1, 1), word_b(order=0xD), word_c(cn)]))           # the registration branch: word C is not read
    for nawc, S, cn in ((2, 1, 0), (2, 1, 5), (1, 1, 7), (1, 0, 0), (3, 1, 1)):          # registrations with and without word C
        out.append(burst([word_a(nawc, 1, S), word_b(order=0xD, ordq=rnd(3), mtype=rnd(5)), word_c(cn)]))
    for n in (1, 2, 3, 4, 1, 2, 3):                                # originations with the serial number, dialling 0... and not
        first = 10 if n % 2 else int(rng.integers(1, 10))
        called = [word_d([first] + [int(rng.integers(1, 13)) for _ in range(7)])] + [filler() for _ in range(n - 1)]
        out.append(burst([word_a(n + 2, 1, 1), word_b(order=rnd(3) if n > 2 else 0), word_c(n)] + called))
    assert len(out) == 40
    return np.stack(out)


def make_bursts():
    import test_second_restatement as t2
    return np.concatenate([t2.reference_set()[0], t2._bursts(160, 2024), steered_bursts()]).astype(np.uint8)


def parse_decode(lines, n):
    d = {"class": np.full(n, -1, np.int8), "min": np.zeros(n, "S10"), "esn": np.full(n, -1, np.int64), "dialed": np.zeros(n, "S40"),
         "nawc_mismatch": np.zeros(n, bool), "bad_digit": np.zeros(n, bool), "dcc": np.zeros((n, 7), np.uint8),
         "dcc_bad": np.zeros(n, np.int64), "manch_bad": np.zeros((n, 7), np.int64), "a": np.zeros((n, 8), np.int64),
         "b": np.zeros((n, 12), np.int64)}
    msgs, owner, i, closed = [], [], -1, True
    for ln in lines:
        key, _, rest = ln.partition(" ")
        if key == "BURST":
            assert closed and int(rest) == i + 1
            i, closed = int(rest), False
        elif key == "CLASS":
            d["class"][i] = int(rest)
        elif key == "MIN":
            d["min"][i] = rest.encode()
        elif key == "ESN":
            d["esn"][i] = int(rest, 16)
        elif key == "DIALED":
            d["dialed"][i] = rest.encode()
        elif key == "FLAG":
            d[rest][i] = True
        elif key == "DCC":
            b, bad = rest.split()
            d["dcc"][i], d["dcc_bad"][i] = [int(c) for c in b], int(bad)
        elif key == "MANCH":
            d["manch_bad"][i] = [int(x) for x in rest.split()]
        elif key in ("A", "B"):
            d[key.lower()][i] = [int(kv.split("=")[1]) for kv in rest.split()]
        elif key == "MSG":
            msgs.append(ln)
            owner.append(i)
        else:
            assert ln == "END", ln
            closed = True
    assert i == n - 1 and closed
    d["lines"], d["line_owner"] = np.array(msgs), np.array(owner, np.int64)
    return d


# ------------------------------------------------------------------------------------------------ words and values for `fields`
def make_fields():
    rng = np.random.default_rng(7007)
    f = {}
    for k in "abcd":
        f["words_" + k] = rng.integers(0, 2, (512, 48)).astype(np.uint8)
    # every digit code in every position of a called-address word; the other seven positions hold digits (codes 1 - 12)
    sweep = []
    for pos in range(8):
        for code in range(16):
            codes = [int(x) for x in rng.integers(1, 13, 8)]
            codes[pos] = code
            d = 0
            for c in codes:
                d = (d << 4) | c
            sweep.append([0] + [int(x) for x in rng.integers(0, 2, 3)] + [(d >> (31 - i)) & 1 for i in range(32)] + [0] * 12)
    sweep.append([0, 0, 0, 0] + [(0x5551212A >> (31 - i)) & 1 for i in range(32)] + [0] * 12)     # survey_kats.json "called_digits"
    f["words_d"] = np.concatenate([f["words_d"], np.array(sweep, np.uint8)])
    mins = rng.integers(0, 10, (256, 10))
    for i in range(10):                                            # a zero in every position, alone and beside others
        mins[i, :] = rng.integers(1, 10, 10)
        mins[i, i] = 0
        mins[10 + i, i] = 0
    mins[20], mins[21] = 0, 9
    mins[22], mins[23] = [2, 1, 2, 5, 5, 5, 1, 2, 1, 2], [9, 0, 7, 5, 5, 5, 0, 0, 0, 0]       # the two of survey_kats.json
    f["min_strings"] = np.array(["".join(str(int(c)) for c in m) for m in mins], "S10")
    cm = np.stack([rng.integers(0, 1 << 24, 256), rng.integers(0, 1 << 10, 256)], axis=1).astype(np.uint64)
    for t in range(16):                                            # every thousands code, 10 - 15 among them
        cm[t, 0] = (int(cm[t, 0]) & ~(0xF << 10)) | (t << 10)
    f["calc_min_args"] = cm
    w1 = np.stack([rng.integers(0, 2, 256), rng.integers(0, 4, 256), rng.integers(0, 1 << 24, 256)], axis=1).astype(np.uint64)
    w1[0] = [1, 0, 0x6F2BE7]
    w2g = np.stack([rng.integers(0, 1 << 10, 256), rng.integers(0, 32, 256), rng.integers(0, 8, 256), rng.integers(0, 32, 256)], axis=1).astype(np.uint64)
    w2g[0] = [0x380, 0, 0, 7]
    w2v = np.stack([rng.integers(0, 4, 256), rng.integers(0, 1 << 10, 256), rng.integers(0, 8, 256), rng.integers(0, 2048, 256)], axis=1).astype(np.uint64)
    w2v[0] = [1, 0x380, 0, 356]
    fvc = np.stack([rng.integers(0, 4, 256), rng.integers(0, 32, 256), rng.integers(0, 8, 256), rng.integers(0, 32, 256)], axis=1).astype(np.uint64)
    f.update(focc_word1_args=w1, focc_word2_general_args=w2g, focc_word2_voice_channel_args=w2v, fvc_word1_general_args=fvc)
    # symbol buffers for the Manchester decoder: every pair value, the lengths bursts_message uses (7, 240) and odd ones
    lens = [4, 7, 240] + [int(x) for x in rng.integers(1, 300, 61)]
    bufs = [rng.integers(0, 2, 2 * n).astype(np.uint8) for n in lens]
    bufs[0] = np.array([1, 0, 0, 1, 1, 1, 0, 0], np.uint8)         # survey_kats.json
    f["manch_nbits"] = np.array(lens, np.int64)
    f["manch_syms"] = np.concatenate(bufs)
    return f


def fields_payload(f):
    u8 = lambda v: np.array([v], "u1").tobytes()                   # noqa: E731
    u64 = lambda v: np.array([v], "<u8").tobytes()                 # noqa: E731
    out = []
    for tag, k in ((TAG_A, "a"), (TAG_B, "b"), (TAG_C, "c"), (TAG_D, "d")):
        out += [u8(tag) + w.tobytes() for w in f["words_" + k]]
    out.append(u8(TAG_X3))
    out += [u8(TAG_PM) + bytes(m) for m in f["min_strings"]]
    out += [u8(TAG_CM) + u64(a) + u64(b) for a, b in f["calc_min_args"]]
    out += [u8(TAG_W1) + u8(m) + u8(d) + u64(v) for m, d, v in f["focc_word1_args"]]
    out += [u8(TAG_W2G) + u64(v) + u8(t) + u8(q) + u8(o) for v, t, q, o in f["focc_word2_general_args"]]
    out += [u8(TAG_W2V) + u8(s) + u64(v) + u8(m) + np.array([c], "<u2").tobytes() for s, v, m, c in f["focc_word2_voice_channel_args"]]
    out += [u8(TAG_FVC) + u8(p) + u8(t) + u8(q) + u8(o) for p, t, q, o in f["fvc_word1_general_args"]]
    off = 0
    for n in f["manch_nbits"]:
        out.append(u8(TAG_MD) + np.array([n], "<u4").tobytes() + f["manch_syms"][off:off + 2 * n].tobytes())
        off += 2 * int(n)
    out.append(u8(TAG_TRIG))
    return b"".join(out)


def parse_fields(lines, f):
    it = iter(lines)

    def kv(ln, key):
        assert ln.startswith(key + " "), ln
        return [x.split("=", 1)[1] for x in ln.split()[1:]]

    o = {}
    o["out_a"] = np.array([[int(x) for x in kv(next(it), "A")] for _ in f["words_a"]], np.int64)
    o["out_b"] = np.array([[int(x) for x in kv(next(it), "B")] for _ in f["words_b"]], np.int64)
    o["out_c"] = np.array([[int(x) for x in kv(next(it), "C")] for _ in f["words_c"]], np.int64)
    d = [kv(next(it), "D") for _ in f["words_d"]]
    o["out_d"] = np.array([[int(r[0]), int(r[1]), int(r[2]), int(r[4])] for r in d], np.int64)      # F, NAWC, DIGITS, bad
    o["out_d_digits"] = np.array([r[3] for r in d], "S8")
    x3 = [next(it).split() for _ in range(1024)]
    assert [int(r[1]) for r in x3] == list(range(1024)) and all(r[0] == "X3" for r in x3)
    o["out_extract_min_3"] = np.array([r[2] for r in x3], "S3")
    pm = [next(it).split() for _ in f["min_strings"]]
    assert all(r[0] == "PM" for r in pm)
    o["out_parse_min"] = np.array([[int(r[1]), int(r[2]), int(r[3])] for r in pm], np.int64)        # ok, MIN1, MIN2
    o["out_parse_min_back"] = np.array([r[4] for r in pm], "S10")
    cm = [next(it).split() for _ in f["calc_min_args"]]
    assert all(r[0] == "CM" for r in cm)
    o["out_calc_min"] = np.array([r[1] for r in cm], "S10")
    for k in ("focc_word1", "focc_word2_general", "focc_word2_voice_channel", "fvc_word1_general"):
        w = [next(it).split() for _ in f[k + "_args"]]
        assert all(r[0] == "W" and len(r[1]) == 28 for r in w)
        o["out_" + k] = np.array([r[1] for r in w], "S28")
    md = [next(it).split() for _ in f["manch_nbits"]]
    assert all(r[0] == "MD" for r in md)
    o["out_manch_bits"] = np.array([int(c) for r in md for c in r[1]], np.uint8)
    o["out_manch_bad"] = np.array([int(r[2]) for r in md], np.int64)
    t = next(it).split()
    assert t[0] == "TRIG" and next(it, None) is None
    o["out_trigger"] = np.array([int(c) for c in t[1]], np.uint8)
    return o


# ------------------------------------------------------------------------------------------------ words for `bch`
def bch_words():
    """a 63-bit word for every one of the 4096 remainders modulo the generator: the remainder itself (degree < 12) plus a code
    word, so that the words are not all zero in the message part; entry j = coefficient of x^(62-j) (tests/bchref.py)"""
    import bchref
    rng = np.random.default_rng(4096)
    out = np.zeros((4096, 63), np.uint8)
    for r in range(4096):
        m = int(rng.integers(0, 1 << 51)) << 12
        out[r] = bchref.bits(m ^ bchref.polymod(m) ^ r)
    return out


def parse_bch(lines):
    ok = np.array([int(l.split()[1]) for l in lines], np.uint8)
    msg = np.array([[int(c) for c in l.split()[2]] for l in lines], np.uint8)
    err = np.array([int(l.split()[3], 16) if l.split()[3] != "-" else 0 for l in lines], np.uint64)
    return ok, msg, err


# ------------------------------------------------------------------------------------------------ the file
def inputs():
    streams, names, cases = make_streams()
    return {"streams": streams, "stream_names": names, "cases": cases, "bursts": make_bursts(), "fields": make_fields(), "bch": bch_words()}


HOST_CASES = (("q2", [4096]), ("pin sym_spaced", [4096]))         # what the host blocks' test runs: their published bursts are decoded too


def run_all(inp, driver=DRIVER):
    """every input through `driver`; returns the raw outputs (the sanitizer build is run through here too).  The bursts the reference
    published on HOST_CASES are appended to the decode set, in that order: "decode_bursts" is what `decode` was given."""
    work = run_driver("work", work_payload(inp["streams"], [(si, sc) for _, si, sc in inp["cases"]]), driver, text=False)
    pubs = parse_work(work)
    keys = [(c[0], c[2]) for c in inp["cases"]]
    host = [pubs["payload"][pubs["case"] == keys.index((n, sc))] for n, sc in HOST_CASES]
    bursts = np.concatenate([inp["bursts"]] + host)
    return {"work": work, "decode_bursts": bursts, "host_counts": [len(h) for h in host],
            "decode": run_driver("decode", bursts.tobytes(), driver),
            "fields": run_driver("fields", fields_payload(inp["fields"]), driver),
            "bch": run_driver("bch", inp["bch"].tobytes(), driver)}


def check_coverage(inp, pubs, dec):
    count = lambda name, sched: int(sum(1 for p in pubs if inp["cases"][p["case"]][0] == name and inp["cases"][p["case"]][2] == sched))  # noqa: E731
    per_class = np.bincount(dec["class"], minlength=7)
    assert (per_class >= 8).all() and (dec["class"] >= 0).all(), dict(zip(CLASS_NAMES, per_class))
    # the stream outcomes SURVEY.md 8a recorded (Q1: strictly more than 3374; Q2: 3 / 3 / 3 / 2; Q4: lost at 63 000, kept at 60 000)
    assert [count("q2", [c]) for c in (1000, 4096, 333, 8191)] == [3, 3, 3, 2]
    assert count("pin sym_q1_short_tail", [4096]) == 0 and count("pin sym_q1_one_more", [4096]) == 1
    assert count("pin sym_q4_lost", [4096]) == 0 and count("pin sym_q4_kept", [4096]) == 1
    assert count("first fill 63000", [4096]) == 0 and count("first fill 60000", [4096]) == 1
    assert count("first fill 62087", [4096]) == 1 and count("first fill 62088", [4096]) == 0
    assert count("tail 3374", [333]) == 0 and count("tail 3375", [333]) == 1
    # streams on which the reference's rule and a rule that searches everything differ
    by_name = dict(zip(inp["stream_names"], inp["streams"]))
    differ = {n: (count(n, s), naive_count(by_name[n])) for n, s in (("q2", [8191]), ("q3 lost", [1000]), ("q3 ghost", [1000]), ("same call", [1000]))}
    assert all(a != b for a, b in differ.values()), differ
    assert differ["q3 ghost"][0] > differ["q3 ghost"][1] and differ["q3 lost"][0] < differ["q3 lost"][1]
    assert all(count("edge %d" % k, [512]) == 1 for k in range(TRIGGER_LEN))
    return dict(zip(CLASS_NAMES, per_class.tolist())), differ


def build_arrays(driver=DRIVER):
    inp = inputs()
    raw = run_all(inp, driver)
    pubs = parse_work(raw["work"])
    dec = parse_decode(raw["decode"], len(raw["decode_bursts"]))
    cover = check_coverage(inp, pubs, dec)
    out = {}
    out["stream_bits"] = np.packbits(np.concatenate(inp["streams"]))
    out["stream_len"] = np.array([s.size for s in inp["streams"]], np.int64)
    out["stream_name"] = np.array(inp["stream_names"])
    out["case_name"] = np.array([c[0] for c in inp["cases"]])
    out["case_stream"] = np.array([c[1] for c in inp["cases"]], np.int64)
    out["case_sched"] = np.array([x for c in inp["cases"] for x in c[2]], np.int64)
    out["case_sched_len"] = np.array([len(c[2]) for c in inp["cases"]], np.int64)
    out["pub_case"] = pubs["case"].astype(np.int64)
    out["pub_call"] = pubs["call"].astype(np.int64)
    out["pub_payload_bits"] = np.packbits(pubs["payload"], axis=1)
    out["burst_bits"] = np.packbits(raw["decode_bursts"], axis=1)
    keys = [(c[0], c[2]) for c in inp["cases"]]
    out["host_case"] = np.array([keys.index((n, sc)) for n, sc in HOST_CASES], np.int64)       # the bursts these cases published are the
    out["host_count"] = np.array(raw["host_counts"], np.int64)                                 # last sum(host_count) of the decode set
    assert out["host_count"].tolist() == [3, 6]
    for k, v in dec.items():
        out["dec_" + k] = v
    for k, v in inp["fields"].items():
        out["fld_" + k] = np.packbits(v, axis=-1) if k.startswith("words_") or k == "manch_syms" else v
    for k, v in parse_fields(raw["fields"], inp["fields"]).items():
        out["fld_" + k] = v
    out["bch_word_bits"] = np.packbits(inp["bch"], axis=1)
    out["bch_ok"], msg, out["bch_error"] = parse_bch(raw["bch"])
    out["bch_message_bits"] = np.packbits(msg, axis=1)
    return out, cover


def main():
    if not os.path.exists(DRIVER):
        sys.exit("oracle/_ref/refdriver is not built (python -c 'import oracle; oracle.build_reference()'; needs the reference's sources)")
    out, cover = build_arrays()
    if "--check" in sys.argv[1:]:
        old = np.load(PATH)
        assert sorted(old.files) == sorted(out), (sorted(set(old.files) ^ set(out)))
        for k, v in out.items():
            v = np.asarray(v)
            assert old[k].dtype == v.dtype and old[k].shape == v.shape and old[k].tobytes() == v.tobytes(), k
        print("reference_compiled.npz: %d arrays rebuilt, byte for byte equal" % len(out))
        return
    np.savez_compressed(PATH, **out)
    print("classes:", cover[0])
    print("bursts published (reference, search-everything):", cover[1])
    print("%s: %d bytes, %d streams, %d cases, %d publishes, %d bursts" % (os.path.basename(PATH), os.path.getsize(PATH), len(out["stream_len"]),
                                                                            len(out["case_name"]), len(out["pub_case"]), len(out["burst_bits"])))


if __name__ == "__main__":
    main()
