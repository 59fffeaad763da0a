"""Loader of tests/golden/reference_compiled.npz (made by tests/golden/make_reference_compiled.py: inputs from seeds and what the
reference's own compiled code makes of them) for tests/test_cpu_reference_compiled.py and tests/test_gpu_reference_compiled.py.
Reads the committed file only; unpacks the bits once and hands out the same arrays to every test (do not write to them)."""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_compiled.npz")
CAPTURE = 3374
A_FIELDS = ("F", "NAWC", "T", "S", "E", "ER", "SCM", "MIN1")
B_FIELDS = ("F", "NAWC", "MSG_TYPE", "ORDQ", "ORDER", "LT", "EP", "SCM4", "MPCI", "SDCC1", "SDCC2", "MIN2")
INVALID_WORD_A, E_ZERO, PAGE_RESPONSE, REGISTRATION, ORIGINATION, BAD_NAWC, UNKNOWN = range(7)

_cache = {}


class Fixture:
    def __init__(self):
        z = np.load(PATH)
        self.z = {k: z[k] for k in z.files}
        z = self.z
        bits = np.unpackbits(z["stream_bits"])
        ends = np.cumsum(z["stream_len"])
        self.streams = [bits[e - n:e] for e, n in zip(ends, z["stream_len"])]
        self.stream_names = [str(s) for s in z["stream_name"]]
        sched_end = np.cumsum(z["case_sched_len"])
        # (name, stream index, schedule)
        self.cases = [(str(z["case_name"][i]), int(z["case_stream"][i]), [int(x) for x in z["case_sched"][e - n:e]])
                      for i, (e, n) in enumerate(zip(sched_end, z["case_sched_len"]))]
        payloads = np.unpackbits(z["pub_payload_bits"], axis=1)[:, :CAPTURE]
        # per case: [(call index, payload bytes)] as the reference published them
        self.pubs = [[] for _ in self.cases]
        for c, call, p in zip(z["pub_case"], z["pub_call"], payloads):
            self.pubs[int(c)].append((int(call), p.tobytes()))
        self.bursts = np.unpackbits(z["burst_bits"], axis=1)[:, :CAPTURE]
        self.lines = [[] for _ in self.bursts]
        for o, l in zip(z["dec_line_owner"], z["dec_lines"]):
            self.lines[int(o)].append(str(l))

    def host_cases(self):
        """[(case index, [message lines the reference's recc_decode published for the bursts its recc published on that case])]"""
        out, at = [], len(self.bursts) - int(self.z["host_count"].sum())
        for c, n in zip(self.z["host_case"], self.z["host_count"]):
            assert [p for _, p in self.pubs[int(c)]] == [self.bursts[at + k].tobytes() for k in range(int(n))]
            out.append((int(c), [l for k in range(int(n)) for l in self.lines[at + k]]))
            at += int(n)
        return out

    def case(self, name, sched):
        i = [k for k, c in enumerate(self.cases) if c[0] == name and c[2] == list(sched)]
        assert len(i) == 1, (name, sched)
        return i[0]

    def words(self, k):
        return np.unpackbits(self.z["fld_words_" + k], axis=1)[:, :48]

    def manchester_buffers(self):
        syms = np.unpackbits(self.z["fld_manch_syms"])
        out, off, boff = [], 0, 0
        for n, bad in zip(self.z["fld_manch_nbits"], self.z["fld_out_manch_bad"]):
            n = int(n)
            out.append((syms[off:off + 2 * n], self.z["fld_out_manch_bits"][boff:boff + n], int(bad)))
            off, boff = off + 2 * n, boff + n
        return out

    def expected_record(self, i):
        """what the reference revealed about burst i, as {record field: value}: only what it revealed.  has_esn and n_called_words
        are not printed by the reference; they follow from fields it parsed (S of word A is what the registration and origination
        branches hand on as has_esn; the origination loop reads NAWC - 2 S called-address words)."""
        z = self.z
        cls = int(z["dec_class"][i])
        a = dict(zip(A_FIELDS, (int(v) for v in z["dec_a"][i])))
        b = dict(zip(B_FIELDS, (int(v) for v in z["dec_b"][i])))
        want = {"msg_class": cls, "dcc": z["dec_dcc"][i].tolist(), "dcc_bad": int(z["dec_dcc_bad"][i]), "manch_bad": z["dec_manch_bad"][i].tolist(),
                "nawc_mismatch": bool(z["dec_nawc_mismatch"][i]), "bad_digit": bool(z["dec_bad_digit"][i])}
        want.update({"a_" + k: v for k, v in a.items()})
        want.update({"b_" + k: v for k, v in b.items()})
        if cls in (PAGE_RESPONSE, REGISTRATION, ORIGINATION):
            want["min"] = z["dec_min"][i].decode()
        if int(z["dec_esn"][i]) >= 0:
            want["esn"] = int(z["dec_esn"][i])
        elif cls == REGISTRATION:
            want["esn"] = 0                                        # handle_registration is handed esn = 0 when word C is not read
        want["has_esn"] = a["S"] if cls in (REGISTRATION, ORIGINATION, BAD_NAWC) else 0
        want["dialed"] = z["dec_dialed"][i].decode() if cls == ORIGINATION else ""
        want["n_called_words"] = a["NAWC"] - 2 * a["S"] if cls == ORIGINATION else 0
        return want


def fixture():
    if "f" not in _cache:
        _cache["f"] = Fixture()
    return _cache["f"]


def check_record(rec, want, what):
    """a record of the oracle or of the device (BURST_DTYPE) against expected_record()"""
    flags = int(rec["flags"])
    got = {"msg_class": int(rec["msg_class"]), "dcc": rec["dcc"].tolist(), "dcc_bad": int(rec["dcc_bad"]), "manch_bad": rec["manch_bad"].tolist(),
           "nawc_mismatch": bool(flags & 2), "bad_digit": bool(flags & 4), "min": rec["min"].decode(), "esn": int(rec["esn"]),
           "has_esn": int(rec["has_esn"]), "dialed": rec["dialed"].decode(), "n_called_words": int(rec["n_called_words"])}
    got.update({"a_" + k: int(rec["a_" + k]) for k in A_FIELDS})
    got.update({"b_" + k: int(rec["b_" + k]) for k in B_FIELDS})
    for k, v in want.items():
        assert got[k] == v, (what, k, got[k], v)


def reply_lines(r):
    """the message lines of a reply structure (oracle.Reply / capi.Reply), in the form tests/test_cpu_reference_pins.py defines"""
    bits = lambda a: "".join(str(int(b)) for b in a)                # noqa: E731
    lines = []
    if r.has_focc:
        lines.append("MSG focc_words stream=%d n=%d w1=%s w2=%s" % (r.focc_stream, r.focc_nwords, bits(r.focc_word1), bits(r.focc_word2)))
    if r.has_fvc:
        lines.append("MSG fvc_words n=%d w1=%s repeat=%d" % (r.fvc_count, bits(r.fvc_word1), r.fvc_repeat))
    if r.has_mutes:
        lines.append("MSG fvc_mute %d" % r.fvc_mute)
        lines.append("MSG audio_mute %d" % r.audio_mute)
    if r.has_command:
        lines.append("MSG command_out " + r.command.decode())
    return lines
