"""-m gpu: the symbol seam (recc_symbols_kernel), the decode kernel, amps_recc_reply_words and the host blocks against what the
REFERENCE'S OWN COMPILED CODE produced -- tests/golden/reference_compiled.npz (tests/golden/make_reference_compiled.py; the CPU side of
the same comparison is tests/test_cpu_reference_compiled.py).  Reads the committed file only.  Every comparison is exact."""
import subprocess

import numpy as np
import pytest

import refcompiled
from gr_amps_amd import capi
from gr_amps_amd.host import build_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return refcompiled.fixture()


def _sizes(sched, n):
    out, off, k = [], 0, 0
    while off < n:
        out.append(min(sched[k % len(sched)], n - off))
        off += out[-1]
        k += 1
    return out


def test_push_symbols_publishes_what_the_reference_published(gpu, fx):
    """every stream and schedule of the fixture through amps_recc_push_symbols on one one-channel handle (reset between cases):
    (call index, payload) of every burst as the reference's recc_impl::work published them"""
    calls = 0
    with capi.Recc(n_channels=1, sps=10, max_samples=0, max_bursts=4) as r:
        for i, (name, si, sched) in enumerate(fx.cases):
            r.reset()
            s, got, off = fx.streams[si], [], 0
            for call, n in enumerate(_sizes(sched, s.size)):
                bursts, chans = r.push_symbols(s[None, off:off + n])
                got += [(call, bytes(b)) for b in bursts]
                assert not len(chans) or set(chans.tolist()) == {0}
                off += n
                calls += 1
            assert got == fx.pubs[i], (name, sched)
    print("\n%d cases, %d work() calls, %d bursts" % (len(fx.cases), calls, sum(len(p) for p in fx.pubs)))


def test_push_symbols_on_three_channels_publishes_what_the_reference_published(gpu, fx):
    """three different streams at once through a three-channel handle: the last first-fill trigger the reference keeps (62 087), the
    first one it loses (62 088) and one that ends with the buffer (65 462, lost)"""
    ids = [fx.case("first fill %d" % p, [4096]) for p in (62087, 62088, 65462)]
    syms = np.stack([fx.streams[fx.cases[i][1]] for i in ids])
    got = [[] for _ in ids]
    with capi.Recc(n_channels=3, sps=10, max_samples=0, max_bursts=8) as r:
        for call, off in enumerate(range(0, syms.shape[1], 4096)):
            bursts, chans = r.push_symbols(np.ascontiguousarray(syms[:, off:off + 4096]))
            for b, ch in zip(bursts, chans):
                got[int(ch)].append((call, bytes(b)))
    assert got == [fx.pubs[i] for i in ids]
    assert [len(fx.pubs[i]) for i in ids] == [1, 0, 0]


def test_decode_kernel_and_reply_words_equal_the_reference(gpu, fx):
    """every burst of the fixture through amps_recc_decode_bursts, in one batch and with a channel array: class, MIN, ESN, dialled digits,
    flags and every parsed field as the reference's bursts_message revealed them; amps_recc_reply_words of each record = the messages the
    reference's recc_decode published"""
    channels = (np.arange(len(fx.bursts), dtype=np.uint32) * 11) % 7
    with capi.Recc(n_channels=1, max_bursts=8) as r:
        plain = r.decode_bursts(fx.bursts)
        tagged = r.decode_bursts(fx.bursts, channels)
    for i in range(len(fx.bursts)):
        want = fx.expected_record(i)
        refcompiled.check_record(plain[i], want, i)
        refcompiled.check_record(tagged[i], want, (i, "channels"))
        assert int(plain[i]["channel"]) == 0 and int(tagged[i]["channel"]) == int(channels[i])
        assert refcompiled.reply_lines(capi.reply_words(plain[i])) == fx.lines[i], i
        assert refcompiled.reply_lines(capi.reply_words(tagged[i])) == fx.lines[i], i
    assert {int(c) for c in plain["msg_class"]} == set(range(7))


def test_host_blocks_print_the_lines_the_reference_published(gpu, fx, tmp_path):
    """gr::amps::recc into gr::amps::recc_decode (gr_amps_amd/recctest) on two of the fixture's streams: every message, in order"""
    _, exe = build_host()
    for case, want in fx.host_cases():
        name, si, sched = fx.cases[case]
        p = tmp_path / ("case%d.syms" % case)
        fx.streams[si].tofile(p)
        out = subprocess.run([exe, "syms", str(p), str(sched[0])], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert [l for l in out.stdout.splitlines() if l.startswith("MSG ")] == want and len(want) >= 3, name
