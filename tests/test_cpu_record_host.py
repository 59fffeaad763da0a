"""The host's half of a drain without a GPU: gr_amps_amd/csrc/recc_record_host.h (expand_packed_record, expand_packed_burst, record_key,
gather_sorted) is on the path of every record the library returns.  tests/record_host_main.cc sees that header and include/amps_recc.h
only, is built with AddressSanitizer and UndefinedBehaviorSanitizer (nothing in LD_PRELOAD: the runtimes are linked in) and runs as
a child process on a file of packed records.  The input is packed here, in numpy, from the layout written above PACKED_RECORD_BYTES:

    dwords  0 .. 12   the record's first 52 bytes as they are
    dwords 13 .. 23   word_raw (336 bytes of 0 / 1): bit 4 j + i of dword 13 + g is byte 32 g + 4 j + i of the array
    dwords 24 .. 31   word_dec (252 bytes) likewise
    dwords 32 .. 53   the record's last 88 bytes as they are

The bits past either array, and past the 3374 symbols of a kept burst, are don't-care: they are set to ONES here, so that a gather
that leaks them is caught."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "record_host_main.cc")
REC, PACKED, KEPT, KEPT_PACKED = 728, 216, 3374, 424
RAW_OFF, DEC_OFF, TAIL_OFF = 52, 388, 640
N = 64
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover"]


def _pack_bits(arr, ndwords):
    """[n][len] bytes of 0 / 1 -> [n][ndwords] dwords, bit 4 j + i of dword g = byte 32 g + 4 j + i; ones past the array's end"""
    n, length = arr.shape
    padded = np.ones((n, 32 * ndwords), np.uint32)
    padded[:, :length] = arr
    out = np.zeros((n, ndwords), np.uint32)
    for g in range(ndwords):
        for j in range(8):
            for i in range(4):
                out[:, g] |= padded[:, 32 * g + 4 * j + i] << np.uint32(4 * j + i)
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert shutil.which("g++"), "this test needs g++"
    out = str(tmp_path_factory.mktemp("record_host") / "record_host_main")
    base = ["g++", "-std=c++17", "-g", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "gr_amps_amd", "csrc"), SRC, "-o", out]
    # the runtimes linked into the program, as the sanitizer itself advises where something else is preloaded
    p = subprocess.run(base + SANITIZE + ["-static-libasan", "-static-libubsan"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        p = subprocess.run(base + SANITIZE, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0 and "cannot find" in p.stdout and ("asan" in p.stdout or "ubsan" in p.stdout):
        print("no sanitizer runtimes for g++ here: the comparison runs without them\n" + p.stdout)
        p = subprocess.run(base, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    return out


@pytest.fixture(scope="module")
def lists():
    """64 records and their kept bursts, and the packed form of both"""
    rng = np.random.default_rng(20261018)
    recs = rng.integers(0, 256, (N, REC), dtype=np.uint8)
    recs[:, RAW_OFF:TAIL_OFF] = rng.integers(0, 2, (N, TAIL_OFF - RAW_OFF), dtype=np.uint8)        # word_raw, word_dec: a byte per bit
    channel = rng.choice(np.array([0, 1, (1 << 20) - 1], np.uint32), N)
    channel[:6] = [0, 0, 1, 1, (1 << 20) - 1, (1 << 20) - 1]                                          # either end on every channel
    position = rng.choice(np.arange(1, 1 << 20, dtype=np.uint64), N, replace=False) * np.uint64((1 << 24) - 3)   # distinct, below 2^44
    position[:6] = [0, (1 << 44) - 1] * 3
    assert position.max() < (1 << 44) and len(set(zip(channel.tolist(), position.tolist()))) == N
    recs[:, 0:4] = channel.astype("<u4").view(np.uint8).reshape(N, 4)
    recs[:, 8:16] = position.astype("<u8").view(np.uint8).reshape(N, 8)
    packed = np.zeros((N, PACKED // 4), np.uint32)
    packed[:, 0:13] = recs[:, :RAW_OFF].copy().view("<u4")
    packed[:, 13:24] = _pack_bits(recs[:, RAW_OFF:DEC_OFF], 11)
    packed[:, 24:32] = _pack_bits(recs[:, DEC_OFF:TAIL_OFF], 8)
    packed[:, 32:54] = recs[:, TAIL_OFF:].copy().view("<u4")
    kept = rng.integers(0, 2, (N, KEPT), dtype=np.uint8)
    kept_packed = _pack_bits(kept, KEPT_PACKED // 4)
    order = sorted(range(N), key=lambda i: (int(channel[i]), int(position[i])))
    assert any(channel[a] == channel[b] for a, b in zip(order, order[1:]))                          # ties on the channel
    return recs, kept, packed.astype("<u4").tobytes(), kept_packed.astype("<u4").tobytes(), order


@pytest.mark.parametrize("cap", [0, 1, 63, 64])
def test_sorted_gather_of_packed_records(exe, lists, tmp_path, cap):
    recs, kept, packed, kept_packed, order = lists
    assert len(packed) == N * PACKED and len(kept_packed) == N * KEPT_PACKED
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([N, cap], "<u8").tobytes() + packed + kept_packed)
    p = subprocess.run([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, (p.returncode, p.stderr[-4000:])
    raw = open(fout, "rb").read()
    k, overflow = (int(v) for v in np.frombuffer(raw[:16], "<u8"))
    assert k == min(cap, N) and overflow == (1 if N > cap else 0)
    assert len(raw) == 16 + k * (REC + KEPT)
    got = np.frombuffer(raw[16:16 + k * REC], np.uint8).reshape(k, REC)
    got_kept = np.frombuffer(raw[16 + k * REC:], np.uint8).reshape(k, KEPT)
    keys = [(int(got[i, 0:4].copy().view("<u4")[0]), int(got[i, 8:16].copy().view("<u8")[0])) for i in range(k)]
    assert keys == sorted(keys)                                               # ordered by (channel, position)
    for i in range(k):                                                        # exactly the first `cap` of that order, byte for byte
        assert got[i].tobytes() == recs[order[i]].tobytes(), (cap, i)
        assert got_kept[i].tobytes() == kept[order[i]].tobytes(), (cap, i)    # the last six symbols included
