"""-m gpu: the two block rings of one handle (AMPS_RECC_FLAG_STREAM_POWER with AMPS_RECC_FLAG_STREAM_OFFSET_UNIT) through the code they
share (gr_amps_amd/csrc/recc_block_ring.hip.h): the same window for both, whole rows against streampowerref / streamoffsetunitref within
the bounds of test_gpu_stream_power (REL) and test_gpu_stream_offset_unit (ABS), and the queries by record bit for bit against the
stated reductions, back to back on the same records, each ring with scratch of its own."""
import numpy as np
import pytest

import gatherref
import streamoffsetref as sor
import streampowerref as spr
from gr_amps_amd import capi
from test_gpu_stream_offset_unit import _check as _check_unit
from test_gpu_stream_power import _bits, _check as _check_power, _noise

pytestmark = pytest.mark.gpu


def test_both_rings_of_one_handle_answer_from_the_same_window(gpu):
    C, sps, push, pushes = 3, 3, 1000, 50
    y = _noise(61, (C, push * pushes))
    with capi.Recc(n_channels=C, sps=sps, max_samples=4096, max_bursts=16, stream_power=True, stream_offset="unit") as r:
        slots = r.power_ring_snaps
        assert slots == r.autocorr_ring_blocks == 64                 # R = 16384: the smallest power of two >= 4096 + 3 * 3586 + 1024
        for a in range(0, y.shape[1], push):
            r.push_iq(np.ascontiguousarray(y[:, a:a + push]))
        P, first = r.channel_power()
        U, first_u = r.channel_autocorr()
        # one record per row inside the window (the last ends with the newest block and crosses slot 63 -> 0), then one that has left
        # the window and one that is not produced yet; only `channel` and `position` are read
        positions = [33536, 36000, 39999, 30000, 45000]
        recs = np.zeros(len(positions), capi.BURST_DTYPE)
        recs["position"] = positions
        recs["channel"] = [0, 1, 2, 1, 2]
        mean, cnt = r.burst_power(recs)
        total, cnt_u = r.burst_autocorr(recs)                        # back to back, on the same records
        mean2, cnt2 = r.burst_power(recs)                            # the offset ring's query has not touched the power ring's scratch
        bad = recs.copy()
        bad["channel"][1] = C
        for call in (r.burst_power, r.burst_autocorr):
            with pytest.raises(capi.AmpsError) as e:
                call(bad)
            assert e.value.code == -22

    produced = y.shape[1] // 64 * 64
    hi = produced // 256
    assert hi > 3 * slots and first == first_u == hi - slots and P.shape == U.shape == (C, slots)       # a little over three turns
    _check_power(P, spr.blocks(y[:, :produced])[:, first:hi])
    _check_unit(U, y[:, :produced], cols=slice(first, hi))

    assert np.array_equal(cnt, cnt_u) and np.array_equal(cnt, cnt2) and np.array_equal(_bits(mean), _bits(mean2))
    held = 0
    for g, m, t, c in zip(recs, mean, total, cnt):
        j0, count = spr.burst_window(int(g["position"]), sps)
        if j0 < first or j0 + count > hi:
            assert int(c) == 0 and gatherref.bits(m) == 0 and not _bits(t.real).any() and not _bits(t.imag).any()
            continue
        assert int(c) == count
        row = slice(j0 - first, j0 - first + count)
        assert gatherref.bits(m) == gatherref.bits(gatherref.gather_mean(P[int(g["channel"]), row]))
        re, im = sor.gather_sum(U[int(g["channel"]), row])
        assert np.float32(t.real).view(np.uint32) == re.view(np.uint32) and np.float32(t.imag).view(np.uint32) == im.view(np.uint32)
        held += 1
    assert held == C and list(cnt[C:]) == [0, 0] and 33536 // 256 == first and (39999 + 3374 * sps) // 256 == hi
    assert 39999 // 256 + 1 < 3 * slots <= hi - 1                                                       # that capture crosses slot 63 -> 0
