"""-m gpu: drain(copy=False) and drain_end(copy=False) hand out views of ONE buffer the handle owns (what bench.py's loop relies on:
no allocation and no copy per step), and the default drain() hands out an array of its own."""
import numpy as np
import pytest

import oracle
from gr_amps_amd import capi, synth

pytestmark = pytest.mark.gpu
N = 65536


def test_drain_without_copy_is_a_view_of_the_handles_buffer(gpu):
    iq = np.stack([synth.make_channel_block(N, 1, seed=100 + c)[0] for c in range(2)])
    want = oracle.fused_push_all(iq)
    assert len(want) == 2
    with capi.Recc(n_channels=2, sps=10, max_samples=N, max_bursts=8) as r:
        r.push_iq(iq)
        a = r.drain(copy=False)
        assert len(a) == 2 and a.base is not None and not a.flags.owndata
        assert a.tobytes() == want.tobytes()
        r.reset()
        r.push_iq(iq)
        r.drain_begin()
        b = r.drain_end(copy=False)
        assert len(b) == 2 and b.base is not None and np.shares_memory(a, b)
        assert b.tobytes() == want.tobytes()
        r.reset()
        r.push_iq(iq)
        c = r.drain()
        assert len(c) == 2 and c.flags.owndata and not np.shares_memory(a, c)
        assert c.tobytes() == want.tobytes()
