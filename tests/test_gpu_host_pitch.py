"""Host blocks whose row pitch exceeds their sample count: push_iq / push_raw with nsamp < ld.  Every other host push of the suite is
contiguous, so the 2-D form of the staging copy (recc_devmem.hip.h: HostStage) otherwise only ever runs with pitch = width.

Each test pushes one stream three ways -- contiguous host blocks, pitched host blocks, the same pitched arrays as device tensors --
as two blocks of unequal length back to back with no drain in between, and asks for byte-equal records and every burst found."""
import numpy as np
import pytest

from gr_amps_amd import capi, synth

pytestmark = pytest.mark.gpu

PAD = 37            # columns behind the samples of a pitched block


def _pitched(block, rng):
    """[C][n] -> contiguous [C][n + PAD]; the pad carries strong noise, which would show in the records if it were read"""
    pad = (rng.standard_normal((block.shape[0], PAD)) + 1j * rng.standard_normal((block.shape[0], PAD))) * 4.0
    return np.ascontiguousarray(np.concatenate([block, pad.astype(np.complex64)], axis=1))


def _three_ways(make_handle, push, iq, split):
    """records of (contiguous host, pitched host, pitched device) pushes of iq[:, :split] then iq[:, split:]"""
    import torch
    rng = np.random.default_rng(5)
    blocks = [np.ascontiguousarray(iq[:, :split]), np.ascontiguousarray(iq[:, split:])]
    pitched = [_pitched(b, rng) for b in blocks]
    on_device = [torch.from_numpy(p).to("cuda:0") for p in pitched]     # the caller's until the drain
    torch.cuda.synchronize()
    out = []
    for form in (blocks, pitched, on_device):
        with make_handle() as r:
            for b, blk in zip(blocks, form):
                push(r, blk, b.shape[1])
            out.append(r.drain())
    return out


def _check(out, truth):
    plain, host, dev = out
    assert len(plain) == len(truth)
    for c, t in enumerate(truth):
        assert plain[c]["channel"] == c and plain[c]["min"].decode() == t[2] and plain[c]["valid"].all()
    assert host.tobytes() == plain.tobytes()
    assert dev.tobytes() == plain.tobytes()


def test_iq_seam_pitched_host_blocks(gpu):
    C, N, split = 3, 45000, 17003
    chans = [synth.make_channel_block(N, 1, seed=910 + c, sps=10) for c in range(C)]
    iq = np.stack([c[0] for c in chans]).astype(np.complex64)
    out = _three_ways(lambda: capi.Recc(n_channels=C, sps=10, max_samples=N, max_bursts=16),
                      lambda r, blk, n: r.push_iq(blk, nsamp=n), iq, split)
    _check(out, [c[1][0] for c in chans])


def test_translate_seam_pitched_host_blocks(gpu):
    N, split, fc = 90000, 51001, 160e3
    iq400, truth = synth.make_channel_block(N, 1, seed=920, sps=20)
    iq = (iq400 * np.exp(2j * np.pi * fc * np.arange(N) / 400e3)).astype(np.complex64)[None, :]

    def handle():
        r = capi.Recc(n_channels=1, sps=10, max_samples=N // 2, max_bursts=16)
        r.set_xlate(rate_hz=400e3, center_hz=fc, decim=2)
        return r
    out = _three_ways(handle, lambda r, blk, n: r.push_raw(blk, nsamp=n), iq, split)
    _check(out, [truth[0]])
