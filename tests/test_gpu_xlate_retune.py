"""-m gpu: amps_recc_retune_xlate (include/amps_recc.h) -- new centres for the configured translate form in mid-stream.

The contract is bit equality, so there is no tolerance here: from the first push after the call the stage's output (the debug taps)
is that of a twin handle configured with the new centres from the start and fed the same pushes; before it, that of a twin with the
old centres.  A sample's phasor comes from its absolute index and the carry holds unmixed input, which is why this can hold at all:
the pushes after the retune begin inside the filter's history of samples that arrived before it."""
import numpy as np
import pytest

from gr_amps_amd import capi, synth
from test_gpu_stream_power import _cuts, _ints

pytestmark = pytest.mark.gpu


def _noise(seed, shape, scale=0.5):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * scale).astype(np.complex64)


def _bits(a):
    return np.ascontiguousarray(a, np.complex64).view(np.uint32)


def _handle(C, sps, nmax, **kw):
    return capi.Recc(n_channels=C, sps=sps, max_samples=nmax, max_bursts=16, **kw)


# two pushes, retune, three ragged pushes (one shorter than any decimation, none a multiple of one)
PUSHES = [3001, 2222, 1999, 7, 2771]
FORMS = {
    # name: (rate, decimation or (interp, decim), sps, old centres, new centres, format)
    "shared_d2": (400e3, 2, 10, [-160e3, 44e3, 130e3], [-158.8e3, 45.2e3, 131.2e3], capi.SAMPLES_FC32),
    "wide_d12": (2.4e6, 12, 10, [-615e3, 1.11e6], [-616.5e3, 1.1085e6], capi.SAMPLES_SC16),
    "rational_5_64": (2.048e6, (5, 64), 8, [-800e3, 15e3, 615e3], [-801.2e3, 13.8e3, 613.8e3], capi.SAMPLES_CU8),
}


def _configure(r, rate, d, centres):
    if isinstance(d, tuple):
        r.set_xlate_resampled(rate, centres, d[0], d[1])
    else:
        r.set_xlate_shared(rate, centres, d)


def _tap(r, x, fmt):
    return r.debug_xlate_shared(x) if fmt == capi.SAMPLES_FC32 else r.debug_xlate_shared_as(x, fmt)


@pytest.mark.parametrize("name", sorted(FORMS))
def test_shared_forms_deliver_the_twins_output_from_the_next_push_on(gpu, name):
    rate, d, sps, old, new, fmt = FORMS[name]
    scale = 12 if name == "wide_d12" else 1                          # about the same number of outputs per push
    pushes = [p * scale + (1 if scale > 1 else 0) for p in PUSHES]
    n = sum(pushes)
    x = _noise(31, n) if fmt == capi.SAMPLES_FC32 else _ints(fmt, n, 32)
    C, nmax = len(old), 6000
    with _handle(C, sps, nmax) as r, _handle(C, sps, nmax) as t_old, _handle(C, sps, nmax) as t_new:
        _configure(r, rate, d, old)
        _configure(t_old, rate, d, old)
        _configure(t_new, rate, d, new)
        for i, (a, b) in enumerate(_cuts(pushes)):
            if i == 2:
                r.retune_xlate(new)
            got, want_new = _tap(r, x[a:b], fmt), _tap(t_new, x[a:b], fmt)
            assert got.shape == want_new.shape and got.shape[0] == C
            if i < 2:
                want_old = _tap(t_old, x[a:b], fmt)
                assert np.array_equal(_bits(got), _bits(want_old)), i
                assert not np.array_equal(_bits(got), _bits(want_new))           # the centres differ: so do the outputs
            else:
                assert np.array_equal(_bits(got), _bits(want_new)), i
        # a second retune, back: the twin with the old centres is matched again
        r.retune_xlate(old)
        tail = x[:1500 * scale]
        _tap(t_old, x[pushes[0] + pushes[1]:], fmt)                  # bring the old twin to the same position
        assert np.array_equal(_bits(_tap(r, tail, fmt)), _bits(_tap(t_old, tail, fmt)))


def test_per_row_form(gpu):
    C, n = 2, sum(PUSHES)
    x = _noise(33, (C, n))
    with _handle(C, 10, 4000) as r, _handle(C, 10, 4000) as t_old, _handle(C, 10, 4000) as t_new:
        r.set_xlate(rate_hz=400e3, center_hz=160e3, decim=2)
        t_old.set_xlate(rate_hz=400e3, center_hz=160e3, decim=2)
        t_new.set_xlate(rate_hz=400e3, center_hz=158.7e3, decim=2)
        for i, (a, b) in enumerate(_cuts(PUSHES)):
            if i == 2:
                with pytest.raises(capi.AmpsError) as e:             # the per-row form has ONE centre
                    r.retune_xlate([158.7e3, 158.7e3])
                assert e.value.code == -22
                r.retune_xlate([158.7e3])
            blk = np.ascontiguousarray(x[:, a:b])
            got = r.debug_xlate(blk)
            want = (t_old if i < 2 else t_new).debug_xlate(blk)
            (t_new if i < 2 else t_old).debug_xlate(blk)
            assert got.shape[0] == C and np.array_equal(_bits(got), _bits(want)), i


def test_refused_calls_leave_the_handle_as_it_was(gpu):
    rate, d, sps, old, new, fmt = FORMS["shared_d2"]
    x = _noise(34, 6000)
    with _handle(3, sps, 4000) as r, _handle(3, sps, 4000) as twin, _handle(3, sps, 4000) as bare:
        with pytest.raises(capi.AmpsError) as e:                     # no translate form configured
            bare.retune_xlate(new)
        assert e.value.code == -38
        _configure(r, rate, d, old)
        _configure(twin, rate, d, old)
        assert np.array_equal(_bits(_tap(r, x[:2501], fmt)), _bits(_tap(twin, x[:2501], fmt)))
        for bad in (new[:2], new + [0.0], [new[0], float("nan"), new[2]], [new[0], new[1], 401e3], [new[0], -float("inf"), new[2]]):
            with pytest.raises(capi.AmpsError) as e:
                r.retune_xlate(bad)
            assert e.value.code == -22, bad
        assert capi.load().amps_recc_retune_xlate(r._h, None, 3) == -22
        assert np.array_equal(_bits(_tap(r, x[2501:], fmt)), _bits(_tap(twin, x[2501:], fmt)))


def _burst_stream(fs, decim, fc, first, seed):
    n = first + (3374 + 300) * 10 * decim + 4000 * decim
    iq, truth = synth.make_channel_block(n, 1, seed=seed, sps=10 * decim, snr_db=30.0 - 10.0 * np.log10(decim), first=first, jitter=False)
    assert len(truth) == 1 and truth[0][0] == first
    return (iq * np.exp(2j * np.pi * fc * np.arange(n) / fs)).astype(np.complex64), truth


def test_a_burst_well_behind_the_retune_gives_the_twins_record(gpu):
    """retune point: channel-rate sample 5000; the burst's dotting begins beyond sample 8000 > 5000 + 2048"""
    fs, decim = 400e3, 2
    old, new = [-160e3, 44e3, 130e3], [-158.8e3, 45.2e3, 131.2e3]
    cut, first = 10000, 16000
    x, truth = _burst_stream(fs, decim, new[1], first, 9300)
    assert (first - cut) // decim > 2048
    recs = []
    for centres in (old, new):
        with _handle(3, 10, x.size // decim) as r:
            r.set_xlate_shared(fs, centres, decim)
            r.push_raw_shared(x[:cut])
            r.retune_xlate(new)                                      # on the twin: the same centres again, which changes nothing
            r.push_raw_shared(x[cut:cut + 33333])
            r.push_raw_shared(x[cut + 33333:])
            recs.append(r.drain())
    assert [(int(g["channel"]), g["min"].decode()) for g in recs[1]] == [(1, truth[0][2])]
    assert len(recs[0]) == 1 and recs[0].tobytes() == recs[1].tobytes()


def test_a_retune_between_drain_begin_and_drain_end(gpu):
    """the streaming use: a burst is decoded, the drain is begun, the retune and the next push are enqueued behind it, the drain ends.
    The records are those of a handle that was never retuned, and the stage then delivers the new twin's output"""
    fs, decim = 400e3, 2
    old, new = [-160e3, 44e3, 130e3], [-158.8e3, 45.2e3, 131.2e3]
    x, truth = _burst_stream(fs, decim, old[1], 4000, 9301)
    more = _noise(35, 5000)
    nmax = x.size // decim
    with _handle(3, 10, nmax) as r, _handle(3, 10, nmax) as plain, _handle(3, 10, nmax) as t_new:
        for h, c in ((r, old), (plain, old), (t_new, new)):
            h.set_xlate_shared(fs, c, decim)
        r.push_raw_shared(x)
        plain.push_raw_shared(x)
        t_new.debug_xlate_shared(x)
        want = plain.drain()
        r.drain_begin()
        r.retune_xlate(new)
        r.push_raw_shared(more[:2501])
        got = r.drain_end()
        t_new.debug_xlate_shared(more[:2501])
        assert [g["min"].decode() for g in want] == [truth[0][2]] and got.tobytes() == want.tobytes()
        assert np.array_equal(_bits(r.debug_xlate_shared(more[2501:])), _bits(t_new.debug_xlate_shared(more[2501:])))
