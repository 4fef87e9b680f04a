"""The lagged, folded delta + shuffle kernels alone on the MI355X (-m gpu): glcLagDeltaShuffleDevice, glcUnlagDeltaUnshuffleDevice and
glcUnlagDeltaUnshuffleRangeDevice against the numpy definition of tests/lag_model.py, byte for byte, over element sizes 2, 4, 8 x lags
1, 2, 3, 5, 8, 16 x fold 0, 1 -- lengths around an element, the lag, a run (2048 elements: a chain must not cross it) and a 16 KiB
tile, several tiles, 70 tiles; input and output misaligned by 0, 1, 3 and 15 bytes; 64 guard bytes on each side of the output;
values that force carries; (1, 0) against glcDeltaShuffleDevice; ranges; refusals that leave the output untouched."""
import numpy as np
import pytest

import container_model as M
import lag_model as G

pytestmark = pytest.mark.gpu

ILLEGAL = 2
RUN, TILE = 2048, 16384
ELEMS, LAGS, FOLDS = (2, 4, 8), (1, 2, 3, 5, 8, 16), (0, 1)
OFFSETS = (0, 1, 3, 15)
GUARD = 64


def _lengths(e, lag):
    return [0, 1, e - 1, e, lag * e - 1, lag * e + e, RUN * e - e, RUN * e, RUN * e + e, TILE, TILE + lag * e + 3, 3 * TILE + 5]


def _aligned(torch, n, cuda, fill=None):
    """a device byte buffer of n bytes whose first byte is 256-byte aligned"""
    buf = torch.empty(n + 256, dtype=torch.uint8, device=cuda) if fill is None else torch.full((n + 256,), fill, dtype=torch.uint8, device=cuda)
    a = (-buf.data_ptr()) % 256
    return buf[a:a + n]


def _random(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _check_both(glc, torch, cuda, e, lag, fold, x, offsets):
    """forward and inverse of x at every (input offset, output offset) of `offsets`, against the model, guards included"""
    n = x.size
    want = G.lag_delta_shuffle(x, e, lag, fold)
    assert np.array_equal(G.unlag_delta_unshuffle(want, e, lag, fold), x)
    d_x, d_want = torch.from_numpy(x.copy()).to(cuda), torch.from_numpy(want.copy()).to(cuda)
    src = _aligned(torch, n + 16, cuda)
    for fn, a, b in ((glc.lag_delta_shuffle, d_x, d_want), (glc.unlag_delta_unshuffle, d_want, d_x)):
        for so in offsets:
            src[so:so + n] = a
            for do in offsets:
                dst = _aligned(torch, n + 2 * GUARD + 16, cuda, fill=0xA5)
                out = dst[GUARD + do:GUARD + do + n]
                fn(src[so:so + n], e, lag, fold, out=out)
                assert torch.equal(out, b), (fn.__name__, e, lag, fold, n, so, do)
                assert bool((dst[:GUARD + do] == 0xA5).all()) and bool((dst[GUARD + do + n:] == 0xA5).all()), (fn.__name__, e, lag, fold, n, so, do)


@pytest.mark.parametrize("fold", FOLDS)
@pytest.mark.parametrize("lag", LAGS)
@pytest.mark.parametrize("e", ELEMS)
def test_lengths_against_the_model(glc, cuda, e, lag, fold):
    import torch
    for i, n in enumerate(_lengths(e, lag)):
        _check_both(glc, torch, cuda, e, lag, fold, _random(n, 1000 * e + 10 * lag + i), (0, 3) if n else (0,))


@pytest.mark.parametrize("e", ELEMS)
def test_every_pairing_of_misalignments(glc, cuda, e):
    import torch
    for lag, fold in ((3, 1), (16, 0), (1, 1)):
        _check_both(glc, torch, cuda, e, lag, fold, _random(TILE + lag * e + 3, 50 + e + lag), OFFSETS)


@pytest.mark.parametrize("fold", FOLDS)
@pytest.mark.parametrize("e", ELEMS)
def test_values_that_force_carries(glc, cuda, e, fold):
    import torch
    dt, top = "<u%d" % e, (1 << (8 * e)) - 1
    q = TILE // e + RUN + 37
    ones = np.full(q, top, dtype=dt)
    alternating = np.tile(np.array([0, 1 << (8 * e - 1)], dtype=dt), q // 2 + 1)[:q]
    for lag in (1, 2, 3, 16):
        for x in (ones, alternating):
            _check_both(glc, torch, cuda, e, lag, fold, np.concatenate([x.view(np.uint8), np.arange(e - 1, dtype=np.uint8)]), (0, 3))


@pytest.mark.parametrize("fold", FOLDS)
def test_carries_cross_the_dword_boundary_of_8_byte_elements(glc, cuda, fold):
    """three interleaved channels around multiples of 2^32: the subtraction borrows from the high dword and the sums carry into it"""
    import torch
    rng = np.random.default_rng(8)
    q = TILE // 8 + 555
    k = rng.integers(1, 1 << 20, q, dtype=np.int64) << 32
    x = (k + rng.integers(-5, 6, q)).astype("<u8")
    d = x[3:] - x[:-3]
    assert ((d >> np.uint64(32)) != ((d + np.uint64(16)) >> np.uint64(32))).any() and (x.astype(np.uint32) > 0xFFFFFFF0).any()
    _check_both(glc, torch, cuda, 8, 3, fold, x.view(np.uint8), (0, 1))


def test_seventy_tiles(glc, cuda):
    import torch
    for e, lag, fold in ((2, 3, 1), (4, 2, 0), (8, 5, 1)):
        _check_both(glc, torch, cuda, e, lag, fold, _random(70 * TILE + 7, e + lag), (1,))


@pytest.mark.parametrize("e", ELEMS)
def test_lag_1_fold_0_is_the_delta_shuffle(glc, cuda, e):
    import torch
    x = _random(2 * TILE + 5 * e + 1, e)
    d = torch.from_numpy(x).to(cuda)
    y = glc.delta_shuffle(d, e)
    assert torch.equal(glc.lag_delta_shuffle(d, e, 1, 0), y) and np.array_equal(y.cpu().numpy(), M.delta_shuffle(x, e))
    assert torch.equal(glc.unlag_delta_unshuffle(y, e, 1, 0), d)
    assert np.array_equal(G.lag_delta_shuffle(x, e, 1, 0), M.delta_shuffle(x, e))


@pytest.mark.parametrize("lag,fold", [(1, 1), (2, 0), (3, 1), (5, 0), (16, 1)])
@pytest.mark.parametrize("e", ELEMS)
def test_range_inverse(glc, cuda, e, lag, fold):
    import torch
    n = 3 * TILE + 2 * RUN * e + 37 * e + (e - 1)                   # a ragged end, behind first = 3 * 2048 for every e
    x = _random(n, 7 * e + lag)
    y = G.lag_delta_shuffle(x, e, lag, fold)
    d = torch.from_numpy(y).to(cuda)
    q = n // e
    for first in (0, RUN, 3 * RUN):
        for count in (1, RUN - 1, RUN, RUN + 1, q - first):
            want = x[first * e:(first + count) * e]
            assert np.array_equal(G.unlag_delta_unshuffle_range(y, e, lag, fold, first, count), want)
            for do in (0, 3):
                dst = _aligned(torch, count * e + 2 * GUARD + 16, cuda, fill=0xA5)
                out = dst[GUARD + do:GUARD + do + count * e]
                glc.unlag_delta_unshuffle_range(d, e, lag, fold, first, count, out=out)
                assert np.array_equal(out.cpu().numpy(), want), (e, lag, fold, first, count, do)
                assert bool((dst[:GUARD + do] == 0xA5).all()) and bool((dst[GUARD + do + count * e:] == 0xA5).all())
    out = torch.full((n,), 0xA5, dtype=torch.uint8, device=cuda)
    for first in (1, RUN - 1, RUN + 8):
        with pytest.raises(glc.CudppError) as err:
            glc.unlag_delta_unshuffle_range(d, e, lag, fold, first, 10, out=out)
        assert err.value.code == ILLEGAL
    with pytest.raises(glc.CudppError):
        glc.unlag_delta_unshuffle_range(d, e, lag, fold, RUN, q, out=out)       # beyond the segment
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())


def test_refusals_leave_the_output_untouched(glc, cuda):
    import torch
    n = 4096
    src = torch.arange(n, dtype=torch.int32, device=cuda).to(torch.uint8)
    dst = torch.full((n,), 0xA5, dtype=torch.uint8, device=cuda)
    both = torch.full((2 * n,), 0xA5, dtype=torch.uint8, device=cuda)
    for fn in (glc.lag_delta_shuffle, glc.unlag_delta_unshuffle):
        for elem, lag, fold in ((4, 0, 0), (4, 17, 0), (4, 2, 2), (3, 2, 1), (0, 2, 1), (16, 2, 1), (4, 1 << 31, 0)):
            with pytest.raises(glc.CudppError) as err:
                fn(src, elem, lag, fold, out=dst)
            assert err.value.code == ILLEGAL
        for a, b in ((0, 0), (0, n - 1), (n - 1, 0), (1, 0)):
            with pytest.raises(glc.CudppError) as err:
                fn(both[a:a + n], 4, 2, 1, out=both[b:b + n])
            assert err.value.code == ILLEGAL
    for lag, fold in ((0, 0), (17, 1), (2, 2)):
        with pytest.raises(glc.CudppError) as err:
            glc.unlag_delta_unshuffle_range(src, 4, lag, fold, 0, 16, out=dst)
        assert err.value.code == ILLEGAL
    torch.cuda.synchronize()
    assert bool((dst == 0xA5).all()) and bool((both == 0xA5).all())
    both = torch.zeros(2 * n, dtype=torch.uint8, device=cuda)       # adjacent, not overlapping: accepted
    both[:n] = src
    glc.lag_delta_shuffle(both[:n], 4, 2, 1, out=both[n:])
    assert np.array_equal(both[n:].cpu().numpy(), G.lag_delta_shuffle(src.cpu().numpy(), 4, 2, 1))
