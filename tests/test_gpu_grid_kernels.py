"""The 2-D predictor's kernels alone on the MI355X (-m gpu): glcGridDeltaShuffleDevice, glcUngridDeltaUnshuffleDevice and
glcUngridDeltaUnshuffleRangeDevice against the numpy definition of tests/grid_model.py, byte for byte, over element sizes 2, 4, 8 x
widths 2, 3, 63, 64, 65, 1000, 4096 x fold 0, 1 x lengths 0, elem - 1, W elem - 1 (one ragged row), P elem (one band) and two bands
plus 777 elements and a ragged tail; width 65536 with 8-byte elements (a row longer than a tile, one band and a ragged one); input
and output bases offset by 0, 1 and 3 bytes, which takes k_grid_vsum down both of its paths (16-byte accesses need W elem and the
output address to be multiples of 16); 64 guard bytes on each side of the output; values that force carries; ranges; refusals that
leave the output untouched."""
import numpy as np
import pytest

import grid_model as G

pytestmark = pytest.mark.gpu

ILLEGAL = 2
ELEMS, WIDTHS, FOLDS = (2, 4, 8), (2, 3, 63, 64, 65, 1000, 4096), (0, 1)
OFFSETS = ((0, 0), (1, 3), (3, 1), (0, 1))                       # (input, output)
GUARD = 64


def _lengths(e, W):
    P = G.period(W)
    return [0, e - 1, W * e - 1, P * e, 2 * P * e + 777 * e + (e - 1)]


def _aligned(torch, n, cuda, fill=None):
    """a device byte buffer of n bytes whose first byte is 256-byte aligned"""
    buf = torch.empty(n + 256, dtype=torch.uint8, device=cuda) if fill is None else torch.full((n + 256,), fill, dtype=torch.uint8, device=cuda)
    a = (-buf.data_ptr()) % 256
    return buf[a:a + n]


def _random(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _check_both(glc, torch, cuda, e, W, fold, x, offsets):
    """forward and inverse of x at every (input offset, output offset) of `offsets`, against the model, guards included"""
    n = x.size
    want = G.grid_delta_shuffle(x, e, W, fold)
    assert np.array_equal(G.ungrid_delta_unshuffle(want, e, W, fold), x)
    d_x, d_want = torch.from_numpy(x.copy()).to(cuda), torch.from_numpy(want.copy()).to(cuda)
    src = _aligned(torch, n + 16, cuda)
    for fn, a, b in ((glc.grid_delta_shuffle, d_x, d_want), (glc.ungrid_delta_unshuffle, d_want, d_x)):
        for so, do in offsets:
            src[so:so + n] = a
            dst = _aligned(torch, n + 2 * GUARD + 16, cuda, fill=0xA5)
            out = dst[GUARD + do:GUARD + do + n]
            fn(src[so:so + n], e, W, fold, out=out)
            assert torch.equal(out, b), (fn.__name__, e, W, fold, n, so, do)
            assert bool((dst[:GUARD + do] == 0xA5).all()) and bool((dst[GUARD + do + n:] == 0xA5).all()), (fn.__name__, e, W, fold, n, so, do)


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("e", ELEMS)
def test_lengths_against_the_model(glc, cuda, e, W):
    import torch
    for fold in FOLDS:
        for i, n in enumerate(_lengths(e, W)):
            _check_both(glc, torch, cuda, e, W, fold, _random(n, 1000 * e + 10 * W + i), OFFSETS if n else OFFSETS[:1])


def test_a_row_longer_than_a_tile(glc, cuda):
    """W = 65536 with 8-byte elements: the row above lies 512 KiB back, P = 2^21 elements; one full band plus a ragged one"""
    import torch
    W, e = 65536, 8
    n = (G.period(W) + 2048 + 5) * e + 3
    _check_both(glc, torch, cuda, e, W, 1, _random(n, 65536), OFFSETS[:2])


@pytest.mark.parametrize("e", ELEMS)
def test_values_that_force_carries(glc, cuda, e):
    import torch
    dt, top = "<u%d" % e, (1 << (8 * e)) - 1
    W = 24
    q = G.period(W) + 5 * W + 7
    ones = np.full(q, top, dtype=dt)
    alternating = np.tile(np.array([0, 1 << (8 * e - 1)], dtype=dt), q // 2 + 1)[:q]
    ramp = (np.arange(q, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).astype(dt)      # every sum and difference wraps somewhere
    for fold in FOLDS:
        for x in (ones, alternating, ramp):
            _check_both(glc, torch, cuda, e, W, fold, np.concatenate([x.view(np.uint8), np.arange(e - 1, dtype=np.uint8)]), OFFSETS[:2])


@pytest.mark.parametrize("W,fold", [(65, 1), (64, 0), (1000, 1), (2, 0)])
@pytest.mark.parametrize("e", ELEMS)
def test_range_inverse(glc, cuda, e, W, fold):
    import torch
    P = G.period(W)
    n = 2 * P * e + 777 * e + (e - 1)                             # two bands and a ragged third
    x = _random(n, 7 * e + W)
    y = G.grid_delta_shuffle(x, e, W, fold)
    d = torch.from_numpy(y).to(cuda)
    q = n // e
    for first in (0, P, 2 * P):
        for count in (1, P - 1, q - first):
            if first + count > q:
                continue
            want = x[first * e:(first + count) * e]
            assert np.array_equal(G.ungrid_delta_unshuffle_range(y, e, W, fold, first, count), want)
            for do in (0, 3):
                dst = _aligned(torch, count * e + 2 * GUARD + 16, cuda, fill=0xA5)
                out = dst[GUARD + do:GUARD + do + count * e]
                glc.ungrid_delta_unshuffle_range(d, e, W, fold, first, count, out=out)
                assert np.array_equal(out.cpu().numpy(), want), (e, W, fold, first, count, do)
                assert bool((dst[:GUARD + do] == 0xA5).all()) and bool((dst[GUARD + do + count * e:] == 0xA5).all())
    out = torch.full((n,), 0xA5, dtype=torch.uint8, device=cuda)
    for first in (1, 2048 if P > 2048 else 1024, P - 1, P + 8):
        with pytest.raises(glc.CudppError) as err:
            glc.ungrid_delta_unshuffle_range(d, e, W, fold, first, 10, out=out)
        assert err.value.code == ILLEGAL
    with pytest.raises(glc.CudppError):
        glc.ungrid_delta_unshuffle_range(d, e, W, fold, P, q, out=out)          # beyond the segment
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())


def test_refusals_leave_the_output_untouched(glc, cuda):
    import torch
    n = 4096
    src = torch.arange(n, dtype=torch.int32, device=cuda).to(torch.uint8)
    dst = torch.full((n,), 0xA5, dtype=torch.uint8, device=cuda)
    both = torch.full((2 * n,), 0xA5, dtype=torch.uint8, device=cuda)
    for fn in (glc.grid_delta_shuffle, glc.ungrid_delta_unshuffle):
        for elem, width, fold in ((4, 0, 0), (4, 1, 0), (4, 65537, 0), (4, 64, 2), (3, 64, 1), (0, 64, 1), (16, 64, 1), (4, 1 << 31, 0)):
            with pytest.raises(glc.CudppError) as err:
                fn(src, elem, width, fold, out=dst)
            assert err.value.code == ILLEGAL
        for a, b in ((0, 0), (0, n - 1), (n - 1, 0), (1, 0)):
            with pytest.raises(glc.CudppError) as err:
                fn(both[a:a + n], 4, 64, 1, out=both[b:b + n])
            assert err.value.code == ILLEGAL
    for width, fold in ((0, 0), (1, 1), (65537, 1), (64, 2)):
        with pytest.raises(glc.CudppError) as err:
            glc.ungrid_delta_unshuffle_range(src, 4, width, fold, 0, 16, out=dst)
        assert err.value.code == ILLEGAL
    torch.cuda.synchronize()
    assert bool((dst == 0xA5).all()) and bool((both == 0xA5).all())
    both = torch.zeros(2 * n, dtype=torch.uint8, device=cuda)       # adjacent, not overlapping: accepted
    both[:n] = src
    glc.grid_delta_shuffle(both[:n], 4, 64, 1, out=both[n:])
    assert np.array_equal(both[n:].cpu().numpy(), G.grid_delta_shuffle(src.cpu().numpy(), 4, 64, 1))
