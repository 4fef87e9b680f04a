"""The 3-D predictor's kernels alone on the MI355X (-m gpu): glcVolDeltaShuffleDevice, glcUnvolDeltaUnshuffleDevice and
glcUnvolDeltaUnshuffleRangeDevice against the numpy definition of tests/vol_model.py, byte for byte, over element sizes 2, 4, 8 x
widths 5, 64, 100 x plane strides W + 1, 1000 (S elem a multiple of 16: k_grid_vsum's 16-byte path up the slabs), 1003 and 7 W + 3
(neither a multiple of 16 nor of W: its element path), 5000 (the plane behind lies beyond the tile) x fold 0, 1 x lengths 0, less
than one plane, and about 2.5 slabs with a ragged tail; input and output bases offset by 0, 1, 3 and 7 bytes; 64 guard bytes on each
side of the output; a stride at or beyond the segment, where the bytes are glcGridDeltaShuffleDevice's; the largest stride and
width; values that force carries; ranges; refusals that leave the output untouched."""
import numpy as np
import pytest

import grid_model as G
import vol_model as V

pytestmark = pytest.mark.gpu

ILLEGAL = 2
ELEMS, WIDTHS, FOLDS = (2, 4, 8), (5, 64, 100), (0, 1)
OFFSETS = ((0, 0), (1, 3), (3, 7), (7, 1))                       # (input, output)
GUARD = 64


def _planes(W):
    return (W + 1, 1000, 1003, 7 * W + 3, 5000)


def _lengths(e, W, S):
    Q = V.slab(W, S)
    return [0, S * e - 1, 5 * Q * e // 2 + 3 * e + (e - 1)]


def _aligned(torch, n, cuda, fill=None):
    """a device byte buffer of n bytes whose first byte is 256-byte aligned"""
    buf = torch.empty(n + 256, dtype=torch.uint8, device=cuda) if fill is None else torch.full((n + 256,), fill, dtype=torch.uint8, device=cuda)
    a = (-buf.data_ptr()) % 256
    return buf[a:a + n]


def _random(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _check_both(glc, torch, cuda, e, W, S, fold, x, offsets, want=None):
    """forward and inverse of x at every (input offset, output offset) of `offsets`, against the model, guards included"""
    n = x.size
    if want is None:
        want = V.vol_delta_shuffle(x, e, W, S, fold)
        assert np.array_equal(V.unvol_delta_unshuffle(want, e, W, S, fold), x)
    d_x, d_want = torch.from_numpy(x.copy()).to(cuda), torch.from_numpy(want.copy()).to(cuda)
    src = _aligned(torch, n + 16, cuda)
    for fn, a, b in ((glc.vol_delta_shuffle, d_x, d_want), (glc.unvol_delta_unshuffle, d_want, d_x)):
        for so, do in offsets:
            src[so:so + n] = a
            dst = _aligned(torch, n + 2 * GUARD + 16, cuda, fill=0xA5)
            out = dst[GUARD + do:GUARD + do + n]
            fn(src[so:so + n], e, W, S, fold, out=out)
            assert torch.equal(out, b), (fn.__name__, e, W, S, fold, n, so, do)
            assert bool((dst[:GUARD + do] == 0xA5).all()) and bool((dst[GUARD + do + n:] == 0xA5).all()), (fn.__name__, e, W, S, fold, n, so, do)


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("e", ELEMS)
def test_lengths_against_the_model(glc, cuda, e, W):
    import torch
    for S in _planes(W):
        for fold in FOLDS:
            for i, n in enumerate(_lengths(e, W, S)):
                _check_both(glc, torch, cuda, e, W, S, fold, _random(n, 1000 * e + 10 * W + S + i), OFFSETS if n else OFFSETS[:1])


@pytest.mark.parametrize("e", ELEMS)
def test_no_plane_behind_is_the_grid_call(glc, cuda, e):
    """S >= q: no element has a plane behind it, and the bytes are glcGridDeltaShuffleDevice's"""
    import torch
    for W, fold in ((5, 1), (100, 0)):
        n = 3 * G.period(W) * e + 5 * e + 1
        x = _random(n, 31 * e + W)
        d = torch.from_numpy(x).to(cuda)
        grid = glc.grid_delta_shuffle(d, e, W, fold)
        assert np.array_equal(grid.cpu().numpy(), G.grid_delta_shuffle(x, e, W, fold))
        for S in (n // e, n // e + 1, 1 << 24):
            y = glc.vol_delta_shuffle(d, e, W, S, fold)
            assert torch.equal(y, grid), (e, W, S)
            assert torch.equal(glc.unvol_delta_unshuffle(y, e, W, S, fold), d)


def test_the_largest_width_and_a_stride_beyond_it(glc, cuda):
    """W = 65536 with 8-byte elements and S = W + 1: the row above and the plane behind lie 512 KiB back, P = 2^21 and Q = 2^21
    elements: one slab of 31 planes and a ragged one"""
    import torch
    W, e = 65536, 8
    S = W + 1
    assert V.slab(W, S) == G.period(W) == 1 << 21
    n = (V.slab(W, S) + 2 * S + 5) * e + 3
    _check_both(glc, torch, cuda, e, W, S, 1, _random(n, 65537), OFFSETS[:2])


@pytest.mark.parametrize("e", ELEMS)
def test_values_that_force_carries(glc, cuda, e):
    import torch
    dt, top = "<u%d" % e, (1 << (8 * e)) - 1
    W, S = 24, 24 * 9 + 5
    q = V.slab(W, S) + 3 * S + 7
    ones = np.full(q, top, dtype=dt)
    alternating = np.tile(np.array([0, 1 << (8 * e - 1)], dtype=dt), q // 2 + 1)[:q]
    ramp = (np.arange(q, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).astype(dt)      # every sum and difference wraps somewhere
    for fold in FOLDS:
        for x in (ones, alternating, ramp):
            _check_both(glc, torch, cuda, e, W, S, fold, np.concatenate([x.view(np.uint8), np.arange(e - 1, dtype=np.uint8)]), OFFSETS[:2])


@pytest.mark.parametrize("W,S,fold", [(5, 6, 1), (64, 1000, 0), (100, 1003, 1), (100, 5000, 0)])
@pytest.mark.parametrize("e", ELEMS)
def test_range_inverse(glc, cuda, e, W, S, fold):
    import torch
    Q = V.slab(W, S)
    n = 5 * Q * e // 2 + 3 * e + (e - 1)                          # two slabs and a ragged third
    x = _random(n, 7 * e + W + S)
    y = V.vol_delta_shuffle(x, e, W, S, fold)
    d = torch.from_numpy(y).to(cuda)
    q = n // e
    for first in (0, Q, 2 * Q):
        for count in (1, Q - 1, q - first):
            if first + count > q:
                continue
            want = x[first * e:(first + count) * e]
            for do in (0, 3):
                dst = _aligned(torch, count * e + 2 * GUARD + 16, cuda, fill=0xA5)
                out = dst[GUARD + do:GUARD + do + count * e]
                glc.unvol_delta_unshuffle_range(d, e, W, S, fold, first, count, out=out)
                assert np.array_equal(out.cpu().numpy(), want), (e, W, S, fold, first, count, do)
                assert bool((dst[:GUARD + do] == 0xA5).all()) and bool((dst[GUARD + do + count * e:] == 0xA5).all())
    out = torch.full((n,), 0xA5, dtype=torch.uint8, device=cuda)
    for first in (1, 2048, G.period(W), Q - 1, Q + 8):
        if first % Q:
            with pytest.raises(glc.CudppError) as err:
                glc.unvol_delta_unshuffle_range(d, e, W, S, fold, first, 10, out=out)
            assert err.value.code == ILLEGAL
    with pytest.raises(glc.CudppError):
        glc.unvol_delta_unshuffle_range(d, e, W, S, fold, Q, q, out=out)        # beyond the segment
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())


def test_refusals_leave_the_output_untouched(glc, cuda):
    import torch
    n = 4096
    src = torch.arange(n, dtype=torch.int32, device=cuda).to(torch.uint8)
    dst = torch.full((n,), 0xA5, dtype=torch.uint8, device=cuda)
    both = torch.full((2 * n,), 0xA5, dtype=torch.uint8, device=cuda)
    bad = ((4, 0, 300, 0), (4, 1, 300, 0), (4, 65537, 70000, 0), (4, 64, 300, 2), (3, 64, 300, 1), (0, 64, 300, 1), (16, 64, 300, 1), (4, 64, 64, 1),
           (4, 64, 63, 1), (4, 64, 0, 0), (4, 64, (1 << 24) + 1, 1), (4, 64, 1 << 31, 0), (4, 65536, 65536, 0))
    for fn in (glc.vol_delta_shuffle, glc.unvol_delta_unshuffle):
        for elem, width, plane, fold in bad:
            with pytest.raises(glc.CudppError) as err:
                fn(src, elem, width, plane, fold, out=dst)
            assert err.value.code == ILLEGAL
        for a, b in ((0, 0), (0, n - 1), (n - 1, 0), (1, 0)):
            with pytest.raises(glc.CudppError) as err:
                fn(both[a:a + n], 4, 64, 300, 1, out=both[b:b + n])
            assert err.value.code == ILLEGAL
    for elem, width, plane, fold in bad:
        with pytest.raises(glc.CudppError) as err:
            glc.unvol_delta_unshuffle_range(src, elem, width, plane, fold, 0, 16, out=dst)
        assert err.value.code == ILLEGAL
    torch.cuda.synchronize()
    assert bool((dst == 0xA5).all()) and bool((both == 0xA5).all())
    both = torch.zeros(2 * n, dtype=torch.uint8, device=cuda)       # adjacent, not overlapping: accepted
    both[:n] = src
    glc.vol_delta_shuffle(both[:n], 4, 64, 300, 1, out=both[n:])
    assert np.array_equal(both[n:].cpu().numpy(), V.vol_delta_shuffle(src.cpu().numpy(), 4, 64, 300, 1))
