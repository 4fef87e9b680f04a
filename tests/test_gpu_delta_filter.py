"""The fused delta + shuffle kernels alone on the MI355X (-m gpu): glcDeltaShuffleDevice and glcUndeltaUnshuffleDevice against the
numpy definition of tests/container_model.py for element sizes 2, 4 and 8 -- lengths around an element, a run (2048
elements) and a 16 KiB tile, several tiles and more than 2^20 bytes; every pairing of input and output misalignments; series that
wrap, carries across the dword boundary of 8-byte elements, a run boundary inside a last partial tile; guard bytes on both sides
of the output; refusals that leave the output untouched."""
import numpy as np
import pytest

import container_model as M

pytestmark = pytest.mark.gpu

ILLEGAL = 2
RUN, TILE = 2048, 16384
OFFSETS = (0, 1, 3, 8, 15)
GUARD = 64


def _lengths(e):
    return [0, 1, e - 1, e, RUN * e - 1, RUN * e + 1, RUN * e - e, RUN * e + e, TILE - 1, TILE + 1, TILE - e, TILE + e, 3 * TILE + 5,
            (1 << 20) + 13]


def _aligned(torch, n, cuda, fill=None):
    """a device byte buffer of n bytes whose first byte is 256-byte aligned"""
    buf = torch.empty(n + 256, dtype=torch.uint8, device=cuda) if fill is None else torch.full((n + 256,), fill, dtype=torch.uint8, device=cuda)
    a = (-buf.data_ptr()) % 256
    return buf[a:a + n]


def _series(e, n, seed):
    """n bytes: a random walk of e-byte integers with steps of either sign up to a quarter of the range (differences wrap and
    sums carry through every byte), then n % e loose bytes"""
    rng = np.random.default_rng(seed)
    q = n // e
    steps = rng.integers(0, 1 << (8 * e - 2), q, dtype=np.uint64) * rng.choice(np.array([1, (1 << 64) - 1], np.uint64), q)
    x = np.cumsum(steps, dtype=np.uint64).astype("<u%d" % e).view(np.uint8)
    return np.concatenate([x, rng.integers(0, 256, n - q * e, dtype=np.uint8)])


def _check_both(glc, torch, cuda, e, x, offsets):
    """forward and inverse of x at every (input offset, output offset) of `offsets`, against the model, guards included"""
    n = x.size
    want = M.delta_shuffle(x, e)
    assert np.array_equal(M.undelta_unshuffle(want, e), x)
    d_x, d_want = torch.from_numpy(x.copy()).to(cuda), torch.from_numpy(want.copy()).to(cuda)
    src = _aligned(torch, n + 16, cuda)
    for fn, a, b in ((glc.delta_shuffle, d_x, d_want), (glc.undelta_unshuffle, d_want, d_x)):
        for so in offsets:
            src[so:so + n] = a
            for do in offsets:
                dst = _aligned(torch, n + 2 * GUARD + 16, cuda, fill=0xA5)
                out = dst[GUARD + do:GUARD + do + n]
                fn(src[so:so + n], e, out=out)
                assert torch.equal(out, b), (fn.__name__, e, n, so, do)
                assert bool((dst[:GUARD + do] == 0xA5).all()) and bool((dst[GUARD + do + n:] == 0xA5).all()), (fn.__name__, e, n, so, do)


@pytest.mark.parametrize("e", [2, 4, 8])
def test_lengths_and_alignments_against_the_model(glc, cuda, e):
    import torch
    for i, n in enumerate(_lengths(e)):
        _check_both(glc, torch, cuda, e, _series(e, n, 100 * e + i), OFFSETS)


@pytest.mark.parametrize("e", [2, 4, 8])
def test_series_that_wrap(glc, cuda, e):
    import torch
    dt, top = "<u%d" % e, (1 << (8 * e)) - 1
    q = 2 * TILE // e + RUN + 37
    descending = (np.uint64(top) - np.arange(q, dtype=np.uint64) * np.uint64(3)).astype(dt) if e == 8 else \
        ((top - 3 * np.arange(q, dtype=np.int64)) % (top + 1)).astype(dt)
    zero_max = np.tile(np.array([0, top], dtype=dt), q // 2 + 1)[:q]
    for x in (descending, zero_max):
        _check_both(glc, torch, cuda, e, np.concatenate([x.view(np.uint8), np.arange(e - 1, dtype=np.uint8)]), (0, 3))


def test_carries_cross_the_dword_boundary_of_8_byte_elements(glc, cuda):
    """values that straddle multiples of 2^32, up and down: the subtraction borrows from the high dword and the sums carry into it"""
    import torch
    rng = np.random.default_rng(8)
    q = 3 * TILE // 8 + 555
    k = rng.integers(1, 1 << 20, q, dtype=np.int64) << 32
    x = (k + rng.integers(-5, 6, q)).astype("<u8")
    d = np.diff(x)
    assert ((d >> np.uint64(32)) != ((d + np.uint64(16)) >> np.uint64(32))).any() and (x.astype(np.uint32) > 0xFFFFFFF0).any()
    _check_both(glc, torch, cuda, 8, x.view(np.uint8), (0, 1, 8))
    y = (np.int64(1 << 32) + np.cumsum(np.tile(np.array([3, -7, 5], np.int64), q // 3 + 1)[:q])).astype("<u8")   # around 2^32 itself
    _check_both(glc, torch, cuda, 8, y.view(np.uint8), (0, 15))


@pytest.mark.parametrize("e", [2, 4, 8])
def test_run_boundary_in_the_last_partial_tile(glc, cuda, e):
    """e = 2, 4: a tile holds several runs, and the last, partial tile ends 100 elements behind its second run's start;
    e = 8: a tile is one run, and the last tile is a partial run"""
    import torch
    n = TILE + (RUN + 100) * e + (e - 1) if e < 8 else 2 * TILE + 100 * e + 3
    assert 0 < n % TILE < TILE - e
    _check_both(glc, torch, cuda, e, _series(e, n, 7 + e), (0, 1, 15))


def test_refusals_leave_the_output_untouched(glc, cuda):
    import torch
    n = 4096
    src = torch.arange(n, dtype=torch.int32, device=cuda).to(torch.uint8)
    dst = torch.full((n,), 0xA5, dtype=torch.uint8, device=cuda)
    for fn in (glc.delta_shuffle, glc.undelta_unshuffle):
        for elem in (0, 1, 3, 5, 16):
            with pytest.raises(glc.CudppError) as err:
                fn(src, elem, out=dst)
            assert err.value.code == ILLEGAL
        both = torch.full((2 * n,), 0xA5, dtype=torch.uint8, device=cuda)
        for a, b in ((0, 0), (0, n - 1), (n - 1, 0), (1, 0)):
            with pytest.raises(glc.CudppError) as err:
                fn(both[a:a + n], 4, out=both[b:b + n])
            assert err.value.code == ILLEGAL
        torch.cuda.synchronize()
        assert bool((dst == 0xA5).all()) and bool((both == 0xA5).all())
    fn = glc.delta_shuffle                                      # adjacent, not overlapping: accepted
    both = torch.zeros(2 * n, dtype=torch.uint8, device=cuda)
    both[:n] = src
    fn(both[:n], 4, out=both[n:])
    assert np.array_equal(both[n:].cpu().numpy(), M.delta_shuffle(src.cpu().numpy(), 4))
