"""The byte predictor's kernels alone on the MI355X (-m gpu): glcByteDeltaDevice, glcUnbyteDeltaDevice and glcUnbyteDeltaRangeDevice
against the numpy definition of tests/byte_delta_model.py, byte for byte, over lags 1, 2, 3, 4, 5, 8, 16 x strides 0, 2, 3, 15, 16, 64,
65, 600, 1281, 4096 x lengths around the lag, a run, a row, a band and a tile; stride 65536 (a row longer than a tile, P = 2 MiB);
input and output bases misaligned by every pairing of 0, 1, 3 and 15 bytes; 64 guard bytes of 0xA5 on each side of the output;
values that would show a carry leaking between the packed bytes of a dword; 70 tiles; ranges; refusals that leave the output
untouched."""
import numpy as np
import pytest

import byte_delta_model as B

pytestmark = pytest.mark.gpu

ILLEGAL = 2
LAGS, STRIDES = (1, 2, 3, 4, 5, 8, 16), (0, 2, 3, 15, 16, 64, 65, 600, 1281, 4096)
OFFSETS = ((0, 0), (1, 3), (3, 15), (15, 1))                     # (input, output)
ALL_OFFSETS = tuple((a, b) for a in (0, 1, 3, 15) for b in (0, 1, 3, 15))
GUARD, TILE = 64, 16384


def _lengths(lag, S):
    P = B.step(S)
    want = [0, 1, lag - 1, lag, lag + 1, 2047, 2048, 2049, S - 1, S, S + 1, P - 1, P, P + 1, TILE, TILE + lag + 3, 3 * TILE + 5, 2 * P + S + 7]
    return sorted({n for n in want if n >= 0})


def _aligned(torch, n, cuda, fill=None):
    """a device byte buffer of n bytes whose first byte is 256-byte aligned"""
    buf = torch.empty(n + 256, dtype=torch.uint8, device=cuda) if fill is None else torch.full((n + 256,), fill, dtype=torch.uint8, device=cuda)
    a = (-buf.data_ptr()) % 256
    return buf[a:a + n]


def _random(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _check_both(glc, torch, cuda, lag, S, x, offsets):
    """forward and inverse of x at every (input offset, output offset) of `offsets`, against the model, guards included"""
    n = x.size
    want = B.byte_delta(x, lag, S)
    assert want.size == n and np.array_equal(B.unbyte_delta(want, lag, S), x)
    d_x, d_want = torch.from_numpy(x.copy()).to(cuda), torch.from_numpy(want.copy()).to(cuda)
    src = _aligned(torch, n + 16, cuda)
    for fn, a, b in ((glc.byte_delta, d_x, d_want), (glc.unbyte_delta, d_want, d_x)):
        for so, do in offsets:
            src[so:so + n] = a
            dst = _aligned(torch, n + 2 * GUARD + 16, cuda, fill=0xA5)
            out = dst[GUARD + do:GUARD + do + n]
            fn(src[so:so + n], lag, S, out=out)
            assert torch.equal(out, b), (fn.__name__, lag, S, n, so, do)
            assert bool((dst[:GUARD + do] == 0xA5).all()) and bool((dst[GUARD + do + n:] == 0xA5).all()), (fn.__name__, lag, S, n, so, do)


@pytest.mark.parametrize("S", STRIDES)
@pytest.mark.parametrize("lag", LAGS)
def test_lengths_against_the_model(glc, cuda, lag, S):
    import torch
    for i, n in enumerate(_lengths(lag, S)):
        _check_both(glc, torch, cuda, lag, S, _random(n, 1000 * lag + 10 * S + i), OFFSETS if n else OFFSETS[:1])


def test_a_row_longer_than_a_tile(glc, cuda):
    """stride 65536: the row above lies four tiles back, P = 2 MiB; two bands and a ragged third, about 4.1 MiB"""
    import torch
    S = 65536
    P = B.period(S)
    assert P == 1 << 21
    _check_both(glc, torch, cuda, 3, S, _random(2 * P + S + 7, 65536), OFFSETS[:2])


@pytest.mark.parametrize("S", (0, 3, 1281))
@pytest.mark.parametrize("lag", LAGS)
def test_every_pairing_of_misalignments(glc, cuda, lag, S):
    import torch
    P = B.step(S)
    for i, n in enumerate((2049, TILE + lag + 3, 2 * P + S + 7)):
        _check_both(glc, torch, cuda, lag, S, _random(n, 77 * lag + S + i), ALL_OFFSETS)


@pytest.mark.parametrize("S", (0, 3))
@pytest.mark.parametrize("lag", (1, 2, 3))
def test_values_that_would_leak_a_carry_between_packed_bytes(glc, cuda, lag, S):
    import torch
    n = 2 * 2048 + 37
    for pattern in ((0xFF,), (0x00, 0xFF), (0x00, 0x80), (0x7F, 0x80, 0x7F, 0x80)):
        x = np.tile(np.array(pattern, np.uint8), n // len(pattern) + 1)[:n]
        _check_both(glc, torch, cuda, lag, S, x, OFFSETS)
    ramp = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) >> np.uint64(56)).astype(np.uint8)
    _check_both(glc, torch, cuda, lag, S, ramp, OFFSETS[:2])


@pytest.mark.parametrize("lag,S", [(1, 0), (3, 1281)])
def test_seventy_tiles(glc, cuda, lag, S):
    import torch
    _check_both(glc, torch, cuda, lag, S, _random(70 * TILE + 11, 70 + lag), OFFSETS[:2])


@pytest.mark.parametrize("lag,S", [(1, 0), (3, 0), (2, 65), (16, 600), (3, 1281)])
def test_range_inverse(glc, cuda, lag, S):
    import torch
    step = B.step(S)
    n = 4 * step + S + 777
    x = _random(n, 7 * lag + S)
    y = B.byte_delta(x, lag, S)
    d = torch.from_numpy(y).to(cuda)
    for first in (0, step, 3 * step):
        for count in (1, step - 1, step, step + 1, n - first):
            want = x[first:first + count]
            assert np.array_equal(B.unbyte_delta_range(y, lag, S, first, count), want)
            for do in (0, 3):
                dst = _aligned(torch, count + 2 * GUARD + 16, cuda, fill=0xA5)
                out = dst[GUARD + do:GUARD + do + count]
                glc.unbyte_delta_range(d, lag, S, first, count, out=out)
                assert np.array_equal(out.cpu().numpy(), want), (lag, S, first, count, do)
                assert bool((dst[:GUARD + do] == 0xA5).all()) and bool((dst[GUARD + do + count:] == 0xA5).all())
    out = torch.full((n + 1,), 0xA5, dtype=torch.uint8, device=cuda)
    for first in (1, 1024, step - 1, step + 8) + ((2048,) if step > 2048 else ()):      # a misaligned first
        with pytest.raises(glc.CudppError) as err:
            glc.unbyte_delta_range(d, lag, S, first, 10, out=out)
        assert err.value.code == ILLEGAL
    for first, count in ((step, n), (0, n + 1), (4 * step, S + 778)):                   # beyond the segment
        with pytest.raises(glc.CudppError) as err:
            glc.unbyte_delta_range(d, lag, S, first, count, out=out)
        assert err.value.code == ILLEGAL
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())


def test_refusals_leave_the_output_untouched(glc, cuda):
    import torch
    n = 4096
    src = torch.arange(n, dtype=torch.int32, device=cuda).to(torch.uint8)
    dst = torch.full((n,), 0xA5, dtype=torch.uint8, device=cuda)
    both = torch.full((2 * n,), 0xA5, dtype=torch.uint8, device=cuda)
    for fn in (glc.byte_delta, glc.unbyte_delta):
        for lag, stride in ((0, 0), (17, 0), (1 << 31, 0), (1, 1), (3, 1), (3, 65537), (3, 1 << 31), (0, 600), (17, 600)):
            with pytest.raises(glc.CudppError) as err:
                fn(src, lag, stride, out=dst)
            assert err.value.code == ILLEGAL
        for a, b in ((0, 0), (0, n - 1), (n - 1, 0), (1, 0)):
            with pytest.raises(glc.CudppError) as err:
                fn(both[a:a + n], 3, 64, out=both[b:b + n])
            assert err.value.code == ILLEGAL
    for lag, stride in ((0, 0), (17, 64), (3, 1), (3, 65537)):
        with pytest.raises(glc.CudppError) as err:
            glc.unbyte_delta_range(src, lag, stride, 0, 16, out=dst)
        assert err.value.code == ILLEGAL
    with pytest.raises(glc.CudppError) as err:
        glc.unbyte_delta_range(both, 3, 64, 0, 16, out=both[8:])          # overlapping
    assert err.value.code == ILLEGAL
    torch.cuda.synchronize()
    assert bool((dst == 0xA5).all()) and bool((both == 0xA5).all())
    both = torch.zeros(2 * n, dtype=torch.uint8, device=cuda)       # adjacent, not overlapping: accepted
    both[:n] = src
    glc.byte_delta(both[:n], 3, 64, out=both[n:])
    assert np.array_equal(both[n:].cpu().numpy(), B.byte_delta(src.cpu().numpy(), 3, 64))
    glc.unbyte_delta(both[n:], 3, 64, out=both[:n])
    assert torch.equal(both[:n], src)
