"""The range forms of the two inverse filters on the MI355X (-m gpu): glcUnshuffleRangeDevice and glcUndeltaUnshuffleRangeDevice
against slices of container_model.unshuffle / undelta_unshuffle, for every element size, a segment of one short tile and one of
several tiles with a ragged last tile and a byte tail, ranges at every edge the tiling has, and both buffers at byte offsets 0, 1
and 5.  Every call runs twice, with the input bytes outside the elem plane runs [j q + first, + count) filled with 0xA5 and with
0x5A: the outputs must be the reference both times, so nothing outside those runs is an input.  64 guard bytes either side of the
output stay as they were.  Refused calls write nothing."""
import numpy as np
import pytest

import container_model as M

pytestmark = pytest.mark.gpu

ILLEGAL = 2
GUARD = 64
OFFSETS = (0, 1, 5)
RUN = 2048


def _lens(elem):
    return (16 * elem, 5 * 16384 + 3 * elem + 1)


def _ranges(elem, q, delta):
    """(first, count): whole; one element; the last element; across a tile edge; across a 2048 boundary; a misaligned first"""
    tq = 16384 // elem
    if q == 16:
        return [(0, 16), (0, 1), (0, 15), (0, 7)] if delta else [(0, 16), (0, 1), (15, 1), (0, 7), (5, 1), (3, 7), (9, 7)]
    assert q > 2 * tq and q % tq and q > 2 * RUN
    if delta:
        # first is a run start: the tile edge and the 2048 boundary are crossed from the run start in front of them
        edge = (tq - RUN, RUN + 9) if tq > RUN else (0, tq + 9)
        return [(0, q), (RUN, 1), ((q - 1) // RUN * RUN, q - (q - 1) // RUN * RUN), edge, (RUN, RUN + 3), (2 * RUN, 1234),
                (q // tq * tq, q - q // tq * tq)]
    return [(0, q), (tq + 77, 1), (q - 1, 1), (tq - 3, 7), (RUN - 5, 11), (13, 1001), (2 * tq - 1, q - 2 * tq + 1), (q - 19, 19)]


_REF = {}


def _case(elem, length, delta):
    """(original, filtered) of one seeded segment; the reference is the model's inverse of the filtered bytes, computed once"""
    key = (elem, length, delta)
    if key not in _REF:
        rng = np.random.default_rng(1000 * elem + length % 997 + (7 if delta else 0))
        x = rng.integers(0, 256, length, dtype=np.uint8)
        if delta:                                               # slowly varying elements: the sums carry across bytes
            v = np.cumsum(rng.integers(0, 300, length // elem, dtype=np.uint64)).astype("<u%d" % elem)
            x[:length - length % elem] = v.view(np.uint8)
        f = np.asarray((M.delta_shuffle if delta else M.shuffle)(x, elem), np.uint8)
        ref = np.asarray((M.undelta_unshuffle if delta else M.unshuffle)(f, elem), np.uint8)
        assert np.array_equal(ref, x)
        _REF[key] = (ref, f)
    return _REF[key]


def _run(glc, cuda, elem, delta, f, first, count, off_in, off_out, fill):
    """one call on a copy of the filtered segment in which every byte outside the elem plane runs is `fill`; returns the output
    buffer with its guards"""
    import torch
    q = f.size // elem
    host = np.full(GUARD + off_in + f.size + GUARD, fill, np.uint8)
    for j in range(elem):
        host[GUARD + off_in + j * q + first: GUARD + off_in + j * q + first + count] = f[j * q + first: j * q + first + count]
    d_in = torch.from_numpy(host).to(cuda)
    d_out = torch.full((GUARD + off_out + count * elem + GUARD,), 0xCD, dtype=torch.uint8, device=cuda)
    fn = glc.undelta_unshuffle_range if delta else glc.unshuffle_range
    fn(d_in[GUARD + off_in: GUARD + off_in + f.size], elem, first, count, out=d_out[GUARD + off_out: GUARD + off_out + count * elem])
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("delta", [False, True])
@pytest.mark.parametrize("elem", [2, 4, 8])
def test_range_equals_the_sliced_whole_inverse(glc, cuda, elem, delta):
    for length in _lens(elem):
        ref, f = _case(elem, length, delta)
        q = length // elem
        for first, count in _ranges(elem, q, delta):
            assert count >= 1 and first + count <= q and (not delta or first % RUN == 0)
            want = ref[first * elem:(first + count) * elem]
            for off_in in OFFSETS:
                for off_out in OFFSETS:
                    if length > 16 * elem and count > 4096 and (off_in, off_out) not in ((0, 0), (1, 5), (5, 1)):
                        continue                                # the long ranges: three of the nine offset pairs
                    for fill in (0xA5, 0x5A):
                        got = _run(glc, cuda, elem, delta, f, first, count, off_in, off_out, fill)
                        lo = GUARD + off_out
                        where = (length, first, count, off_in, off_out, fill)
                        assert np.array_equal(got[lo:lo + count * elem], want), where
                        assert (got[:lo] == 0xCD).all() and (got[lo + count * elem:] == 0xCD).all(), where


@pytest.mark.parametrize("delta", [False, True])
def test_refusals_write_nothing(glc, cuda, delta):
    import torch
    elem, length = 4, 5 * 16384 + 13
    _, f = _case(elem, length, delta)
    q = length // elem
    d_in = torch.from_numpy(f.copy()).to(cuda)
    out = torch.full((length,), 0xCD, dtype=torch.uint8, device=cuda)
    fn = "glcUndeltaUnshuffleRangeDevice" if delta else "glcUnshuffleRangeDevice"
    call = getattr(glc._ct(), fn)
    bad = [(d_in.data_ptr(), out.data_ptr(), length, elem, q, 1),                       # first + count > q
           (d_in.data_ptr(), out.data_ptr(), length, elem, 0, q + 1),
           (d_in.data_ptr(), out.data_ptr(), length, elem, 1 << 63, 1 << 63),           # ... and where the sum wraps
           (d_in.data_ptr(), out.data_ptr(), length, 3, 0, 4),                          # elem
           (d_in.data_ptr(), out.data_ptr(), length, 16, 0, 4),
           (d_in.data_ptr(), None, length, elem, 0, 4),                                 # null
           (None, out.data_ptr(), length, elem, 0, 4),
           (d_in.data_ptr(), d_in.data_ptr() + 64, length, elem, 0, 4),                 # the output overlaps the segment
           (d_in.data_ptr(), d_in.data_ptr() + length - 1, length, elem, 0, 4),
           (d_in.data_ptr() + 8, d_in.data_ptr(), length - 8, elem, 0, 4)]              # ... its end reaches into it
    if delta:
        bad += [(d_in.data_ptr(), out.data_ptr(), length, elem, 100, 4), (d_in.data_ptr(), out.data_ptr(), length, elem, 2047, 1)]
    for args in bad:
        assert call(*args, None) == ILLEGAL, args
    torch.cuda.synchronize()
    assert bool((out == 0xCD).all()) and np.array_equal(d_in.cpu().numpy(), f)
    assert call(d_in.data_ptr(), out.data_ptr(), length, elem, 0, 0, None) == 0         # nothing asked for, nothing written
    assert call(d_in.data_ptr(), out.data_ptr(), length, elem, q // RUN * RUN if delta else q, 0, None) == 0
    # the output may touch the segment's ends without overlapping it
    both = torch.full((length + 64,), 0xCD, dtype=torch.uint8, device=cuda)
    both[16:16 + length] = d_in
    assert call(both.data_ptr() + 16, both.data_ptr(), length, elem, 0, 4, None) == 0
    assert call(both.data_ptr() + 16, both.data_ptr() + 16 + length, length, elem, 0, 4, None) == 0
    torch.cuda.synchronize()
    assert bool((out == 0xCD).all())
