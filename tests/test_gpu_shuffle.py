"""The byte-plane shuffle kernels on the MI355X (-m gpu): forward and inverse against numpy for every element size, lengths from
0 to 64 MiB + 5 and every combination of source and destination misalignment, with guard bytes around the destination; the
batched form against the per-segment results; refusals that write nothing."""
import numpy as np
import pytest

import container_model as M

pytestmark = pytest.mark.gpu

ILLEGAL = 2
GUARD = 256
OFFSETS = (0, 1, 3, 8)


def _lengths(elem):
    return [0, 1, elem - 1, elem, 255, 4096, 65537, (1 << 20) + 3, (64 << 20) + 5]


@pytest.mark.parametrize("elem", [2, 4, 8])
def test_forward_and_inverse_equal_numpy_at_every_alignment(glc, cuda, elem):
    import torch
    rng = np.random.default_rng(elem)
    for n in _lengths(elem):
        x = rng.integers(0, 256, n, dtype=np.uint8)
        y = M.shuffle(x, elem)                                 # numpy: the reference for every alignment of this length
        assert np.array_equal(M.unshuffle(y, elem), x)
        d_x, d_y = torch.from_numpy(x).to(cuda), torch.from_numpy(y).to(cuda)
        src = torch.empty(n + 64, dtype=torch.uint8, device=cuda)
        dst = torch.empty(n + 64 + 2 * GUARD, dtype=torch.uint8, device=cuda)
        assert src.data_ptr() % 256 == 0 and dst.data_ptr() % 256 == 0
        for so in OFFSETS:
            for do in OFFSETS:
                for fn, d_in, d_want in ((glc.shuffle, d_x, d_y), (glc.unshuffle, d_y, d_x)):
                    s = src[so:so + n]
                    s.copy_(d_in)
                    dst.fill_(0xA5)
                    o = dst[GUARD + do:GUARD + do + n]
                    assert n == 0 or (s.data_ptr() % 256 == so and o.data_ptr() % 256 == do)   # (an empty view has no address)
                    fn(s, elem, out=o)
                    torch.cuda.synchronize()
                    assert torch.equal(o, d_want), (fn.__name__, elem, n, so, do)
                    assert bool((dst[:GUARD + do] == 0xA5).all()) and bool((dst[GUARD + do + n:] == 0xA5).all()), (elem, n, so, do)
                    assert torch.equal(s, d_in)                # the source is read only


@pytest.mark.parametrize("count", [1, 7, 300])
@pytest.mark.parametrize("elem", [2, 4, 8])
def test_batched_form_equals_the_per_segment_results(glc, cuda, elem, count):
    import torch
    rng = np.random.default_rng(100 * elem + count)
    lens = rng.choice([0, 0, 1, elem - 1, elem, elem + 1, 37, 255, 4096, 16384, 16385, 70001, 300007], count).astype(np.int64)
    if count > 1:
        lens[1], lens[-1] = 0, (1 << 20) + 3
    gaps = rng.integers(0, 40, count)
    offs = np.cumsum(np.concatenate([[5], lens[:-1] + gaps[:-1]])).astype(np.int64)   # any alignment, never overlapping
    total = int(offs[-1] + lens[-1]) + 64
    x = rng.integers(0, 256, total, dtype=np.uint8)
    want_f = np.full(total, 0x5A, np.uint8)
    for o, n in zip(offs, lens):
        want_f[o:o + n] = M.shuffle(x[o:o + n], elem)
    d_x = torch.from_numpy(x).to(cuda)
    out = torch.full((total,), 0x5A, dtype=torch.uint8, device=cuda)
    glc.shuffle_segments(d_x, out, offs, lens, elem)
    assert np.array_equal(out.cpu().numpy(), want_f)           # segments shuffled, every byte between them untouched
    for i in (0, count // 2, count - 1):                       # ... and equal to the single-segment form
        o, n = int(offs[i]), int(lens[i])
        if n:
            assert torch.equal(glc.shuffle(d_x[o:o + n].clone(), elem), out[o:o + n])
    back = torch.full((total,), 0x5A, dtype=torch.uint8, device=cuda)
    glc.shuffle_segments(out, back, offs, lens, elem, inverse=True)
    want_b = np.full(total, 0x5A, np.uint8)
    for o, n in zip(offs, lens):
        want_b[o:o + n] = x[o:o + n]
    assert np.array_equal(back.cpu().numpy(), want_b)


def test_bad_arguments_are_refused_with_nothing_written(glc, cuda):
    import torch
    n = 4096
    x = torch.arange(n, dtype=torch.int32, device=cuda).to(torch.uint8)
    out = torch.full((n,), 0xA5, dtype=torch.uint8, device=cuda)
    for fn in (glc.shuffle, glc.unshuffle):
        for elem in (0, 1, 3, 6, 16):
            with pytest.raises(glc.CudppError) as e:
                fn(x, elem, out=out)
            assert e.value.code == ILLEGAL
        buf = torch.arange(2 * n, dtype=torch.int32, device=cuda).to(torch.uint8)
        keep = buf.clone()
        for a, b in ((0, 0), (0, 1), (1, 0), (0, n - 1), (n - 1, 0)):
            with pytest.raises(glc.CudppError) as e:
                fn(buf[a:a + n], 4, out=buf[b:b + n])
            assert e.value.code == ILLEGAL
        fn(buf[:n], 4, out=buf[n:])                            # adjacent is not overlapping
        torch.cuda.synchronize()
        assert torch.equal(buf[:n], keep[:n])
        buf.copy_(keep)
        off = torch.zeros(1, dtype=torch.int64, device=cuda)
        ln = torch.full((1,), n, dtype=torch.int64, device=cuda)
        name = "glcShuffleSegments" if fn is glc.shuffle else "glcUnshuffleSegments"
        for elem, src, dst in ((3, x, out), (4, buf, buf)):
            rc = getattr(glc._ct(), name)(src.data_ptr(), dst.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, elem, None)
            assert rc == ILLEGAL
        torch.cuda.synchronize()
        assert bool((out == 0xA5).all()) and torch.equal(buf, keep)
