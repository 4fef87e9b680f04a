"""The zero-run passes on the MI355X (-m gpu): glcZeroRunSplitSegments and glcZeroRunJoinSegments against the model
(tests/runs_model.py), bit for bit, in one launch over segments of every length at which the kernels take another path and every
kind of content, at odd byte offsets, with sentinel bytes around every output; the join of streams that do not fit each other
stays inside its segment and gives what the model's tolerant join gives; bad arguments are refused with nothing written."""
import numpy as np
import pytest

import runs_model as R

pytestmark = pytest.mark.gpu

ILLEGAL = 2
LENGTHS = (1, 2, 255, 256, 257, 511, 1000, 4096, 70001)
CONTENTS = ("zeros", "nonzero", "run256", "run300", "to_end", "alternating", "random97")
SENTINEL = 0xEE


def _content(kind, n, rng):
    x = rng.integers(1, 256, n).astype(np.uint8)
    if kind == "zeros":
        x[:] = 0
    elif kind == "run256":                                      # a run of exactly 256 on a tile (what the segment holds of it)
        t = 256 if n > 512 else 0
        x[t:t + 256] = 0
    elif kind == "run300":                                      # a run of 300 across a tile edge
        x[100:400] = 0
    elif kind == "to_end":
        x[max(0, n - 77):] = 0
    elif kind == "alternating":
        x[0::2] = 0
    elif kind == "random97":
        x[rng.random(n) < 0.97] = 0
    return x


def _layout():
    """[(offset, segment)] at odd offsets with gaps, and the buffer size"""
    rng = np.random.default_rng(77)
    segs, pos = [], 1
    for n in LENGTHS:
        for kind in CONTENTS:
            segs.append((pos, _content(kind, n, rng)))
            pos += n + 37
            pos |= 1
    return segs, pos + 64


def _gpu(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint8, copy=True)).cuda()


@pytest.fixture(scope="module")
def launch(glc, cuda):
    """one split and one join of every segment; everything the tests compare, on the host"""
    import torch
    segs, size = _layout()
    x = np.full(size, SENTINEL, np.uint8)
    for off, s in segs:
        x[off:off + s.size] = s
    offs, lens = [o for o, _ in segs], [s.size for _, s in segs]
    d_x = _gpu(x)
    d_a = torch.full((size,), SENTINEL, dtype=torch.uint8, device=cuda)
    d_b = torch.full((size,), SENTINEL, dtype=torch.uint8, device=cuda)
    alen, blen = glc.zerorun_split_segments(d_x, d_a, d_b, offs, lens)
    d_out = torch.full((size,), SENTINEL, dtype=torch.uint8, device=cuda)
    glc.zerorun_join_segments(d_a, d_b, d_out, offs, alen, blen, lens)
    return dict(segs=segs, size=size, x=x, a=d_a.cpu().numpy(), b=d_b.cpu().numpy(), alen=alen.cpu().numpy(), blen=blen.cpu().numpy(),
                out=d_out.cpu().numpy(), d_a=d_a, d_b=d_b, offs=offs, lens=lens)


def test_split_equals_the_model_and_touches_nothing_else(launch):
    want_a = np.full(launch["size"], SENTINEL, np.uint8)
    want_b = np.full(launch["size"], SENTINEL, np.uint8)
    for i, (off, s) in enumerate(launch["segs"]):
        A, B = R.split(s)
        assert (int(launch["alen"][i]), int(launch["blen"][i])) == (A.size, B.size), (i, s.size)
        want_a[off:off + A.size] = A
        want_b[off:off + B.size] = B
    assert np.array_equal(launch["a"], want_a)
    assert np.array_equal(launch["b"], want_b)


def test_join_inverts_the_split_and_touches_nothing_else(launch):
    assert np.array_equal(launch["out"], launch["x"])


def test_join_of_streams_that_do_not_fit_stays_inside_the_segment(glc, cuda, launch):
    """too few B bytes (a zero beyond them is a run of one; the output's end is zeros) and a B that overruns n (nothing is written
    past the segment): well-defined, and what the model's join gives"""
    import torch
    segs, size = launch["segs"], launch["size"]
    rng = np.random.default_rng(5)
    a, b = launch["a"].copy(), launch["b"].copy()
    alen, blen = launch["alen"].copy(), launch["blen"].copy()
    for i, (off, s) in enumerate(segs):
        if i % 2:
            blen[i] //= 2                                       # too few
        else:
            b[off:off + int(blen[i])] = rng.integers(200, 256, int(blen[i]))      # overruns
    d_out = torch.full((size,), SENTINEL, dtype=torch.uint8, device=cuda)
    glc.zerorun_join_segments(_gpu(a), _gpu(b), d_out, launch["offs"], alen, blen, launch["lens"])
    want = np.full(size, SENTINEL, np.uint8)
    for i, (off, s) in enumerate(segs):
        want[off:off + s.size] = R.join(a[off:off + int(alen[i])], b[off:off + int(blen[i])], s.size)
    assert np.array_equal(d_out.cpu().numpy(), want)
    # lengths beyond maxLen are clamped to it: A and B are read no further, the segment is written no further
    d_out = torch.full((size,), SENTINEL, dtype=torch.uint8, device=cuda)
    off, s = segs[-1]
    glc.zerorun_join_segments(_gpu(a), _gpu(b), d_out, [off], [1 << 40], [1 << 40], [1 << 40], max_len=1000)
    want = np.full(size, SENTINEL, np.uint8)
    want[off:off + 1000] = R.join(a[off:off + 1000], b[off:off + 1000], 1000)
    assert np.array_equal(d_out.cpu().numpy(), want)


def test_bad_arguments_are_refused_with_nothing_written(glc, cuda):
    import torch
    L = glc._ct()
    x = _gpu(np.zeros(4096, np.uint8))
    a = torch.full((4096,), SENTINEL, dtype=torch.uint8, device=cuda)
    b = torch.full((4096,), SENTINEL, dtype=torch.uint8, device=cuda)
    off = torch.zeros(1, dtype=torch.int64, device=cuda)
    ln = torch.full((1,), 4096, dtype=torch.int64, device=cuda)
    la = torch.full((1,), 123, dtype=torch.int64, device=cuda)
    lb = torch.full((1,), 123, dtype=torch.int64, device=cuda)
    p = lambda t: t.data_ptr()
    bad_split = [(None, p(off), p(ln), 1, 4096, p(a), p(b), p(la), p(lb)), (p(x), p(off), p(ln), 1, 4096, p(a), p(a), p(la), p(lb)),
                 (p(x), p(off), p(ln), 1, 4096, p(x), p(b), p(la), p(lb)), (p(x), p(off), p(ln), 1, (1 << 20) + 1, p(a), p(b), p(la), p(lb)),
                 (p(x), p(off), p(ln), 1, 4096, p(a), p(b), None, p(lb))]
    for args in bad_split:
        assert L.glcZeroRunSplitSegments(*args, None) == ILLEGAL
    bad_join = [(p(a), p(b), p(off), p(la), p(lb), p(ln), 1, 4096, None), (p(a), p(b), p(off), p(la), p(lb), p(ln), 1, 4096, p(a)),
                (p(a), p(b), p(off), p(la), p(lb), p(ln), 1, (1 << 20) + 1, p(x)), (p(a), p(b), None, p(la), p(lb), p(ln), 1, 4096, p(x))]
    for args in bad_join:
        assert L.glcZeroRunJoinSegments(*args, None) == ILLEGAL
    torch.cuda.synchronize()
    assert bool((a == SENTINEL).all()) and bool((b == SENTINEL).all()) and bool((x == 0).all())
    assert int(la.item()) == 123 and int(lb.item()) == 123
