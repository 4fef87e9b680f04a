"""glcByteProbeSegments and glcBytePlanesSegments (csrc/byte_probe.hip) on the MI355X (-m gpu) against tests/filter_byte_model.py:
per segment the sixteen lag sums, every one of the 65537 stride sums, the two winners, the two histograms at those words and their
two costs, exactly -- every statistic is an integer.  Lengths 0, 7, 8, 1023, 1024, 1031 (the first byte that counts, the first
length with a candidate), 2047, 2048, 2049 (a run head), 16383, 16384, 16385 (a tile), 3 * 16384 + 5, 131072 + 8 (the first
length with Wmax = 65536) and 256 KiB (its expected values come from the golden fixture: the model needs ten seconds for them);
segment starts 3 and 0 bytes from a 16-byte boundary; greyscale images 17 and 721 wide, an RGB image 427 wide, 8-bit stereo,
zeros (the uniform shortcut; winners 1 and 17) and noise, several segments in one call; a batch with maxLen clamping, twice on the
same buffers; lag words 0, 1, 16, 17 and 0xFFFFFFFF and stride words 0, 1, 16, 17, 65536 and 65537; outputs pre-filled with 0xA5."""
import os

import numpy as np
import pytest

import byte_delta_inputs as BI
import filter_byte_inputs as BFI
import filter_byte_model as B

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filter_byte_probe_256k.npz")
CASES = [("noise", 0), ("noise", 7), ("noise", 8), ("grey17", 1023), ("grey17", 1024), ("noise", 1031), ("stereo8", 2047), ("zeros", 2048),
         ("rgb8", 2049), ("grey721", 16383), ("zeros", 16384), ("stereo8", 16385), ("rgb8", 3 * 16384 + 5), ("grey721", 131072 + 8)]


def content(kind, n):
    if kind == "grey17":
        return BI.grey8(n, 17)
    if kind == "grey721":
        return BI.grey8(n, 721)
    if kind == "rgb8":
        return BI.rgb8(n, 427)
    if kind == "stereo8":
        return BI.stereo8(n)
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    assert kind == "noise"
    return BI.noise(n)


def _reference(segs, words=None, probes=None):
    """(lag sums [n, 16], stride sums [n, 65537], winners [n, 2], rows [n, 2, 256], costs [n, 2]); the rows and costs at `words`
    where given"""
    A = [B.lag_sums(s) for s in segs] if probes is None else [p[0] for p in probes]
    S = [B.stride_sums(s) for s in segs] if probes is None else [p[1] for p in probes]
    W = [B.winners(a, s) for a, s in zip(A, S)]
    use = [w if words is None else words[i] for i, w in enumerate(W)]
    rows = [B.byte_planes(s, u) for s, u in zip(segs, use)]
    return (np.asarray(A, np.int64).reshape(len(segs), 16), np.stack(S).astype(np.uint32), np.asarray(W, np.int64).reshape(len(segs), 2),
            np.stack(rows), np.asarray([B.byte_costs(s, r, u) for s, r, u in zip(segs, rows, use)], np.int64))


def _place(segs, shifts):
    """the segments in one buffer, segment i shifts[i] bytes behind a 16-byte boundary"""
    off, pos = [], 0
    for s, sh in zip(segs, shifts):
        pos = (pos + 15) // 16 * 16 + int(sh)
        off.append(pos)
        pos += s.size
    buf = np.full(pos + 64, 0xEE, np.uint8)
    for o, s in zip(off, segs):
        buf[o:o + s.size] = s
    return buf, off


def _gpu(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True)).cuda()


def _prefilled(cuda, n):
    import torch

    def fill(shape, dtype):
        nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=cuda).view(dtype).reshape(shape)

    return (fill((n, 16), torch.int64), fill((n, B.SUM_ROW), torch.int32), fill((n, 2), torch.int32), fill((n, 2, 256), torch.int32),
            fill((n, 2), torch.int64))


def _both(glc, cuda, d, off, lengths, max_len=None, words=None, out=None):
    """the two probes into pre-filled outputs, the second at the first's winners unless `words` (a device tensor) is given"""
    lag_sums, sums, win, planes, costs = _prefilled(cuda, len(lengths)) if out is None else out
    assert planes.data_ptr() % 16 == 0
    a, s, w = glc.byte_probe_segments(d, off, lengths, max_len=max_len, lag_sums=lag_sums, stride_sums=sums, winners=win)
    p, c = glc.byte_planes_segments(d, off, lengths, w if words is None else words, max_len=max_len, planes=planes, costs=costs)
    return a.cpu().numpy(), s.cpu().numpy().view(np.uint32), w.cpu().numpy(), p.cpu().numpy().view(np.uint32), c.cpu().numpy()


def _same(got, want):
    for g, w, name in zip(got, want, ("lag sums", "stride sums", "winners", "planes", "costs")):
        assert g.shape == w.shape and np.array_equal(g, w), name      # (every word of every row)


@pytest.fixture(scope="module")
def matrix():
    segs = [content(kind, n) for kind, n in CASES]
    want = _reference(segs)
    win = {c: want[2][i].tolist() for i, c in enumerate(CASES)}
    assert win[("noise", 0)] == [1, 0] and win[("grey17", 1023)][1] == 0 and win[("grey17", 1024)][1] >= 17 and win[("noise", 1031)][1] >= 17
    assert win[("zeros", 2048)] == [1, 17] and win[("zeros", 16384)] == [1, 17]
    assert win[("grey721", 131072 + 8)] == [1, 721] and win[("rgb8", 3 * 16384 + 5)] == [3, 1281] and win[("stereo8", 16385)][0] == 2
    assert (want[4][CASES.index(("grey17", 1023))] == B.NO_COST).all() and (want[4][CASES.index(("grey17", 1024))] < B.NO_COST).all()
    assert want[1][CASES.index(("grey721", 131072 + 8)), 65536] != B.NO_SUM and want[1][CASES.index(("rgb8", 3 * 16384 + 5)), 24579] == B.NO_SUM
    return segs, want


@pytest.mark.parametrize("shift", [3, 0])
def test_probes_equal_the_model(glc, cuda, matrix, shift):
    segs, want = matrix
    buf, off = _place(segs, [shift] * len(segs))
    d = _gpu(buf)
    assert d.data_ptr() % 16 == 0
    _same(_both(glc, cuda, d, off, [s.size for s in segs]), want)
    assert bytes(d.cpu().numpy()) == buf.tobytes()                # (the input is only read)


def test_256_kib_against_the_golden_probe(glc, cuda):
    """256 KiB of the RGB image 427 wide: Wmax = 65536 and every chunk of strides; sums, winners, rows and costs are the golden
    fixture's, which tests/golden/make_filter_byte_v16_gold.py took from the model"""
    kind, width, n = BFI.PROBE_BIG
    seg = BFI.frame_bytes(kind, width, n)
    g = np.load(GOLD)
    want = (g["lag_sums"].reshape(1, 16), g["stride_sums"].reshape(1, B.SUM_ROW).astype(np.uint32), g["winners"].reshape(1, 2),
            g["rows"].reshape(1, 2, 256), g["costs"].reshape(1, 2))
    assert want[2].tolist() == [[3, 1281]] and want[1][0, 16] == B.NO_SUM and want[1][0, 17] != B.NO_SUM and want[1][0, 65536] != B.NO_SUM
    assert np.array_equal(want[3], B.byte_planes(seg, (3, 1281))[None]) and want[0][0].tolist() == B.lag_sums(seg)
    buf, off = _place([seg], [3])
    _same(_both(glc, cuda, _gpu(buf), off, [n]), want)


def test_mixed_batch_with_clamping_twice_on_the_same_buffers(glc, cuda):
    lengths = [70001, 81960, 9000, 9, 4104]                        # the first two are above maxLen
    max_len = 65536 + 4099                                         # not a multiple of 8
    segs = [content(k, n) for k, n in zip(("grey721", "rgb8", "noise", "stereo8", "grey17"), lengths)]
    buf, off = _place(segs, (5, 0, 9, 2, 8))
    want = _reference([s[:max_len] for s in segs])
    d = _gpu(buf)
    out = _prefilled(cuda, len(segs))
    for _ in range(2):
        _same(_both(glc, cuda, d, off, lengths, max_len=max_len, out=out), want)


@pytest.mark.parametrize("words", [(0, 0), (1, 1), (16, 16), (17, 17), (-1, 65536), (3, 65537), (2, 1281)])
def test_planes_at_words_that_are_not_the_winners(glc, cuda, words):
    """a lag word is used as ((v - 1) & 15) + 1; a stride word outside 17 .. 65536 names no stride: a zero row, the cost 2^56, and
    the word is never a distance"""
    import torch
    lengths = [49157, 4104, 24, 1031, 16384]
    segs = [content(k, n) for k, n in zip(("rgb8", "grey17", "noise", "stereo8", "zeros"), lengths)]
    buf, off = _place(segs, (3, 0, 8, 1, 3))
    assert [B.lag_clamp(v) for v in (0, 1, 16, 17, -1)] == [16, 1, 16, 1, 15]
    assert [B.stride_word(v) for v in (0, 1, 16, 17, 65536, 65537, -1)] == [0, 0, 0, 17, 65536, 0, 0]
    want = _reference(segs, words=[words] * len(segs), probes=[([0] * 16, np.full(B.SUM_ROW, B.NO_SUM, np.uint32))] * len(segs))
    d_w = torch.tensor([words] * len(segs), dtype=torch.int32, device=cuda)
    got = _both(glc, cuda, _gpu(buf), off, lengths, words=d_w)
    assert np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])
    assert (got[4][2] == B.NO_COST).all() and not got[3][2].any()          # 24 bytes: no candidate
    if not B.stride_word(words[1]):
        assert (got[4][:, 1] == B.NO_COST).all() and not got[3][:, 1].any() and (got[4][[0, 1, 3, 4], 0] < B.NO_COST).all()


def test_nothing_to_do_and_refusals_write_nothing(glc, cuda):
    import torch
    d = _gpu(np.arange(4096, dtype=np.uint8))
    lag_sums, sums, win, planes, costs = _prefilled(cuda, 2)
    keep = [t.clone() for t in (lag_sums, sums, win, planes, costs)]
    a, s, w = glc.byte_probe_segments(d, [], [], max_len=64, lag_sums=lag_sums, stride_sums=sums, winners=win)
    p, c = glc.byte_planes_segments(d, [], [], win, max_len=64, planes=planes, costs=costs)
    assert a.numel() == 0 and s.numel() == 0 and w.numel() == 0 and p.numel() == 0 and c.numel() == 0
    off = torch.zeros(1, dtype=torch.int64, device=cuda)
    ln = torch.full((1,), 4096, dtype=torch.int64, device=cuda)
    L = glc._ct()
    ILLEGAL = glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION
    good = [d.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, 4096, lag_sums.data_ptr(), sums.data_ptr(), win.data_ptr()]
    for i, v in [(i, None) for i in (0, 1, 2, 5, 6, 7)] + [(3, (1 << 22) + 1), (4, (1 << 31) + 1), (5, lag_sums.data_ptr() + 4), (6, sums.data_ptr() + 2),
                                                           (7, win.data_ptr() + 2), (6, lag_sums.data_ptr()), (7, sums.data_ptr()), (7, lag_sums.data_ptr())]:
        assert L.glcByteProbeSegments(*(good[:i] + [v] + good[i + 1:]), None) == ILLEGAL
    good = [d.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, 4096, win.data_ptr(), planes.data_ptr(), costs.data_ptr()]
    for i, v in [(i, None) for i in (0, 1, 2, 5, 6, 7)] + [(3, (1 << 22) + 1), (4, (1 << 31) + 1), (6, planes.data_ptr() + 8), (7, costs.data_ptr() + 4),
                                                           (7, planes.data_ptr()), (5, planes.data_ptr()), (5, costs.data_ptr())]:
        assert L.glcBytePlanesSegments(*(good[:i] + [v] + good[i + 1:]), None) == ILLEGAL
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip((lag_sums, sums, win, planes, costs), keep))
    x = np.arange(4096, dtype=np.uint8)
    want = _reference([x])
    _same(_both(glc, cuda, d, [0], [4096], out=(lag_sums, sums, win, planes, costs)), want)      # and then it does work
    assert all(torch.equal(x[1], y[1]) for x, y in zip((lag_sums, sums, win, planes, costs), keep))
