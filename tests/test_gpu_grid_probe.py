"""glcGridProbeSegments and glcGridPlanesSegments (csrc/grid_probe.hip) on the MI355X (-m gpu) against tests/filter_grid_model.py:
per segment every one of the 3 * 65537 sums S_e[W], the three winners, the 14 histograms at those widths and their three costs,
exactly.  Lengths 0, 8, and for every element size 1023, 1024 elements and 1024 elements + 7 bytes (the first length with a
candidate); 64 KiB + 3; 256 KiB, where elem 2 reaches Wmax = 65536 and so the last chunk of widths while elem 4 and 8 stay below
(its expected sums come from the golden fixture: the model needs about ten seconds for them); segment starts 0, 1, 3 and 8 bytes
from a 16-byte boundary; gridded data, noise, zeros (winner 2), 64-bit elements whose differences exceed 2^32 and are negative; a
mixed batch with maxLen clamping, twice on the same buffers; widths that are not the winners, words of 0, 1, 65537 and 0xFFFFFFFF
among them; outputs pre-filled with 0xA5."""
import os

import numpy as np
import pytest

import filter_grid_model as Q
import grid_inputs

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "filter_grid_probe_256k.npz")
SMALL = (0, 8) + tuple(n for e in (2, 4, 8) for n in (1023 * e, 1024 * e, 1024 * e + 7))
CASES = [("noise", n) for n in SMALL] + [("img16", 65536 + 3), ("zeros", 16384), ("sign64", 16392), ("walk64", 24576), ("field32", 40000)]
BIG = ("walk32", 721, 1 << 18)                                     # kind, row width, bytes: the golden segment


def content(kind, n, rng):
    if kind == "img16":
        return grid_inputs.grid_bytes(kind, n, 300)
    if kind == "field32":
        return grid_inputs.grid_bytes(kind, n, 450)
    if kind == "noise":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    if kind == "sign64":                                           # 0 and 2^63 in turn: an odd width's folded difference is all ones
        return (np.uint64(1 << 63) * (np.arange((n + 7) // 8, dtype=np.uint64) & np.uint64(1))).astype("<u8").view(np.uint8)[:n].copy()
    assert kind == "walk64"                                        # a grid of int64 in rows of 96 whose steps exceed 2^32, both signs
    steps = rng.integers(-(1 << 40), 1 << 40, ((n + 7) // 8 // 96 + 1, 96), dtype=np.int64)
    return np.cumsum(steps, axis=0).astype("<i8").reshape(-1).view(np.uint8)[:n].copy()


def _reference(segs, widths=None, sums=None):
    """(sums [n, 3 * 65537], winners [n, 3], rows [n, 14, 256], costs [n, 3]); the rows and costs at `widths` where given"""
    S = [Q.sums(s) for s in segs] if sums is None else sums
    W = [Q.winners(x) for x in S]
    use = [w if widths is None else widths[i] for i, w in enumerate(W)]
    rows = [Q.grid_planes(s, u) for s, u in zip(segs, use)]
    return (np.stack(S).astype(np.uint32), np.asarray(W, np.int64).reshape(len(segs), 3), np.stack(rows),
            np.asarray([Q.grid_costs(r, u) for r, u in zip(rows, use)], np.int64))


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

    return (fill((n, Q.SUMS), torch.int32), fill((n, 3), torch.int32), fill((n, Q.ROWS, 256), torch.int32), fill((n, 3), torch.int64))


def _both(glc, cuda, d, off, lengths, max_len=None, widths=None, out=None):
    """the two probes into pre-filled outputs, the second at the first's winners unless `widths` (a device tensor) is given"""
    sums, win, planes, costs = _prefilled(cuda, len(lengths)) if out is None else out
    assert planes.data_ptr() % 16 == 0
    s, w = glc.grid_probe_segments(d, off, lengths, max_len=max_len, sums=sums, widths=win)
    p, c = glc.grid_planes_segments(d, off, lengths, w if widths is None else widths, max_len=max_len, planes=planes, costs=costs)
    return s.cpu().numpy().view(np.uint32), w.cpu().numpy(), p.cpu().numpy().view(np.uint32), c.cpu().numpy()


def _same(got, want):
    for g, w, name in zip(got, want, ("sums", "winners", "planes", "costs")):
        assert g.shape == w.shape and np.array_equal(g, w), name      # (every word of every row)


@pytest.fixture(scope="module")
def matrix():
    rng = np.random.default_rng(141)
    segs = [content(kind, n, rng) for kind, n in CASES]
    want = _reference(segs)
    win = {c: want[1][i].tolist() for i, c in enumerate(CASES)}
    assert win[("noise", 8)] == [0, 0, 0] and win[("noise", 2046)] == [0, 0, 0] and win[("zeros", 16384)] == [2, 2, 2]
    assert win[("noise", 2048)][0] >= 2 and win[("noise", 2048)][1:] == [0, 0] and win[("noise", 8184)][2] == 0 and win[("noise", 8192)][2] >= 2
    assert win[("walk64", 24576)][2] == 96 and win[("sign64", 16392)] == [8, 4, 2]
    assert (want[3][CASES.index(("noise", 8))] == Q.NO_COST).all()
    return segs, want


@pytest.mark.parametrize("shift", [0, 1, 3, 8])
def test_probes_equal_the_model(glc, cuda, matrix, shift):
    segs, want = matrix
    buf, off = _place(segs, [shift] * len(segs))
    d = _gpu(buf)
    assert d.data_ptr() % 16 == 0
    _same(_both(glc, cuda, d, off, [s.size for s in segs]), want)
    assert bytes(d.cpu().numpy()) == buf.tobytes()                # (the input is only read)


def test_the_last_chunk_of_widths(glc, cuda):
    """256 KiB: elem 2 has Wmax = 65536, elem 4 32768 and elem 8 16384.  The sums are the golden fixture's, which
    tests/golden/make_filter_grid_v14_gold.py took from the model; winners, rows and costs follow from them here."""
    kind, width, n = BIG
    seg = grid_inputs.grid_bytes(kind, n, width)
    gold = np.load(GOLD)["sums"]
    assert gold.shape == (Q.SUMS,) and gold[65536] != Q.NO_SUM and gold[Q.SUM_ROW + 32768] != Q.NO_SUM and gold[Q.SUM_ROW + 32769] == Q.NO_SUM
    want = _reference([seg], sums=[gold])
    for shift in (0, 2):
        buf, off = _place([seg], [shift])
        _same(_both(glc, cuda, _gpu(buf), off, [n]), want)


def test_mixed_batch_with_clamping_twice_on_the_same_buffers(glc, cuda):
    rng = np.random.default_rng(142)
    lengths = [70001, 81960, 9000, 9, 4104]                        # the first two are above maxLen
    max_len = 65536 + 4099                                         # not a multiple of 8 (test_gpu_lag_probe.py's cut)
    segs = [content(k, n, rng) for k, n in zip(("img16", "walk64", "noise", "field32", "sign64"), lengths)]
    buf, off = _place(segs, (5, 0, 9, 2, 8))
    want = _reference([s[:max_len] for s in segs])
    d = _gpu(buf)
    out = _prefilled(cuda, len(segs))
    for _ in range(2):
        _same(_both(glc, cuda, d, off, lengths, max_len=max_len, out=out), want)


@pytest.mark.parametrize("widths", [(300, 7, 96), (0, 1, 65537), (-1, 65536, 2), (2, 0x40000002, 1 << 16 | 1 << 20)])
def test_planes_at_widths_that_are_not_the_winners(glc, cuda, widths):
    """a width word outside 2 .. 65536 names no width: zero rows, the cost 2^56, and the word is never a distance"""
    import torch
    rng = np.random.default_rng(143)
    lengths = [65539, 4104, 24, 24576]
    segs = [content(k, n, rng) for k, n in zip(("img16", "field32", "noise", "walk64"), lengths)]
    buf, off = _place(segs, (0, 3, 8, 1))
    assert [Q.width_word(w) for w in (0, 1, 2, 65536, 65537, -1)] == [0, 0, 2, 65536, 0, 0]
    want = _reference(segs, widths=[widths] * len(segs))
    d_w = torch.tensor([widths] * len(segs), dtype=torch.int32, device=cuda)
    got = _both(glc, cuda, _gpu(buf), off, lengths, widths=d_w)
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    for k, w in enumerate(widths):
        if not Q.width_word(w):
            assert (got[3][:, k] == Q.NO_COST).all() and not got[2][:, Q.PLANE_ROW[2 << k]:Q.PLANE_ROW[2 << k] + (2 << k)].any()


def test_nothing_to_do_and_refusals_write_nothing(glc, cuda):
    import torch
    d = _gpu(np.arange(4096, dtype=np.uint8))
    sums, win, planes, costs = _prefilled(cuda, 2)
    keep = [t.clone() for t in (sums, win, planes, costs)]
    s, w = glc.grid_probe_segments(d, [], [], max_len=64, sums=sums, widths=win)
    p, c = glc.grid_planes_segments(d, [], [], win, max_len=64, planes=planes, costs=costs)
    assert s.numel() == 0 and w.numel() == 0 and p.numel() == 0 and c.numel() == 0
    off = torch.zeros(1, dtype=torch.int64, device=cuda)
    ln = torch.full((1,), 4096, dtype=torch.int64, device=cuda)
    L = glc._ct()
    ILLEGAL = glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION
    good = [d.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, 4096, sums.data_ptr(), win.data_ptr()]
    for i, v in [(i, None) for i in (0, 1, 2, 5, 6)] + [(3, (1 << 22) + 1), (4, (1 << 31) + 1), (5, sums.data_ptr() + 2), (6, sums.data_ptr())]:
        assert L.glcGridProbeSegments(*(good[:i] + [v] + good[i + 1:]), None) == ILLEGAL
    good = [d.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, 4096, win.data_ptr(), planes.data_ptr(), costs.data_ptr()]
    for i, v in [(i, None) for i in (0, 1, 2, 5, 6, 7)] + [(3, (1 << 22) + 1), (4, (1 << 31) + 1), (6, planes.data_ptr() + 8), (7, costs.data_ptr() + 4),
                                                           (7, planes.data_ptr()), (5, planes.data_ptr()), (5, costs.data_ptr())]:
        assert L.glcGridPlanesSegments(*(good[:i] + [v] + good[i + 1:]), None) == ILLEGAL
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((sums, win, planes, costs), keep))
    x = np.arange(4096, dtype=np.uint8)
    want = _reference([x])
    _same(_both(glc, cuda, d, [0], [4096], out=(sums, win, planes, costs)), want)      # and then it does work
    assert all(torch.equal(a[1], b[1]) for a, b in zip((sums, win, planes, costs), keep))
