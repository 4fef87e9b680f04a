"""glcLagProbeSegments and glcLagPlanesSegments (csrc/lag_probe.hip) on the MI355X (-m gpu) against tests/filter_lag_model.py: per
segment the 48 sums S[e][l], the three winners, the 14 histograms at those lags and their three costs, exactly.
Lengths around 8 bytes, a granule, the delta restarts (4, 8 and 16 KiB), a tile (16 KiB) and a workgroup's span (64 KiB), the last
not a multiple of 8, and 2 MiB under a large maxLen; segment starts 0, 1, 3 and 8 bytes from a 16-byte boundary (the 16-byte and the byte path); interleaved
channels, noise, contents that take the uniform shortcut of every histogram group, and elements whose folded difference has every
bit set; a mixed batch with maxLen clamping; lags that are not the winners, a word of 0 and of 17 among them; outputs pre-filled
with 0xA5; the same call twice on the same buffers."""
import numpy as np
import pytest

import filter_lag_model as FL
import lag_inputs

pytestmark = pytest.mark.gpu

LENGTHS = (0, 7, 8, 9, 24, 4095, 4096, 4104, 16384, 16392, 32776, 65536, 81960, 200000)
CONTENTS = ("adc16x8", "xyz32", "noise", "zeros", "constant", "step64", "ones", "sign64")


def content(kind, n, rng):
    if kind in lag_inputs.KINDS:
        return lag_inputs.lag_bytes(kind, n)
    if kind == "noise":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    if kind == "constant":
        return np.full(n, 0xA5, np.uint8)
    if kind == "step64":                                           # a regular-step int64 series: every plane of E_8 at lag 1 is one byte
        return (np.uint64(0x0102030405060708) + np.uint64(0x0000000300020001) * np.arange((n + 7) // 8, dtype=np.uint64)).astype("<u8").view(np.uint8)[:n].copy()
    if kind == "ones":                                             # every byte 0xFF: the run heads are all-ones elements
        return np.full(n, 0xFF, np.uint8)
    assert kind == "sign64"                                        # 0 and 2^63 in turn: an odd lag's folded difference is all ones
    return (np.uint64(1 << 63) * (np.arange((n + 7) // 8, dtype=np.uint64) & np.uint64(1))).astype("<u8").view(np.uint8)[:n].copy()


def _reference(segs, lags=None):
    """(sums [n, 48], winners [n, 3], rows [n, 14, 256], costs [n, 3]); the rows and costs at `lags` where given"""
    S = [FL.sums(s) for s in segs]
    W = [FL.winners(x) for x in S]
    rows = [FL.lag_planes(s, w if lags is None else lags[i]) for i, (s, w) in enumerate(zip(segs, W))]
    return (np.asarray(S, np.int64).reshape(len(segs), FL.SUMS), np.asarray(W, np.int64).reshape(len(segs), 3),
            np.stack(rows), np.asarray([FL.lag_costs(r) for r in rows], np.int64))


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

    return (fill((n, FL.SUMS), torch.int64), fill((n, 3), torch.int32), fill((n, FL.ROWS, 256), torch.int32), fill((n, 3), torch.int64))


def _both(glc, cuda, d, off, lengths, max_len=None, lags=None):
    """the two probes into pre-filled outputs, the second at the first's winners unless `lags` (a device tensor) is given"""
    sums, win, planes, costs = _prefilled(cuda, len(lengths))
    assert int(sums[0, 0]) == int(np.int64(-0x5A5A5A5A5A5A5A5B)) and planes.data_ptr() % 16 == 0
    s, w = glc.lag_probe_segments(d, off, lengths, max_len=max_len, sums=sums, lags=win)
    p, c = glc.lag_planes_segments(d, off, lengths, w if lags is None else lags, max_len=max_len, planes=planes, costs=costs)
    return s.cpu().numpy(), w.cpu().numpy(), p.cpu().numpy().view(np.uint32), c.cpu().numpy()


@pytest.fixture(scope="module")
def matrix():
    rng = np.random.default_rng(131)
    segs = [content(kind, n, rng) for kind in CONTENTS for n in LENGTHS]
    want = _reference(segs)
    big = {k: want[1][i * len(LENGTHS) + LENGTHS.index(65536)].tolist() for i, k in enumerate(CONTENTS)}
    assert big["adc16x8"][0] == 8 and big["xyz32"][1] == 3 and big["zeros"] == [1, 1, 1] and big["step64"][2] == 1
    assert int(want[0].max()) > 1 << 20 and big["sign64"][2] == 2              # (sign64 at lag 1: 64 bits an element)
    return segs, want


@pytest.mark.parametrize("shift", [0, 1, 3, 8])
def test_probes_equal_the_model(glc, cuda, matrix, shift):
    segs, want = matrix
    buf, off = _place(segs, [shift] * len(segs))
    d = _gpu(buf)
    assert d.data_ptr() % 16 == 0
    got = _both(glc, cuda, d, off, [s.size for s in segs])
    for g, w, name in zip(got, want, ("sums", "winners", "planes", "costs")):
        assert np.array_equal(g, w), name
    assert bytes(d.cpu().numpy()) == buf.tobytes()                # (the input is only read)


def test_mixed_batch_with_clamping_twice_on_the_same_buffers(glc, cuda):
    import torch
    rng = np.random.default_rng(132)
    lengths = [70001, 81960, 40000, 9, 16392]                      # the first two are above maxLen
    max_len = 65536 + 4099                                         # not a multiple of 8
    segs = [content(k, n, rng) for k, n in zip(("adc16x8", "step64", "noise", "xyz32", "sign64"), lengths)]
    buf, off = _place(segs, (5, 0, 9, 2, 8))
    want = _reference([s[:max_len] for s in segs])
    d = _gpu(buf)
    sums, win, planes, costs = _prefilled(cuda, len(segs))
    for _ in range(2):
        s, w = glc.lag_probe_segments(d, off, lengths, max_len=max_len, sums=sums, lags=win)
        p, c = glc.lag_planes_segments(d, off, lengths, w, max_len=max_len, planes=planes, costs=costs)
        got = (s.cpu().numpy(), w.cpu().numpy(), p.cpu().numpy().view(np.uint32), c.cpu().numpy())
        for g, x, name in zip(got, want, ("sums", "winners", "planes", "costs")):
            assert np.array_equal(g, x), name
    assert int(p[0].sum()) == 3 * (max_len - max_len % 8)         # (every counted byte once per element size)
    assert torch.equal(w.cpu(), torch.as_tensor(want[1], dtype=torch.int32))


def test_spans_of_a_large_max_len(glc, cuda):
    """under maxLen = 2^31 a workgroup's span is 2 MiB, where a lane's share of a sum is largest: segments of a span - 8, a span + 8
    and two spans + 13, two of them misaligned, one whose folded differences at odd lags have all 64 bits set"""
    rng = np.random.default_rng(134)
    span = 1 << 21
    lengths = [span - 8, span + 8, 2 * span + 13]
    segs = [content(k, n, rng) for k, n in zip(("sign64", "noise", "adc16x8"), lengths)]
    buf, off = _place(segs, (0, 3, 8))
    want = _reference(segs)
    got = _both(glc, cuda, _gpu(buf), off, lengths, max_len=glc.FILTER_PROBE_MAX_LEN)
    for g, w, name in zip(got, want, ("sums", "winners", "planes", "costs")):
        assert np.array_equal(g, w), name


@pytest.mark.parametrize("lags", [(16, 7, 1), (1, 1, 1), (0, 17, 8)])
def test_planes_at_lags_that_are_not_the_winners(glc, cuda, lags):
    """a word of 0 is used as lag 16 and a word of 17 as lag 1: ((v - 1) & 15) + 1"""
    import torch
    rng = np.random.default_rng(133)
    lengths = [81960, 4104, 24, 200000]
    segs = [content(k, n, rng) for k, n in zip(("adc16x8", "xyz32", "noise", "step64"), lengths)]
    buf, off = _place(segs, (0, 3, 8, 1))
    assert (FL.clamp(0), FL.clamp(17), FL.clamp(16), FL.clamp(1)) == (16, 1, 16, 1)
    want = _reference(segs, lags=[lags] * len(segs))
    d_lags = torch.tensor([lags] * len(segs), dtype=torch.int32, device=cuda)
    got = _both(glc, cuda, _gpu(buf), off, lengths, lags=d_lags)
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])     # (the first probe is its own)


def test_nothing_to_do_and_refusals_write_nothing(glc, cuda):
    import torch
    d = _gpu(np.arange(4096, dtype=np.uint8))
    sums, win, planes, costs = _prefilled(cuda, 2)
    keep = [t.clone() for t in (sums, win, planes, costs)]
    s, w = glc.lag_probe_segments(d, [], [], max_len=64, sums=sums, lags=win)
    p, c = glc.lag_planes_segments(d, [], [], win, max_len=64, planes=planes, costs=costs)
    assert s.numel() == 0 and w.numel() == 0 and p.numel() == 0 and c.numel() == 0
    off = torch.zeros(1, dtype=torch.int64, device=cuda)
    ln = torch.full((1,), 4096, dtype=torch.int64, device=cuda)
    L = glc._ct()
    ILLEGAL = glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION
    good = [d.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, 4096, sums.data_ptr(), win.data_ptr()]
    for i, v in [(i, None) for i in (0, 1, 2, 5, 6)] + [(3, (1 << 22) + 1), (4, (1 << 31) + 1), (5, sums.data_ptr() + 4), (6, sums.data_ptr())]:
        assert L.glcLagProbeSegments(*(good[:i] + [v] + good[i + 1:]), None) == ILLEGAL
    good = [d.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, 4096, win.data_ptr(), planes.data_ptr(), costs.data_ptr()]
    for i, v in [(i, None) for i in (0, 1, 2, 5, 6, 7)] + [(3, (1 << 22) + 1), (4, (1 << 31) + 1), (6, planes.data_ptr() + 8), (7, costs.data_ptr() + 4),
                                                           (7, planes.data_ptr()), (5, planes.data_ptr()), (5, costs.data_ptr())]:
        assert L.glcLagPlanesSegments(*(good[:i] + [v] + good[i + 1:]), None) == ILLEGAL
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((sums, win, planes, costs), keep))
    x = np.arange(4096, dtype=np.uint8)
    s, w = glc.lag_probe_segments(d, [0], [4096], sums=sums, lags=win)             # and then it does work
    p, c = glc.lag_planes_segments(d, [0], [4096], w, planes=planes, costs=costs)
    S, W, rows, C = FL.probe(x)
    assert s.cpu().numpy().tolist() == [S] and w.cpu().numpy().tolist() == [list(W)] and c.cpu().numpy().tolist() == [C]
    assert np.array_equal(p.cpu().numpy()[0], rows)
    assert all(torch.equal(a[1], b[1]) for a, b in zip((sums, win, planes, costs), keep))
