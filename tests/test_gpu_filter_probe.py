"""glcFilterProbeSegments (csrc/filter_probe.hip) on the MI355X (-m gpu) against tests/filter_auto_model.py: per segment the 22
histograms (A_0..7 and the delta planes D_2, D_4, D_8 of the first L - L % 8 bytes) and the seven candidates' costs, exactly.
Lengths around 8 bytes, a lane's granule, a wave's pass (1 KiB), the delta restarts (4, 8 and 16 KiB), a workgroup's span (64 KiB,
and 2 MiB under a large maxLen); segment starts 0, 1, 3 and 8 bytes from a 16-byte boundary; contents that take the uniform
shortcut of every histogram group and contents that never do; a mixed batch with maxLen clamping; rows pre-filled with garbage."""
import numpy as np
import pytest

import filter_auto_model as F
import series_datagen
import typed_datagen

pytestmark = pytest.mark.gpu

TILE, SPAN = 16384, 65536
LENGTHS = (0, 1, 7, 8, 15, 4095, 4096, 4097, 16383, 16384, 16385, TILE - 8, TILE + 8, 2 * TILE + 13, SPAN - 8, SPAN + 8, 2 * SPAN + 13)
CONTENTS = ("zeros", "constant", "step32", "ts64", "float32", "noise")


def content(kind, n, rng):
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    if kind == "constant":
        return np.full(n, 0xA5, np.uint8)
    if kind == "step32":                                           # a regular-step uint32 series: every delta plane is one byte
        return (np.uint32(0x01020304) + np.uint32(0x00030201) * np.arange((n + 3) // 4, dtype=np.uint32)).astype("<u4").view(np.uint8)[:n].copy()
    if kind == "ts64":
        return np.ascontiguousarray(series_datagen.series_bytes("ts64", n + 8))[:n].copy()
    if kind == "float32":
        return np.frombuffer(typed_datagen.typed_bytes("float32", n + 4), np.uint8)[:n].copy()
    assert kind == "noise"
    return rng.integers(0, 256, n, dtype=np.uint8)


def _reference(segs):
    rows = [F.probe(s) for s in segs]
    return np.stack(rows), np.asarray([F.costs(r) for r in rows], np.int64)


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


@pytest.fixture(scope="module")
def matrix():
    rng = np.random.default_rng(91)
    segs = [content(kind, n, rng) for kind in CONTENTS for n in LENGTHS]
    want_rows, want_costs = _reference(segs)
    assert int(want_rows.sum()) > 0 and len({F.pick(list(c)) for c in want_costs}) >= 3
    return segs, want_rows, want_costs


@pytest.mark.parametrize("shift", [0, 1, 3, 8])
def test_probe_equals_the_model(glc, cuda, matrix, shift):
    import torch
    segs, want_rows, want_costs = matrix
    buf, off = _place(segs, [shift] * len(segs))
    d = _gpu(buf)
    assert d.data_ptr() % 16 == 0
    planes = torch.full((len(segs), 22, 256), -0x21524111, dtype=torch.int32, device=cuda)
    costs = torch.full((len(segs), 7), -0x0123456789ABCDEF, dtype=torch.int64, device=cuda)
    got_rows, got_costs = glc.filter_probe_segments(d, off, [s.size for s in segs], planes=planes, costs=costs)
    assert np.array_equal(got_rows.cpu().numpy().view(np.uint32), want_rows)
    assert np.array_equal(got_costs.cpu().numpy(), want_costs)
    assert bytes(d.cpu().numpy()) == buf.tobytes()                # (the input is only read)


def test_mixed_batch_with_clamping(glc, cuda):
    rng = np.random.default_rng(92)
    lengths = [70001, 3 * SPAN + 24, 40000]                       # the first two are above maxLen
    max_len = 2 * SPAN + 13
    segs = [content(k, n, rng) for k, n in zip(("ts64", "step32", "noise"), lengths)]
    buf, off = _place(segs, (5, 0, 9))
    want_rows, want_costs = _reference([s[:max_len] for s in segs])
    got_rows, got_costs = glc.filter_probe_segments(_gpu(buf), off, lengths, max_len=max_len)
    assert np.array_equal(got_rows.cpu().numpy().view(np.uint32), want_rows)
    assert np.array_equal(got_costs.cpu().numpy(), want_costs)
    assert int(got_rows[:, :8].sum(dim=(1, 2)).max()) == max_len - max_len % 8


def test_spans_of_a_large_max_len(glc, cuda):
    """under maxLen = 2^31 a workgroup's span is 2 MiB: segments of a span - 8, a span + 8 and two spans + 13, two of them
    misaligned, one of uniform delta planes"""
    rng = np.random.default_rng(93)
    span = 1 << 21
    lengths = [span - 8, span + 8, 2 * span + 13]
    segs = [content(k, n, rng) for k, n in zip(("ts64", "noise", "step32"), lengths)]
    buf, off = _place(segs, (0, 3, 8))
    want_rows, want_costs = _reference(segs)
    got_rows, got_costs = glc.filter_probe_segments(_gpu(buf), off, lengths, max_len=glc.FILTER_PROBE_MAX_LEN)
    assert np.array_equal(got_rows.cpu().numpy().view(np.uint32), want_rows)
    assert np.array_equal(got_costs.cpu().numpy(), want_costs)


def test_nothing_to_do_and_refusals_write_nothing(glc, cuda):
    import torch
    d = _gpu(np.arange(4096, dtype=np.uint8))
    planes = torch.full((2, 22, 256), 123, dtype=torch.int32, device=cuda)
    costs = torch.full((2, 7), 456, dtype=torch.int64, device=cuda)
    p, c = glc.filter_probe_segments(d, [], [], max_len=64, planes=planes, costs=costs)
    assert p.numel() == 0 and c.numel() == 0
    off = torch.zeros(1, dtype=torch.int64, device=cuda)
    ln = torch.full((1,), 4096, dtype=torch.int64, device=cuda)
    L = glc._ct()
    good = [d.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, 4096, planes.data_ptr(), costs.data_ptr()]
    bad = []
    for i in (0, 1, 2, 5, 6):                                      # each pointer null in turn
        bad.append(good[:i] + [None] + good[i + 1:])
    for i, v in ((3, (1 << 22) + 1), (4, (1 << 31) + 1), (5, planes.data_ptr() + 4), (6, costs.data_ptr() + 4), (6, planes.data_ptr())):
        bad.append(good[:i] + [v] + good[i + 1:])
    for args in bad:
        assert L.glcFilterProbeSegments(*args, None) == glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION
    torch.cuda.synchronize()
    assert bool((planes == 123).all()) and bool((costs == 456).all())
    p, c = glc.filter_probe_segments(d, [0], [4096], planes=planes, costs=costs)      # and then it does work
    assert int(p[0, :8].sum()) == 4096 and bool((planes[1] == 123).all()) and bool((costs[1] == 456).all())
    assert c.cpu().numpy().tolist() == [F.rule(np.arange(4096, dtype=np.uint8))[1]]
