"""glcBigramProbeSegments (csrc/choose.hip) on the MI355X (-m gpu) against the integers of tests/choose_model.py: per segment
{S2, SR, SC, M}, equal in every word.  Lengths around nothing, one position, a lane's 16 bytes, a wave's step (1 KiB), 2^16 and
2^20; segment starts off a 16-byte boundary; a batch with maxLen clipping one segment; one byte value at 2^20 (one cell holds
2^20 - 2, S2 near 2^40) and at 65538 (a cell of exactly 65536: the edge of a 16-bit counter); contexts 127 and 128 only (the seam
between the two half-tables); text and noise at 8192; rows pre-filled with garbage; the refusals, with nothing written."""
import numpy as np
import pytest

import choose_inputs as CI
import choose_model as CM

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 3, 63, 64, 65, 4099, 65537, 65538, 1 << 20)


def _gpu(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True)).cuda()


def _place(segs, shifts):
    """the segments in one buffer, segment i `shifts[i]` bytes behind a 16-byte boundary"""
    off, pos = [], 0
    for s, sh in zip(segs, shifts):
        pos = (pos + 15) // 16 * 16 + int(sh)
        off.append(pos)
        pos += s.size
    buf = np.full(pos + 64, 0xEE, np.uint8)
    for o, s in zip(off, segs):
        buf[o:o + s.size] = s
    return buf, off


def _want(segs):
    return np.array([CM.stats(s) for s in segs], dtype=np.int64).reshape(len(segs), 4)


def _probe(glc, cuda, segs, shifts, lengths=None, max_len=None):
    import torch
    buf, off = _place(segs, shifts)
    d = _gpu(buf)
    assert d.data_ptr() % 16 == 0
    garbage = torch.full((len(segs), 4), -0x2152411021524111, dtype=torch.int64, device=cuda)
    got = glc.bigram_probe_segments(d, off, lengths or [s.size for s in segs], max_len=max_len, stats=garbage)
    assert bytes(d.cpu().numpy()) == buf.tobytes()                # (the input is only read)
    return got.cpu().numpy()


def seam_segment(n, rng):
    """bytes whose every context (31 x[p-2] + x[p-1]) & 255 is 127 or 128: a walk in which each byte is one of the two that make
    such a context with the byte before it"""
    pick = rng.integers(0, 2, n)
    x = np.zeros(n, np.int64)
    x[0] = 3
    for i in range(1, n):
        x[i] = (127 + pick[i] - 31 * x[i - 1]) & 255
    assert set(((31 * x[:-2] + x[1:-1]) & 255).tolist()) == {127, 128}
    return x.astype(np.uint8)


_CASE = []


def _case():
    """(segments, their rows by the model), made once for all placements"""
    if not _CASE:
        rng = np.random.default_rng(60)
        segs = []
        for n in LENGTHS:
            kind = ("text", "noise", "zeros90", "logs")[len(segs) % 4]
            segs.append(CI.block(kind, n, 100 + n % 97) if n else np.zeros(0, np.uint8))
        segs += [CI.block("text", 8192, 5), CI.block("noise", 8192, 6), seam_segment(4099, rng), seam_segment(65537, rng)]
        _CASE.extend([segs, _want(segs)])
    return _CASE


@pytest.mark.parametrize("shift", [0, 1, 3, 15])
def test_probe_equals_the_model(glc, cuda, shift):
    segs, want = _case()
    assert want[:4].tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1]]
    got = _probe(glc, cuda, segs, [shift] * len(segs))
    assert np.array_equal(got, want), [(s.size, g.tolist(), w.tolist()) for s, g, w in zip(segs, got, want) if not np.array_equal(g, w)]


def test_one_byte_value_fills_one_cell(glc, cuda):
    """2^20 equal bytes: one cell holds 2^20 - 2 and S2 = SR = SC = (2^20 - 2)(2^20 - 3); 65538: a cell of exactly 2^16; and the
    same with one other byte in the middle, so that three keys differ from the rest"""
    segs = [np.full(1 << 20, 0, np.uint8), np.full(65538, 0xFF, np.uint8), np.full(1 << 20, 0x41, np.uint8), np.full(65538, 7, np.uint8)]
    segs[2][500001] = 0x42
    segs[3][65537] = 9
    want = _want(segs)
    m = (1 << 20) - 2
    assert want[0].tolist() == [m * (m - 1)] * 3 + [m] and want[1].tolist() == [65536 * 65535] * 3 + [65536]
    got = _probe(glc, cuda, segs, [0, 5, 9, 0])
    assert np.array_equal(got, want)


def test_mixed_batch_with_clipping(glc, cuda):
    rng = np.random.default_rng(78)
    lengths = [70000, 1234, 50001]
    max_len = 50000
    segs = [CI.block(k, n, 9) for k, n in zip(("logs", "zipf", "text"), lengths)]
    want = _want([s[:max_len] for s in segs])
    got = _probe(glc, cuda, segs, rng.integers(0, 16, 3), lengths=lengths, max_len=max_len)
    assert np.array_equal(got, want) and got[:, 3].tolist() == [max_len - 2, 1232, max_len - 2]
    assert [CM.is_bwt(min(n, max_len), tuple(int(v) for v in g)) for n, g in zip(lengths, got)] == [True, False, True]


def test_nothing_to_do_and_refusals_write_nothing(glc, cuda):
    import torch
    d = _gpu(np.arange(4096, dtype=np.uint8))
    rows = torch.full((2, 4), 123, dtype=torch.int64, device=cuda)
    assert glc.bigram_probe_segments(d, [], [], max_len=64, stats=rows).numel() == 0
    off = torch.zeros(1, dtype=torch.int64, device=cuda)
    ln = torch.full((1,), 4096, dtype=torch.int64, device=cuda)
    L = glc._ct()
    for args in ((d.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, (1 << 20) + 1, rows.data_ptr()),
                 (d.data_ptr(), off.data_ptr(), ln.data_ptr(), (1 << 22) + 1, 4096, rows.data_ptr()),
                 (d.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, 4096, rows.data_ptr() + 4),
                 (d.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, 4096, None),
                 (None, off.data_ptr(), ln.data_ptr(), 1, 4096, rows.data_ptr()),
                 (d.data_ptr(), None, ln.data_ptr(), 1, 4096, rows.data_ptr()),
                 (d.data_ptr(), off.data_ptr(), None, 1, 4096, rows.data_ptr())):
        assert L.glcBigramProbeSegments(*args, None) == glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION
    torch.cuda.synchronize()
    assert bool((rows == 123).all())
    got = glc.bigram_probe_segments(d, [0], [4096], stats=rows)               # and then it does work
    assert got.cpu().numpy().tolist() == [list(CM.stats(np.arange(4096, dtype=np.uint8)))] and bool((rows[1] == 123).all())
