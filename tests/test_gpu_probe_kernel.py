"""glcProbeSegments (csrc/auto.hip) on the MI355X (-m gpu) against numpy: per segment the byte counts and, per byte value, the
64-byte chunks -- cut from the segment's start, whatever its address -- made of that byte alone.  Lengths around a chunk, a
wave's pass (1 KiB) and a workgroup's tile (64 KiB) up to 2^20; segment starts at 0, 1, 3 and 15 bytes from a 16-byte boundary;
contents that take every path of the kernel; a mixed batch with maxLen clamping; rows pre-filled with garbage."""
import numpy as np
import pytest

import ans_inputs
import auto_model as U

pytestmark = pytest.mark.gpu

LENGTHS = (1, 63, 64, 65, 127, 4095, 16384 + 17, 70000, 1 << 20)
CONTENTS = ("constant", "noise", "scattered", "alternating", "last byte", "quarters", "short uniform", "short mixed")


def content(kind, n, rng):
    if kind in ("constant", "noise", "scattered"):
        return ans_inputs.segment(kind, n, rng)
    i = np.arange(n)
    c = i // 64
    if kind == "alternating":                                     # uniform chunks and mixed ones in turn
        return np.where(c % 2 == 0, 7, rng.integers(0, 256, n)).astype(np.uint8)
    if kind == "last byte":                                       # every third chunk uniform but for its last byte
        return np.where((c % 3 == 0) & (i % 64 == 63), 0x21, 0x20).astype(np.uint8)
    if kind == "quarters":                                        # each 16-byte quarter one byte; the quarters differ in two chunks of three
        q = (i // 16) % 4
        return np.where(c % 3 == 0, 5, np.where(c % 3 == 1, q + 1, np.where(q == 3, 9, 5))).astype(np.uint8)
    x = rng.integers(0, 256, n, dtype=np.uint8) if kind == "short uniform" else np.zeros(n, np.uint8)
    last = (n - 1) // 64 * 64
    if kind == "short uniform":
        x[last:] = 9
    else:
        assert kind == "short mixed"
        x[n - 1] = 1                                              # (a chunk of one byte is uniform: length 1 and 65 check that too)
    return x


def _reference(segs):
    pairs = [U.probe(s) for s in segs]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def _place(segs, shift):
    """the segments in one buffer, each `shift` bytes behind a 16-byte boundary"""
    off, pos = [], 0
    for s in segs:
        pos = (pos + 15) // 16 * 16 + shift
        off.append(pos)
        pos += s.size
    buf = np.full(pos + 64, 0xEE, np.uint8)
    for o, s in zip(off, segs):
        buf[o:o + s.size] = s
    return buf, off


def _gpu(x):
    import torch
    return torch.from_numpy(np.array(x, copy=True)).cuda()


@pytest.mark.parametrize("shift", [0, 1, 3, 15])
def test_probe_equals_numpy(glc, cuda, shift):
    import torch
    rng = np.random.default_rng(40 + shift)
    segs = [content(kind, n, rng) for kind in CONTENTS for n in LENGTHS]
    want_h, want_u = _reference(segs)
    assert int(want_u.sum()) > 0 and int((want_u > 0).sum(axis=1).max()) >= 2
    buf, off = _place(segs, shift)
    d = _gpu(buf)
    assert d.data_ptr() % 16 == 0
    garbage = [torch.full((len(segs), 256), -0x21524111, dtype=torch.int32, device=cuda) for _ in range(2)]
    hist, uniform = glc.probe_segments(d, off, [s.size for s in segs], hist=garbage[0], uniform=garbage[1])
    assert np.array_equal(hist.cpu().numpy().view(np.uint32), want_h)
    assert np.array_equal(uniform.cpu().numpy().view(np.uint32), want_u)
    assert bytes(d.cpu().numpy()) == buf.tobytes()                # (the input is only read)


def test_mixed_batch_with_clamping(glc, cuda):
    import torch
    rng = np.random.default_rng(77)
    lengths = [int(v) for v in rng.integers(1, 100000, 38)] + [1, 50000, 50001]
    max_len = 50000
    segs = [content(CONTENTS[i % len(CONTENTS)], n, rng) for i, n in enumerate(lengths)]
    shifts = rng.integers(0, 16, len(segs))
    off, pos = [], 0
    for s, sh in zip(segs, shifts):
        pos = (pos + 15) // 16 * 16 + int(sh)
        off.append(pos)
        pos += s.size
    buf = np.zeros(pos + 16, np.uint8)
    for o, s in zip(off, segs):
        buf[o:o + s.size] = s
    want_h, want_u = _reference([s[:max_len] for s in segs])
    garbage = [torch.full((len(segs), 256), 0x5A5A5A5A, dtype=torch.int32, device=cuda) for _ in range(2)]
    hist, uniform = glc.probe_segments(_gpu(buf), off, lengths, max_len=max_len, hist=garbage[0], uniform=garbage[1])
    assert np.array_equal(hist.cpu().numpy().view(np.uint32), want_h)
    assert np.array_equal(uniform.cpu().numpy().view(np.uint32), want_u)
    assert int(hist.sum(dim=1).max()) == max_len


def test_nothing_to_do_and_refusals_write_nothing(glc, cuda):
    import torch
    d = _gpu(np.arange(4096, dtype=np.uint8))
    rows = torch.full((2, 256), 123, dtype=torch.int32, device=cuda)
    other = torch.full((2, 256), 456, dtype=torch.int32, device=cuda)
    h, u = glc.probe_segments(d, [], [], max_len=64, hist=rows, uniform=other)
    assert h.numel() == 0 and u.numel() == 0
    off = torch.zeros(1, dtype=torch.int64, device=cuda)
    ln = torch.full((1,), 4096, dtype=torch.int64, device=cuda)
    L = glc._ct()
    for args in ((d.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, (1 << 20) + 1, rows.data_ptr(), other.data_ptr()),
                 (d.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, 4096, rows.data_ptr() + 2, other.data_ptr()),
                 (d.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, 4096, rows.data_ptr(), rows.data_ptr()),
                 (d.data_ptr(), None, ln.data_ptr(), 1, 4096, rows.data_ptr(), other.data_ptr())):
        assert L.glcProbeSegments(*args, None) == glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION
    torch.cuda.synchronize()
    assert bool((rows == 123).all()) and bool((other == 456).all())
    h, u = glc.probe_segments(d, [0], [4096], hist=rows, uniform=other)      # and then it does work
    assert int(h.sum()) == 4096 and int(u.sum()) == 0 and bool((rows[1] == 123).all())
