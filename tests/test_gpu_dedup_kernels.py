"""The two dedup passes on the MI355X (-m gpu): glcDedupMapSegments against dedup_model.map_segments, entry for entry, and
glcDedupFillSegments against dedup_model.fill_segments, at the lengths where a chunk is short, exact or one byte over, with one
and several blocks of 32 chunks, for one, two and five segments and base alignments 0, 1 and 3, with guards around everything
written.  The model's answer for a batch is computed once and shared by the shifts."""
import numpy as np
import pytest

import dedup_model as D

pytestmark = pytest.mark.gpu

ILLEGAL = 2
LENGTHS = (511, 512, 513, 1031, 4096, 65536)
COUNTS = (1, 2, 5)
SHIFTS = (0, 1, 3)
PATTERNS = ("zeros", "distinct", "twins")
GUARD, GUARD_WORD = 0xA5, 0x5EEDBEEF


def _segments(n, count, pattern):
    rng = np.random.default_rng(1000 * n + 10 * count + len(pattern))
    nch = D.nchunks(n)
    if pattern == "zeros":                                        # every chunk of full length sources chunk 0: the skip-insert path
        return [np.zeros(n, np.uint8) for _ in range(count)]
    if pattern == "distinct":
        return [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(count)]
    # twins: chunks from a pool of four, twins of them that differ only in byte 0 or in byte 511, the same short last chunk in
    # every segment, and a full chunk whose head is that short chunk (the short one must stay kept in segment 0)
    pool = rng.integers(0, 256, (4, D.CHUNK), dtype=np.uint8)
    tail = rng.integers(0, 256, D.CHUNK, dtype=np.uint8)
    segs = []
    for i in range(count):
        s = np.zeros(nch * D.CHUNK, np.uint8)
        for c in range(nch):
            ch = pool[rng.integers(0, 4)].copy()
            r = rng.integers(0, 6)
            if r == 0:
                ch[0] ^= 0x80
            elif r == 1:
                ch[511] ^= 0x01
            elif r == 2:
                ch = rng.integers(0, 256, D.CHUNK, dtype=np.uint8)
            s[D.CHUNK * c:D.CHUNK * (c + 1)] = ch
        if nch > 1:
            s[D.CHUNK * ((i + 1) % (nch - 1)):][:D.CHUNK] = tail   # the full chunk whose head the short last chunk repeats
        s[D.CHUNK * (nch - 1):] = tail
        segs.append(s[:n])
    return segs


def _pack(segs, gap=True):
    off, pos = [], 16
    for i, s in enumerate(segs):
        off.append(pos)
        pos += s.size + ((1 + (i * 7) % 16) if gap else 0)
    buf = np.full(pos + 64, GUARD, np.uint8)
    for o, s in zip(off, segs):
        buf[o:o + s.size] = s
    return dict(segs=segs, off=off, len=[s.size for s in segs], buf=buf, total=pos + 64)


_BATCHES = {}


def _batch(n, count, pattern):
    key = (n, count, pattern)
    if key not in _BATCHES:
        B = _pack(_segments(n, count, pattern), gap=pattern != "zeros")
        B["src"] = D.map_segments(B["segs"], n)
        _BATCHES[key] = B
    return _BATCHES[key]


def _map(glc, cuda, B, shift, max_len):
    import torch
    total, off, ln = B["total"], B["off"], B["len"]
    nch = D.nchunks(max_len)
    buf = torch.full((total + 32,), GUARD, dtype=torch.uint8, device=cuda)
    buf[shift:shift + total] = torch.from_numpy(B["buf"]).to(cuda)
    d_off = torch.tensor(off, dtype=torch.int64, device=cuda)
    d_len = torch.tensor(ln, dtype=torch.int64, device=cuda)
    src = torch.full((len(off) * nch + 2,), GUARD_WORD, dtype=torch.int32, device=cuda)          # a guard entry on either side
    L = glc._ct()
    wb = int(L.glcDedupWorkBytes(len(off), max_len))
    assert wb >= 16 * 2 * len(off) * nch + 8 * len(off) * nch
    work = torch.full((wb + 16,), GUARD, dtype=torch.uint8, device=cuda)
    assert work.data_ptr() % 16 == 0
    rc = L.glcDedupMapSegments(buf[shift:].data_ptr(), d_off.data_ptr(), d_len.data_ptr(), len(off), max_len, src[1:].data_ptr(),
                               work.data_ptr(), wb, None)
    assert rc == 0
    torch.cuda.synchronize()
    h = src.cpu().numpy().view(np.uint32)
    assert h[0] == GUARD_WORD and h[-1] == GUARD_WORD
    assert bool((work[wb:] == GUARD).all())
    assert np.array_equal(buf.cpu().numpy()[shift:shift + total], B["buf"])                       # the input is only read
    return h[1:-1]


def test_the_batches_cover_the_cases():
    for n in LENGTHS:
        nch = D.nchunks(n)
        z = _batch(n, 5, "zeros")["src"].reshape(5, nch)
        full = n // D.CHUNK
        assert (z[:, :full].reshape(-1)[1:] == 0).all() and z[0, 0] == 0                          # every full chunk sources chunk 0
        if n % D.CHUNK:
            assert z[0, -1] == nch - 1 and (z[1:, -1] == nch - 1).all()                           # the short ones the first short one
        d = _batch(n, 5, "distinct")["src"]
        assert np.array_equal(d, np.arange(d.size))
        t = _batch(n, 5, "twins")
        s = t["src"].reshape(5, nch)
        if n % D.CHUNK:
            assert s[0, -1] == nch - 1 and (s[1:, -1] == nch - 1).all()                           # equal short last chunks; the head
        if n >= 4096:                                                                             # of a full chunk is no source
            kept = s.reshape(-1) == np.arange(s.size)
            assert 0 < kept.sum() < s.size
    # twins that differ in byte 0 / byte 511 only are both kept
    a = np.arange(512, dtype=np.uint32).astype(np.uint8)
    b0, b511 = a.copy(), a.copy()
    b0[0] ^= 1
    b511[511] ^= 1
    assert D.map_segments([np.concatenate([a, b0, b511, a])], 2048).tolist() == [0, 1, 2, 0]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("n", LENGTHS)
def test_map_equals_the_model(glc, cuda, n, count, pattern):
    B = _batch(n, count, pattern)
    for shift in SHIFTS:
        got = _map(glc, cuda, B, shift, n)
        assert np.array_equal(got, B["src"]), (shift, np.nonzero(got != B["src"])[0][:8].tolist())


def test_twins_in_byte_0_and_byte_511(glc, cuda):
    a = np.random.default_rng(2).integers(0, 256, 512, dtype=np.uint8)
    b0, b511 = a.copy(), a.copy()
    b0[0] ^= 1
    b511[511] ^= 0x80
    B = _pack([np.concatenate([a, b0, b511, a, b0]), np.concatenate([b511, a, a[:100]]), np.concatenate([a[:100], a, b0, a[:100]])[:1124]])
    want = D.map_segments(B["segs"], 2560)
    assert want.reshape(3, 5).tolist() == [[0, 1, 2, 0, 1], [2, 0, 7, 8, 9], [10, 11, 12, 13, 14]]
    for shift in SHIFTS:
        assert np.array_equal(_map(glc, cuda, B, shift, 2560), want)


def test_ragged_segments_and_a_wider_max_len(glc, cuda):
    rng = np.random.default_rng(9)
    pool = rng.integers(0, 256, (3, 512), dtype=np.uint8)
    lens = [1031, 512, 0, 2000, 513, 40000]
    segs = [np.concatenate([pool[rng.integers(0, 3)] for _ in range(D.nchunks(n) or 1)])[:n] for n in lens]
    B = _pack(segs)
    for max_len in (40000, 40000 + 4096, 1024):                   # rows wider than any segment; and segments cut at max_len
        want = D.map_segments(segs, max_len)
        for shift in (0, 3):
            assert np.array_equal(_map(glc, cuda, B, shift, max_len), want), max_len


def _fill(glc, cuda, B, src, shift, max_len):
    import torch
    total = B["total"]
    buf = torch.full((total + 32,), GUARD, dtype=torch.uint8, device=cuda)
    buf[shift:shift + total] = torch.from_numpy(B["buf"]).to(cuda)
    d_off = torch.tensor(B["off"], dtype=torch.int64, device=cuda)
    d_len = torch.tensor(B["len"], dtype=torch.int64, device=cuda)
    d_src = torch.from_numpy(src.astype(np.uint32).view(np.int32)).to(cuda)
    rc = glc._ct().glcDedupFillSegments(buf[shift:].data_ptr(), d_off.data_ptr(), d_len.data_ptr(), len(B["off"]), max_len, d_src.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    want = np.full(total + 32, GUARD, np.uint8)
    want[shift:shift + total] = B["buf"]
    for o, s in zip(B["off"], D.fill_segments(B["segs"], src, max_len)):
        want[shift + o:shift + o + s.size] = s
    assert np.array_equal(buf.cpu().numpy(), want)


@pytest.mark.parametrize("n", LENGTHS)
def test_fill_restores_what_map_elided(glc, cuda, n):
    B = _batch(n, 5, "twins")
    holes = _pack([np.where(np.repeat(B["src"].reshape(5, -1)[i] != np.arange(i * D.nchunks(n), (i + 1) * D.nchunks(n)), D.CHUNK)[:n], 0xEE, s)
                   .astype(np.uint8) for i, s in enumerate(B["segs"])])
    assert holes["off"] == B["off"]
    import torch
    for shift in SHIFTS:
        buf = torch.full((B["total"] + 32,), GUARD, dtype=torch.uint8, device=cuda)
        buf[shift:shift + B["total"]] = torch.from_numpy(holes["buf"]).to(cuda)
        glc.dedup_fill_segments(buf[shift:], B["off"], B["len"], torch.from_numpy(B["src"].view(np.int32)).to(cuda), n)
        want = np.full(B["total"] + 32, GUARD, np.uint8)
        want[shift:shift + B["total"]] = B["buf"]
        assert np.array_equal(buf.cpu().numpy(), want)


def test_fill_skips_bad_entries(glc, cuda):
    rng = np.random.default_rng(4)
    lens = [2048, 1031, 2048, 700]
    segs = [rng.integers(0, 256, n, dtype=np.uint8) for n in lens]
    B = _pack(segs)
    nch = 4
    src = np.arange(4 * nch, dtype=np.uint32)
    src[1] = 0                       # good: a full chunk from a full chunk
    src[2] = 2                       # its own id
    src[3] = 9                       # a later chunk
    src[4 + 1] = 2                   # good
    src[4 + 2] = 0                   # the short chunk (7 bytes) from a full one
    src[4 + 3] = 0                   # an id past its segment's end: no chunk there
    src[8 + 0] = 4 + 2               # a full chunk from a short one
    src[8 + 1] = 4 + 3               # a source past its segment's end
    src[8 + 2] = 0xFFFFFFFF          # no such id
    src[8 + 3] = 0                   # good, across two segments
    src[12 + 1] = 0                  # the short chunk (188 bytes) from a full one
    src[12 + 0] = 8                  # good
    want = D.fill_segments(segs, src, 2048)
    changed = [[bool((w[512 * c:512 * c + 512] != s[512 * c:512 * c + 512]).any()) for c in range(D.nchunks(s.size))] for w, s in zip(want, segs)]
    assert changed == [[False, True, False, False], [False, True, False], [False, False, False, True], [True, False]]
    for shift in SHIFTS:
        _fill(glc, cuda, B, src, shift, 2048)


def test_bad_arguments_are_refused_with_nothing_written(glc, cuda):
    import torch
    B = _batch(1031, 2, "twins")
    nch = D.nchunks(1031)
    buf = torch.from_numpy(B["buf"]).to(cuda)
    d_off = torch.tensor(B["off"], dtype=torch.int64, device=cuda)
    d_len = torch.tensor(B["len"], dtype=torch.int64, device=cuda)
    src = torch.full((2 * nch + 1,), GUARD_WORD, dtype=torch.int32, device=cuda)
    L = glc._ct()
    wb = int(L.glcDedupWorkBytes(2, 1031))
    work = torch.full((wb + 16,), GUARD, dtype=torch.uint8, device=cuda)
    good = [buf.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), 2, 1031, src.data_ptr(), work.data_ptr(), wb]
    bad = []
    for i in (0, 1, 2, 5, 6):
        a = list(good)
        a[i] = None
        bad.append(a)
    bad += [good[:5] + [good[5] + 2] + good[6:], good[:6] + [good[6] + 8, wb], good[:7] + [wb - 1], good[:4] + [(1 << 20) + 1] + good[5:],
            good[:3] + [(1 << 22) + 1, 1] + good[5:], good[:3] + [1 << 22, 1 << 20] + good[5:]]
    for a in bad:
        assert L.glcDedupMapSegments(*a, None) == ILLEGAL, a
    fgood = good[:4] + [1031, src.data_ptr()]
    fbad = []
    for i in (0, 1, 2, 5):
        a = list(fgood)
        a[i] = None
        fbad.append(a)
    fbad += [fgood[:5] + [fgood[5] + 2], fgood[:4] + [(1 << 20) + 1, fgood[5]], fgood[:3] + [(1 << 22) + 1, 1, fgood[5]]]
    src_before = src.clone()
    for a in fbad:
        assert L.glcDedupFillSegments(*a, None) == ILLEGAL, a
    torch.cuda.synchronize()
    assert bool((src == src_before).all()) and bool((src.view(torch.int32) == GUARD_WORD).all()) and bool((work == GUARD).all())
    assert np.array_equal(buf.cpu().numpy(), B["buf"])
    assert L.glcDedupWorkBytes(2, (1 << 20) + 1) == 0 and L.glcDedupWorkBytes((1 << 22) + 1, 1) == 0 and L.glcDedupWorkBytes(1 << 22, 1 << 20) == 0
    assert L.glcDedupWorkBytes(0, 1031) == 0 and L.glcDedupMapSegments(None, None, None, 0, 1031, None, None, 0, None) == 0
    with pytest.raises(glc.CudppError):                          # the binding raises on the same
        glc.dedup_fill_segments(buf, B["off"], B["len"], torch.zeros(2 * 2049, dtype=torch.int32, device=cuda), (1 << 20) + 1)
    got = glc.dedup_map_segments(buf, B["off"], B["len"], 1031)  # and the binding's own call
    assert np.array_equal(got.cpu().numpy().view(np.uint32), B["src"])
