"""The two passes of the sparse mode on the MI355X (-m gpu): glcSparseSplitSegments and glcSparseJoinSegments against
sparse_model.split / join, byte for byte, mask words and kept lengths included, at the lengths where the kernels change path (chunk,
wave pass, mask word and tile boundaries), for every byte alignment of the two bases, with guard bytes around everything written."""
import numpy as np
import pytest

import sparse_model as S

pytestmark = pytest.mark.gpu

ILLEGAL = 2
LENGTHS = (1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 16383, 16384, 16385, 65536 + 77)
GUARD, GUARD_WORD = 0xA5, 0x5EEDBEEF


def _patterns(n, rng):
    """[(block, fill)] of n bytes"""
    nch = S.nchunks(n)
    last = 64 * (nch - 1)
    out = [(np.full(n, 0x10, np.uint8), 0x10),                                   # all fill
           (rng.integers(1, 256, n, dtype=np.uint8), 0)]                         # nothing elidable
    alt = np.zeros(n, np.uint8)                                                  # kept and elided alternating
    for c in range(0, nch, 2):
        alt[64 * c:64 * c + 64] = rng.integers(0, 256, min(64, n - 64 * c), dtype=np.uint8) | 1
    out.append((alt, 0))
    one = np.full(n, 0xFF, np.uint8)                                             # one byte in the first / last byte of a chunk,
    one[64 * (nch // 2)] = 0                                                     # and in the short last chunk
    if n > 64:
        one[min(64 * (nch // 3) + 63, n - 1)] = 1
    one[n - 1] = 7
    out.append((one, 0xFF))
    tail = rng.integers(0, 256, n, dtype=np.uint8)                               # a (short) last chunk that is all fill
    tail[last:] = 0x10
    out.append((tail, 0x10))
    rep = np.zeros(n, np.uint8)                                                  # a chunk of one repeated non-fill byte
    rep[64 * (nch // 2):64 * (nch // 2) + 64] = 0x33
    out.append((rep, 0))
    return out


_BATCH = {}


def _batch():
    """the segments of every length and pattern packed with gaps of 1 to 16 bytes (so every alignment occurs), and what the model
    makes of each: computed once"""
    if not _BATCH:
        rng = np.random.default_rng(11)
        segs = [p for n in LENGTHS for p in _patterns(n, rng)]
        _BATCH.update(_pack(segs))
    return _BATCH


def _pack(segs, rng_gap=None):
    off, pos = [], 5
    for i, (blk, _) in enumerate(segs):
        off.append(pos)
        pos += blk.size + 1 + (i * 7) % 16
    buf = np.full(pos + 64, GUARD, np.uint8)
    for o, (blk, _) in zip(off, segs):
        buf[o:o + blk.size] = blk
    model = [S.split(blk, fill) for blk, fill in segs]
    return dict(segs=segs, off=off, len=[b.size for b, _ in segs], fill=[f for _, f in segs], buf=buf, model=model, total=pos + 64)


def _run(glc, cuda, B, in_shift, out_shift, max_len=None):
    """split then join of the batch B with the bases shifted; every written byte and every guard checked"""
    import torch
    total, off, ln, fill = B["total"], B["off"], B["len"], B["fill"]
    max_len = max(ln) if max_len is None else max_len
    mw = glc.sparse_mask_words(max_len)
    src = torch.full((total + 32,), GUARD, dtype=torch.uint8, device=cuda)
    src[in_shift:in_shift + total] = torch.from_numpy(B["buf"]).to(cuda)
    kept = torch.full((total + 32,), GUARD, dtype=torch.uint8, device=cuda)
    d_off = torch.tensor(off, dtype=torch.int64, device=cuda)
    d_len = torch.tensor(ln, dtype=torch.int64, device=cuda)
    d_fill = torch.tensor(fill, dtype=torch.int32, device=cuda)
    mask = torch.full((len(off) + 2, mw), GUARD_WORD, dtype=torch.int32, device=cuda)        # a guard row on either side
    klen = torch.full((len(off) + 2,), -1, dtype=torch.int64, device=cuda)
    L = glc._ct()
    rc = L.glcSparseSplitSegments(src[in_shift:].data_ptr(), d_off.data_ptr(), d_len.data_ptr(), len(off), max_len, d_fill.data_ptr(),
                                  mask[1:].data_ptr(), kept[out_shift:].data_ptr(), klen[1:].data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    h_mask, h_klen, h_kept = mask.cpu().numpy().view(np.uint32), klen.cpu().numpy(), kept.cpu().numpy()
    assert (h_mask[0] == GUARD_WORD).all() and (h_mask[-1] == GUARD_WORD).all() and h_klen[0] == -1 and h_klen[-1] == -1
    want_kept = np.full(total + 32, GUARD, np.uint8)
    for i, (f, m, K) in enumerate(B["model"]):
        assert h_mask[1 + i, :m.size].tolist() == m.tolist(), (i, ln[i])
        assert (h_mask[1 + i, m.size:] == GUARD_WORD).all(), (i, ln[i])          # nothing past the segment's own words
        assert int(h_klen[1 + i]) == K.size, (i, ln[i])
        want_kept[out_shift + off[i]:out_shift + off[i] + K.size] = K
    assert np.array_equal(h_kept, want_kept)
    assert np.array_equal(src.cpu().numpy()[in_shift:in_shift + total], B["buf"])                  # the input is only read
    # join: the kept bytes at the input's shift now, the output at the other
    out = torch.full((total + 32,), GUARD, dtype=torch.uint8, device=cuda)
    rc = L.glcSparseJoinSegments(kept[out_shift:].data_ptr(), d_off.data_ptr(), d_len.data_ptr(), len(off), max_len, d_fill.data_ptr(),
                                 mask[1:].data_ptr(), out[in_shift:].data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    want = np.full(total + 32, GUARD, np.uint8)
    for o, (blk, _) in zip(off, B["segs"]):
        want[in_shift + o:in_shift + o + blk.size] = blk
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(kept.cpu().numpy(), want_kept)


def test_the_model_batch_covers_the_cases():
    B = _batch()
    assert len(B["segs"]) == 6 * len(LENGTHS) and {a % 16 for a in B["off"]} == set(range(16))
    kept = [K.size for _, _, K in B["model"]]
    assert 0 in kept and any(k == n for k, n in zip(kept, B["len"])) and {0, 0x10, 0xFF} == set(B["fill"])


@pytest.mark.parametrize("in_shift", [0, 1, 7, 15])
@pytest.mark.parametrize("out_shift", [0, 1, 7, 15])
def test_split_and_join_equal_the_model(glc, cuda, in_shift, out_shift):
    _run(glc, cuda, _batch(), in_shift, out_shift)


def test_one_segment_of_a_mebibyte(glc, cuda):
    rng = np.random.default_rng(3)
    n = 1 << 20
    blk = np.zeros(n, np.uint8)
    for c in rng.choice(n // 64, 3000, replace=False):
        blk[64 * c + rng.integers(0, 64)] = rng.integers(1, 256)
    blk[64 * 8191 + 63] = 9                                                     # the last chunk of a tile, and the first of the next
    blk[64 * 8192] = 9
    blk[n - 1] = 1
    for shifts in ((0, 0), (1, 15)):
        _run(glc, cuda, _pack([(blk, 0)]), *shifts)


def test_a_batch_of_300_segments_of_mixed_lengths(glc, cuda):
    rng = np.random.default_rng(5)
    segs = []
    for i in range(300):
        n = int(rng.choice([0, 1, 64, 100, 1024, 2048, 3000, 5000, 16384, 20000])) if i % 3 else int(rng.integers(0, 6000))
        fill = int(rng.choice([0, 0x10, 0xFF]))
        blk = np.full(n, fill, np.uint8)
        m = rng.random(S.nchunks(n)) < 0.4
        for c in np.nonzero(m)[0]:
            blk[64 * c:64 * c + 64] = rng.integers(0, 256, min(64, n - 64 * c), dtype=np.uint8)
        segs.append((blk, fill))
    B = _pack(segs)
    assert 0 in B["len"]
    _run(glc, cuda, B, 0, 0)
    _run(glc, cuda, B, 7, 1, max_len=20000 + 4096)                             # mask rows wider than any segment needs


def test_bad_arguments_are_refused_with_nothing_written(glc, cuda):
    import torch
    B = _pack(_patterns(1025, np.random.default_rng(1)))
    n = len(B["off"])
    src = torch.from_numpy(B["buf"]).to(cuda)
    kept = torch.full((B["total"],), GUARD, dtype=torch.uint8, device=cuda)
    d_off = torch.tensor(B["off"], dtype=torch.int64, device=cuda)
    d_len = torch.tensor(B["len"], dtype=torch.int64, device=cuda)
    d_fill = torch.tensor(B["fill"], dtype=torch.int32, device=cuda)
    mask = torch.full((n, 4), GUARD_WORD, dtype=torch.int32, device=cuda)
    klen = torch.full((n,), -1, dtype=torch.int64, device=cuda)
    L = glc._ct()
    good = [src.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, 1025, d_fill.data_ptr(), mask.data_ptr(), kept.data_ptr(), klen.data_ptr()]
    bad = []
    for i in (0, 1, 2, 5, 6, 7, 8):
        a = list(good)
        a[i] = None
        bad.append(a)
    bad += [good[:7] + [good[0], good[8]], good[:6] + [good[6] + 2] + good[7:], good[:4] + [(1 << 28) + 1] + good[5:],
            good[:3] + [1 << 32] + good[4:]]
    for a in bad:
        assert L.glcSparseSplitSegments(*a, None) == ILLEGAL
    for a in bad:
        if a[8] is None:
            continue
        j = a[:8]
        if j[7] == good[0]:
            j[0] = j[7] = good[7]
        assert L.glcSparseJoinSegments(*j, None) == ILLEGAL
    torch.cuda.synchronize()
    assert bool((kept == GUARD).all()) and bool((mask.view(torch.int32) == GUARD_WORD).all()) and bool((klen == -1).all())
    assert np.array_equal(src.cpu().numpy(), B["buf"])
    with pytest.raises(glc.CudppError):                                         # the binding raises on the same
        glc.sparse_split_segments(src, src, B["off"], B["len"], B["fill"])
    m, k = glc.sparse_split_segments(src, kept, B["off"], B["len"], B["fill"])  # and the binding's own round trip
    out = torch.zeros_like(src)
    glc.sparse_join_segments(kept, out, B["off"], B["len"], B["fill"], m)
    for o, (blk, _), (_, mm, K) in zip(B["off"], B["segs"], B["model"]):
        assert np.array_equal(out[o:o + blk.size].cpu().numpy(), blk)
    assert k.tolist() == [K.size for _, _, K in B["model"]]
