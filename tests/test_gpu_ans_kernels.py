"""The rANS kernels of csrc/ans.hip on the MI355X (-m gpu), through glcAnsEncodeSegments / glcAnsDecodeSegments: histograms and
records word for word the Python model's (tests/ans_model.py), the decode the input, for the lengths at which the code takes
another path (below a step, a step, one byte more, a batch of 16 steps and a byte, a chunk, a chunk and a byte, two chunks and
a part, the largest segment), six kinds of data, every byte alignment class of input and output, batches of 1, 7 and 300
segments; the tolerant decoder writes nothing outside its segments whatever the records hold; the refused arguments."""
import numpy as np
import pytest

import ans_inputs as I
import ans_model as A

pytestmark = pytest.mark.gpu

ILLEGAL = 2
LENGTHS = (1, 63, 64, 65, 4097, 32768, 32769, 70000)
GUARD = 64
_MODEL = {}


def _segment(kind, n):
    """(bytes, hist, record) of the model, computed once"""
    if (kind, n) not in _MODEL:
        x = I.segment(kind, n, np.random.default_rng(1000 + n + 7 * I.KINDS.index(kind)))
        x.setflags(write=False)
        _MODEL[kind, n] = (x,) + A.encode_record(x)
    return _MODEL[kind, n]


def _place(segs, shift):
    """one host buffer of 0xEE with the segments at offsets = shift mod 16, GUARD bytes apart at least"""
    off, pos = [], 0
    for x in segs:
        pos = (pos + GUARD + 15) // 16 * 16 + shift
        off.append(pos)
        pos += x.size
    buf = np.full(pos + GUARD + 16, 0xEE, np.uint8)
    for o, x in zip(off, segs):
        buf[o:o + x.size] = x
    return buf, off


def _round_trip(glc, cuda, items, in_shift=0, out_shift=0, max_len=None):
    """encode the model segments `items` in one call, compare with the model, decode in one call into guarded space"""
    import torch
    segs = [it[0] for it in items]
    lens = [x.size for x in segs]
    buf, off = _place(segs, in_shift)
    d_in = torch.from_numpy(buf).to(cuda)
    assert d_in.data_ptr() % 16 == 0
    hist, rec, rec_off, words = glc.ans_encode_segments(d_in, off, lens, max_len=max_len)
    hist, rec_h, words = hist.cpu().numpy().view(np.uint32), rec.cpu().numpy().view(np.uint32), words.cpu().numpy()
    for i, (x, h, w) in enumerate(items):
        assert np.array_equal(hist[i], h), i
        assert int(words[i]) == w.size and w.size <= glc.ans_bound_words(x.size) == A.bound_words(x.size), i
        assert np.array_equal(rec_h[rec_off[i]:rec_off[i] + w.size], w), (i, x.size)
    obuf, ooff = _place([np.full(n, 0xAB, np.uint8) for n in lens], out_shift)
    obuf[:] = 0xAB
    d_out = torch.from_numpy(obuf).to(cuda)
    glc.ans_decode_segments(rec, rec_off, words, torch.from_numpy(hist.view(np.int32)).to(cuda), d_out, ooff, lens, max_len=max_len)
    got = d_out.cpu().numpy()
    want = obuf.copy()
    for o, x in zip(ooff, segs):
        want[o:o + x.size] = x
    assert np.array_equal(got, want)                              # the segments, and every guard byte around them untouched
    return rec, rec_off, words, hist


@pytest.mark.parametrize("kind", I.KINDS)
def test_lengths_word_for_word(glc, cuda, kind):
    _round_trip(glc, cuda, [_segment(kind, n) for n in LENGTHS])


def test_the_largest_segment(glc, cuda):
    _round_trip(glc, cuda, [_segment(kind, 1 << 20) for kind in ("scattered", "all256", "noise")])
    assert A.quantise(_segment("all256", 1 << 20)[1], 1 << 20)[1]   # the R < 0 path


def test_the_quantiser_paths_are_covered():
    assert A.quantise(_segment("all256", 70000)[1], 70000)[1] and A.quantise(_segment("dominant", 70000)[1], 70000)[1]
    assert not A.quantise(_segment("scattered", 70000)[1], 70000)[1]
    assert _segment("constant", 32768)[2].size * 4 == 260


@pytest.mark.parametrize("in_shift", (0, 1, 7, 15))
@pytest.mark.parametrize("out_shift", (0, 1, 7, 15))
def test_alignment(glc, cuda, in_shift, out_shift):
    items = [_segment("scattered", n) for n in (1, 63, 65, 4097, 32769)] + [_segment("geometric", 70000)]
    _round_trip(glc, cuda, items, in_shift, out_shift)


@pytest.mark.parametrize("count", (1, 7, 300))
def test_batches_of_mixed_lengths(glc, cuda, count):
    rng = np.random.default_rng(count)
    lens = [int(v) for v in rng.integers(1, 3000, count)]
    lens[0] = 40000
    if count > 2:
        lens[count // 2], lens[-1] = 1, 32768
    items = [_segment(I.KINDS[i % len(I.KINDS)], n) for i, n in enumerate(lens)]
    _round_trip(glc, cuda, items, max_len=40000)


def test_the_decoder_is_tolerant(glc, cuda):
    """records of garbage, counts beyond the record, and record sizes cut short: whatever comes out, it stays inside the
    segments (guard bytes around every one), and the call returns"""
    import torch
    items = [_segment("scattered", n) for n in (1, 65, 4097, 32769, 70000)]
    lens = [it[0].size for it in items]
    rec, rec_off, words, hist = _round_trip(glc, cuda, items)
    d_hist = torch.from_numpy(hist.view(np.int32)).to(cuda)
    rng = np.random.default_rng(5)
    good = rec.cpu().numpy().view(np.uint32)
    variants = []
    g = rng.integers(0, 1 << 32, good.size, dtype=np.uint64).astype(np.uint32)      # everything garbage, counts included
    variants.append((g, [int(w) for w in words]))
    g = good.copy()                                                                   # garbage units behind true counts
    for i, (o, w) in enumerate(zip(rec_off, words)):
        nch = A.nchunks(lens[i])
        g[o + nch + A.LANES:o + int(w)] = rng.integers(0, 1 << 32, int(w) - nch - A.LANES, dtype=np.uint64).astype(np.uint32)
    variants.append((g, [int(w) for w in words]))
    g = good.copy()                                                                   # counts larger than the record holds
    for i, o in enumerate(rec_off):
        g[o:o + A.nchunks(lens[i])] = 0xFFFFFFFF
    variants.append((g, [int(w) for w in words]))
    for cut in (0, 1, 2, 66, 70):                                                     # record sizes cut short
        variants.append((good.copy(), [min(int(w), cut) for w in words]))
    variants.append((good.copy(), [int(w) // 2 for w in words]))
    for recs, sizes in variants:
        obuf, ooff = _place([np.full(n, 0xAB, np.uint8) for n in lens], 3)
        obuf[:] = 0xAB
        inside = np.zeros(obuf.size, bool)
        for o, n in zip(ooff, lens):
            inside[o:o + n] = True
        d_out = torch.from_numpy(obuf).to(cuda)
        glc.ans_decode_segments(torch.from_numpy(recs.view(np.int32)).to(cuda), rec_off, sizes, d_hist, d_out, ooff, lens)
        got = d_out.cpu().numpy()
        assert bool((got[~inside] == 0xAB).all())


def test_refused_arguments(glc, cuda):
    import torch
    L = glc._ct()
    x = torch.zeros(4096, dtype=torch.uint8, device=cuda)
    off = torch.zeros(1, dtype=torch.int64, device=cuda)
    ln = torch.full((1,), 1000, dtype=torch.int64, device=cuda)
    hist = torch.full((256,), -1, dtype=torch.int32, device=cuda)
    rec = torch.full((glc.ans_bound_words(1000) + 4,), -1, dtype=torch.int32, device=cuda)
    words = torch.full((1,), -1, dtype=torch.int64, device=cuda)
    nbytes = glc.ans_work_bytes(1, 1000)
    assert nbytes > 65536 and glc.ans_work_bytes(1, (1 << 20) + 1) == 0 and glc.ans_work_bytes((1 << 22) + 1, 16) == 0
    assert glc.ans_bound_words((1 << 20) + 1) == 0 and glc.ans_bound_words(1 << 20) == A.bound_words(1 << 20)
    work = torch.zeros(nbytes, dtype=torch.uint8, device=cuda)
    good = [x.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, 1000, hist.data_ptr(), rec.data_ptr(), off.data_ptr(), words.data_ptr(),
            work.data_ptr(), nbytes, None]
    bad = []
    for i in (0, 1, 2, 5, 6, 7, 8, 9):                            # a null pointer
        a = list(good)
        a[i] = None
        bad.append(a)
    for i, v in ((3, (1 << 22) + 1), (4, (1 << 20) + 1), (10, nbytes - 1), (6, rec.data_ptr() + 2), (5, hist.data_ptr() + 1),
                 (6, x.data_ptr())):
        a = list(good)
        a[i] = v
        bad.append(a)
    for a in bad:
        assert L.glcAnsEncodeSegments(*a) == ILLEGAL
    dgood = [rec.data_ptr(), off.data_ptr(), words.data_ptr(), hist.data_ptr(), off.data_ptr(), ln.data_ptr(), 1, 1000, x.data_ptr(),
             work.data_ptr(), nbytes, None]
    for i, v in ((0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (8, None), (9, None), (6, (1 << 22) + 1),
                 (7, (1 << 20) + 1), (10, nbytes - 1), (0, rec.data_ptr() + 1), (8, rec.data_ptr())):
        a = list(dgood)
        a[i] = v
        assert L.glcAnsDecodeSegments(*a) == ILLEGAL
    torch.cuda.synchronize()
    assert bool((hist == -1).all()) and bool((rec == -1).all()) and bool((words == -1).all()) and bool((x == 0).all())
    a = list(good)                                                # count 0: nothing to do, whatever the pointers
    a[3] = 0
    a[0] = a[9] = None
    assert L.glcAnsEncodeSegments(*a) == 0
