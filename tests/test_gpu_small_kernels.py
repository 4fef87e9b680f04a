"""The encoder's small kernels against the oracle, word for word (-m gpu): the full-block instance of k_huff_pack and the
guarded one beside it, the half-width sub-block histograms through their four producers and k_huff_build, and the
first-occurrence test of k_mtf_chunk_lists' aligned full-chunk arm.

Packer: the host picks the full-block instance when n is a multiple of 4 x 4096 and the symbols start 16-byte aligned;
16384 is the smallest such n, 32768 has two workgroups per block, 20480 / 12288 / 4096 / 5000 and a view offset by one
byte take the guarded instance.  A block whose longest code is at most 14 bits joins two symbols' codes before the
merge, one whose longest is 15 or more does not: both through the full-block instance.

Sub-histograms: a count of 4096 in the low half of a dword (rank 5) and in the high half (rank 200), as symbols given to
the stand-alone Huffman stage (k_sub_hist) and as MTF ranks of cudppCompress (k_mtf_encode: `_cycling` builds a block
whose BWT cycles through m symbols over whole sub-blocks, so their MTF ranks are all m - 1); 520 blocks of 16384 are more
than 2048 chunks (the FULL instance writes them), 700 blocks of 12288 take the ragged instance, one block the QUARTERS one.

Chunk lists: two chunks, so that the list of chunk 0 decides the ranks at the start of chunk 1; the chunks hold what a
short cut for symbols already met in a chunk's last 1024 bytes could get wrong (two such short cuts were built on these
tests, measured no faster than the kernel as it is, and taken out again: profiles/small_kernels.md)."""
import functools

import numpy as np
import pytest

import datagen
import oracle_lib as O

pytestmark = pytest.mark.gpu

SUB = 4096


def _same(out, k, want, what, index=True):
    nsub, stride = out["nsub"], out["stride"]
    if index:
        assert int(out["bwt_index"][k].item()) == want["bwt_index"], what + ": BWT index"
    assert np.array_equal(out["hist"][256 * k: 256 * k + 256].cpu().numpy().view(np.uint32), want["hist"]), what + ": histogram"
    assert np.array_equal(out["offsets"][nsub * k: nsub * (k + 1)].cpu().numpy().view(np.uint32), want["offsets"]), what + ": offsets"
    size = int(out["size"][k].item())
    assert size == want["size"], what + ": size"
    got = out["words"][stride * k: stride * k + size].cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want["words"]), what + ": stream words"


def _huffman(glc, cuda, x, off=0):
    """rows of x through the stand-alone Huffman stage, read from a tensor view `off` bytes into its allocation"""
    import torch
    nblk, n = x.shape
    d = torch.zeros(n * nblk + off, dtype=torch.uint8, device=cuda)
    d[off:] = torch.from_numpy(x.reshape(-1).copy()).to(cuda)
    view = d[off:]
    assert view.data_ptr() % 16 == off
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=nblk) as plan:
        out = glc.huffman_encode_batch(plan, view, n, nblk)
        plan.synchronize()
        for k in range(nblk):
            want = O.huff_encode(x[k])
            assert want["rc"] == 0
            assert np.array_equal(want["hist"], np.bincount(x[k], minlength=256))
            _same(out, k, want, "n %d block %d of %d (offset %d)" % (n, k, nblk, off), index=False)


def _compress(glc, cuda, x, check=None):
    """rows of x through cudppCompress's batch form; d_hist also against a bincount of the oracle's MTF output"""
    import torch
    nblk, n = x.shape
    d = torch.from_numpy(x.reshape(-1).copy()).to(cuda)
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=nblk) as plan:
        out = glc.compress_batch(plan, d, n, nblk)
        plan.synchronize()
        for k in (range(nblk) if check is None else check):
            want = O.compress(x[k])
            assert want["rc"] == 0
            ranks = O.mtf(O.bwt(x[k])[0])
            assert np.array_equal(out["hist"][256 * k: 256 * k + 256].cpu().numpy().view(np.uint32),
                                  np.bincount(ranks, minlength=256)), "block %d: d_hist is not the histogram of the MTF output" % k
            _same(out, k, want, "n %d block %d of %d" % (n, k, nblk))


@functools.lru_cache(maxsize=None)
def _zipf_rows(n, rows):
    x = datagen.zipf_bytes(n * rows, seed=31 * n + rows).reshape(rows, n)
    x.setflags(write=False)
    return x


# ---- packer ----------------------------------------------------------------------------------------------------------
PACK_N = [16384, 32768, 20480, 12288, 4096, 5000]


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n", PACK_N)
def test_pack_huffman_stage(glc, cuda, n, rows):
    _huffman(glc, cuda, _zipf_rows(n, rows))


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n", PACK_N)
def test_pack_compress(glc, cuda, n, rows):
    _compress(glc, cuda, _zipf_rows(n, rows))


def test_pack_full_block_from_an_unaligned_view(glc, cuda):
    """n says full-block, the base is one byte past a 16-byte boundary: the guarded instance has to run"""
    _huffman(glc, cuda, _zipf_rows(16384, 3), off=1)


def _halving(n, rng):
    """counts n/2, n/4, ... 1, 1 in shuffled order: code lengths 1, 2, 3, ..."""
    parts, c, s = [], n // 2, 0
    while c >= 1:
        parts.append(np.full(c, s, dtype=np.uint8))
        c //= 2
        s += 1
    parts.append(np.full(1, s, dtype=np.uint8))
    x = np.concatenate(parts)
    assert x.size == n
    return rng.permutation(x)


def test_pack_full_block_short_and_long_codes(glc, cuda):
    n = 32768
    rng = np.random.default_rng(5)
    short = rng.integers(0, 256, n, dtype=np.uint8)
    long_ = _halving(n, rng)
    short_lens = O.huff_codes(np.bincount(short, minlength=256))[1]
    long_lens = O.huff_codes(np.bincount(long_, minlength=256))[1]
    assert short_lens.max() <= 14, "the short case must take the joined-pairs merge"
    assert long_lens.max() >= 15, "the long case must take the one-symbol merge"
    _huffman(glc, cuda, np.stack([short, short[::-1]]))
    _huffman(glc, cuda, np.stack([long_, long_[::-1]]))
    _huffman(glc, cuda, np.stack([short, long_, short[::-1]]))           # the decision is per block


# ---- sub-block histograms --------------------------------------------------------------------------------------------
def _equal_subblocks(n, first):
    """sub-blocks of equal symbols, values 5 and 200 in turn (a ragged last one where n is no multiple of 4096)"""
    x = np.empty(n, dtype=np.uint8)
    for k, lo in enumerate(range(0, n, SUB)):
        x[lo:lo + SUB] = (5, 200)[(k + first) & 1]
    return x


def _cycling(n, m, seed):
    """words [p | a b1 b2], p = word number mod m, (a b1 b2) ascending with the word number, in shuffled order: the
    suffixes that start at a word's second byte sort by word and sit next to each other in the BWT, whose bytes there
    are the p's in turn -- MTF rank m - 1 for as long as the stretch lasts (n / 4 positions behind the first n / 4)"""
    nw = n // 4
    j = np.arange(nw)
    w = np.stack([j % m, 201 + j // 784 % 27, 228 + j // 28 % 28, 228 + j % 28], axis=1).astype(np.uint8)
    return w[np.random.default_rng(seed).permutation(nw)].reshape(-1)


@functools.lru_cache(maxsize=None)
def _hist_rows(n, rows):
    """rows in turn: cycling through 201 symbols (rank 200), through 6 (rank 5), equal sub-blocks, Zipf; no two alike"""
    z = _zipf_rows(n, rows // 4 + 1)
    x = np.empty((rows, n), dtype=np.uint8)
    for i in range(rows):
        kind = i & 3
        if kind < 2:
            x[i] = _cycling(n, (201, 6)[kind], seed=i)
        elif kind == 2:
            x[i] = _equal_subblocks(n, i >> 2)
            x[i, :4] = np.frombuffer(np.uint32(i).tobytes(), dtype=np.uint8)
        else:
            x[i] = z[i // 4]
    x.setflags(write=False)
    return x


def _peak(x, rank):
    """largest count of `rank` in a sub-block of the oracle's MTF output"""
    r = O.mtf(O.bwt(x)[0])
    return max(int(np.count_nonzero(r[lo:lo + SUB] == rank)) for lo in range(0, r.size, SUB))


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n", [16384, 12288, 4096, 5000])
def test_subhist_count_4096_in_either_half_huffman_stage(glc, cuda, n, rows):
    x = np.stack([_equal_subblocks(n, r + 1) for r in range(rows)])
    whole = {int(r[lo]) for r in x for lo in range(0, n - SUB + 1, SUB)}          # values of the whole sub-blocks: count 4096
    assert 200 in whole and (5 in whole or (n < 2 * SUB and rows == 1))
    _huffman(glc, cuda, x)


@pytest.mark.parametrize("n,rows", [(16384, 1), (16384, 3), (32768, 2), (12288, 2)])
def test_subhist_quarters_instance(glc, cuda, n, rows):
    """few chunks in the call: a wave per chunk, the four quarters' counters added up on the way out"""
    x = _hist_rows(n, 4)
    if n == 32768:
        assert _peak(x[0], 200) == 4096 and _peak(x[1], 5) == 4096, "whole sub-blocks of one rank: 4096 in a high and in a low half"
    _compress(glc, cuda, x[:rows])
    _compress(glc, cuda, np.stack([_equal_subblocks(n, r) for r in range(rows)]))


def test_subhist_full_instance(glc, cuda):
    n, rows = 16384, 520
    x = _hist_rows(n, rows)
    assert _peak(x[0], 200) >= 3800 and _peak(x[1], 5) >= 4000
    _compress(glc, cuda, x)


def test_subhist_full_instance_whole_sub_blocks_of_one_rank(glc, cuda):
    n, rows = 32768, 260
    x = _hist_rows(n, rows)
    assert _peak(x[0], 200) == 4096 and _peak(x[1], 5) == 4096
    _compress(glc, cuda, x, check=sorted(set(range(0, rows, 3)) | {1, rows - 1}))


def test_subhist_ragged_instance(glc, cuda):
    n, rows = 12288, 700
    x = _hist_rows(n, rows)
    assert _peak(x[0], 200) >= 2000 and _peak(x[1], 5) >= 2000
    _compress(glc, cuda, x, check=sorted(set(range(0, rows, 2)) | {rows - 1}))


# ---- chunk lists -----------------------------------------------------------------------------------------------------
def _mixed_chunk(rng, shift):
    """segment 0 of the backward walk is the chunk's last 1024 bytes, segment 3 its oldest"""
    c = rng.integers(0, 200, SUB, dtype=np.uint8)
    c[[3 + shift, 500, 1023]] = 250                   # only in the oldest 1024 bytes
    c[[2100 + shift, 3000]] = 251                     # first met in segment 1 ...
    c[[1500, 1024 + shift, 17]] = 251                 # ... and again in segments 2 and 3
    c[[4095 - shift, 3500]] = 252                     # in segment 0 ...
    c[[2500, 1600 + shift, 900]] = 252                # ... and again in every later one
    return c


def _all_in_last_1024(rng):
    c = rng.integers(0, 256, SUB, dtype=np.uint8)
    c[3072:3072 + 256] = rng.permutation(256).astype(np.uint8)
    return c


def test_chunk_lists_two_chunks(glc, cuda):
    import torch
    rng = np.random.default_rng(77)
    one = np.full(SUB, 9, dtype=np.uint8)
    mixed = [_mixed_chunk(rng, s) for s in range(4)]
    for c in mixed:
        assert 250 not in c[1024:] and 251 not in c[3072:] and 251 in c[2048:3072] and 252 in c[3072:]
    full = _all_in_last_1024(rng)
    assert np.unique(full[3072:]).size == 256
    blocks = [(mixed[0], mixed[1]), (one, mixed[2]), (mixed[3], one), (full, mixed[0]), (mixed[1], full), (one, full),
              (full, one), (one, np.full(SUB, 200, dtype=np.uint8))]
    n = 2 * SUB
    L = glc.lib()
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_MTF, n, rows=1) as plan:
        for i, pair in enumerate(blocks):
            x = np.concatenate(pair)
            want = O.mtf(x)
            d_in = torch.from_numpy(x).to(cuda)
            d_out = torch.full((n,), 0xA5, dtype=torch.uint8, device=cuda)
            assert d_in.data_ptr() % 16 == 0, "the aligned full-chunk arm is the one under test"
            assert L.cudppMoveToFrontTransform(plan.handle, d_in.data_ptr(), d_out.data_ptr(), n) == 0
            plan.synchronize()
            got = d_out.cpu().numpy()
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, "block %d: %d bytes differ, first at %d" % (i, bad.size, bad[0])


def test_chunk_lists_two_chunks_compress(glc, cuda):
    """the same chunk shapes behind a BWT do not survive it, so cudppCompress gets Zipf and text blocks of two chunks"""
    x = np.stack([datagen.zipf_bytes(2 * SUB, seed=3), datagen.text_bytes(2 * SUB, seed=4), datagen.log_bytes(2 * SUB, seed=5)])
    _compress(glc, cuda, x)
