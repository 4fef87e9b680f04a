"""The span form of the MTF kernels (rows of K consecutive chunks, a recency list and a start list per span of K chunks: K is
the library's GLC_MTF_SPAN, 2 or 4; with K = 1 every shape here takes the FULL form of single chunks) against the oracle.

The span form is taken when a call has more than 2048 chunks in all and n is a multiple of K x 4 x 4096, so every case is
many small blocks.  Four shapes take it with K = 2 -- one wave per block, two, a second workgroup with one wave, ten waves --
and the second and the fourth of them with K = 4 too (one wave, five waves); three shapes are multiples of 16384 that are no
multiple of 2 x 16384 and stay on rows of one chunk whatever K is.

A row that runs on into the next chunk starts it from its own state instead of a start list, and the list kernel ranks the
symbols of K chunks at once and stops reading older chunks once it has met all 256.  Next to the eleven kinds of
test_gpu_mtf_full_rows the inputs are therefore what only a carried state or a span's list can get wrong: previous
occurrences 4095 / 4096 / 4097 back, across every chunk boundary; symbols that occur only in the first, only in the last,
only in the even or only in the odd chunks of every four; all 256 symbols in the last bytes of every chunk (the list kernel
stops after one chunk) and one symbol missing throughout (it never stops early); fewer than 256 distinct symbols (short
lists); a run of one symbol across every chunk boundary.  Every comparison is exact."""
import functools

import numpy as np
import pytest

import datagen
import oracle_lib as O
from test_gpu_mtf_full_rows import KINDS as FULL_KINDS, _check_block, _mtf_block as _full_block, _spaced

pytestmark = pytest.mark.gpu

SPAN_SHAPES = [(32768, 260), (65536, 130), (163840, 52), (327680, 27)]
SINGLE_SHAPES = [(16384, 516), (49152, 172), (81920, 104)]
CHUNK = 4096
SPAN_KINDS = ["back4095", "back4096", "back4097", "first_only", "last_only", "even_only", "odd_only", "all_at_end",
              "missing_one", "few_symbols", "run_across"]
KINDS = FULL_KINDS + SPAN_KINDS


def _only_in(n, keep, rng):
    """six symbols that occur (often) in the chunks c with keep(c) and nowhere else"""
    x = rng.integers(0, 250, n, dtype=np.uint8)
    for c in range(n // CHUNK):
        if keep(c):
            at = rng.integers(0, CHUNK, 40) + c * CHUNK
            x[at] = 250 + (at % 6).astype(np.uint8)
            x[c * CHUNK] = 250                                         # ... also the chunk's first and last byte
            x[c * CHUNK + CHUNK - 1] = 255
    return x


def _span_block(kind, n, i):
    rng = np.random.default_rng(5000 + i)
    if kind.startswith("back"):
        return _spaced(n, int(kind[4:]), rng) + np.uint8(i & 255)      # (wraps: the structure does not change)
    if kind == "first_only":
        return _only_in(n, lambda c: c % 4 == 0, rng)
    if kind == "last_only":
        return _only_in(n, lambda c: c % 4 == 3, rng)
    if kind == "even_only":
        return _only_in(n, lambda c: c % 2 == 0, rng)
    if kind == "odd_only":
        return _only_in(n, lambda c: c % 2 == 1, rng)
    if kind == "all_at_end":
        x = rng.integers(0, 256, n, dtype=np.uint8)
        for c in range(n // CHUNK):
            x[(c + 1) * CHUNK - 256:(c + 1) * CHUNK] = rng.permutation(256).astype(np.uint8)
        return x
    if kind == "missing_one":
        x = rng.integers(0, 255, n, dtype=np.uint8)
        return x + (x >= (i & 255)).astype(np.uint8)                   # every value but i & 255
    if kind == "few_symbols":
        return rng.integers(0, 17, n, dtype=np.uint8) * np.uint8(15) + np.uint8(i & 255)
    assert kind == "run_across"
    x = rng.integers(0, 256, n, dtype=np.uint8)
    for e in range(CHUNK, n, CHUNK):
        x[e - 5:e + 6] = (e // CHUNK + i) & 255
    return x


@functools.lru_cache(maxsize=None)
def _mtf_case(n, nblk):
    """(input blocks, their MTF by the oracle): block i is of kind i mod 22, no two blocks alike"""
    zipf = datagen.zipf_bytes(n * (nblk // len(FULL_KINDS) + 1), seed=n + nblk)
    blocks = []
    for i in range(nblk):
        kind = KINDS[i % len(KINDS)]
        blocks.append(_full_block(kind, n, i, zipf) if kind in FULL_KINDS else _span_block(kind, n, i))
    x = np.stack(blocks)
    want = np.stack([O.mtf(x[i]) for i in range(nblk)])
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


def test_kinds_are_what_they_claim():
    """(no GPU needed, but the module is marked as a whole) the inputs hold the cases their names promise"""
    n = 32768
    x = _span_block("missing_one", n, 7)
    assert 7 not in x and np.unique(x).size == 255
    assert np.unique(_span_block("few_symbols", n, 3)).size == 17
    x = _span_block("all_at_end", n, 0)
    assert all(np.unique(x[c + CHUNK - 256:c + CHUNK]).size == 256 for c in range(0, n, CHUNK))
    x = _span_block("first_only", n, 1)
    assert all((x[c * CHUNK:(c + 1) * CHUNK] >= 250).any() == (c % 4 == 0) for c in range(n // CHUNK))
    x = _span_block("back4096", n, 0)
    at = np.flatnonzero(x == 200)
    assert at.size > 1 and np.all(np.diff(at) == 4096)
    x = _span_block("run_across", n, 0)
    assert np.all(x[CHUNK - 5:CHUNK + 6] == 1)
    assert len(KINDS) == 22 and len(KINDS) <= min(nblk for _, nblk in SPAN_SHAPES + SINGLE_SHAPES)


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("n,nblk", SPAN_SHAPES + SINGLE_SHAPES)
def test_mtf_batch_equals_oracle(glc, cuda, n, nblk, off):
    import torch
    x, want = _mtf_case(n, nblk)
    d_in = torch.zeros(n * nblk + off, dtype=torch.uint8, device=cuda)
    d_in[off:] = torch.from_numpy(x.reshape(-1).copy()).to(cuda)
    d_out = torch.full((n * nblk + off + 64,), 0xA5, dtype=torch.uint8, device=cuda)
    assert (d_in.data_ptr() + off) % 16 == off and (d_out.data_ptr() + off) % 16 == off
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_MTF, n, rows=nblk) as plan:
        assert glc.lib().glcMtfBatch(plan.handle, d_in.data_ptr() + off, d_out.data_ptr() + off, n, nblk) == 0
        plan.synchronize()
    got = d_out.cpu().numpy()
    assert np.all(got[:off] == 0xA5) and np.all(got[off + n * nblk:] == 0xA5), "wrote outside the output"
    got = got[off:off + n * nblk].reshape(nblk, n)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, "n %d: %d blocks differ, first block %d (%s) at byte %d" % (
        n, bad.size, bad[0], KINDS[bad[0] % len(KINDS)], int(np.flatnonzero(got[bad[0]] != want[bad[0]])[0]))


@pytest.mark.parametrize("n,nblk", SPAN_SHAPES)
def test_compress_batch_histogram_instance(glc, cuda, n, nblk):
    """Zipf and uniform blocks in turn; every fifth block (both kinds) and the last two against the oracle -- histogram, the
    offsets of the sub-blocks (they come from the per-chunk histograms a row hands over at every chunk's end), size and
    stream words --, every block decoded back"""
    import torch
    x = np.random.default_rng(n).integers(0, 256, (nblk, n), dtype=np.uint8)
    x[0::2] = datagen.zipf_bytes(n * ((nblk + 1) // 2), seed=7 * n + nblk).reshape((nblk + 1) // 2, n)
    d = torch.from_numpy(x.reshape(-1).copy()).to(cuda)
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=nblk) as plan:
        out = glc.compress_batch(plan, d, n, nblk)
        plan.synchronize()
        for k in sorted(set(range(0, nblk, 5)) | {nblk - 2, nblk - 1}):
            _check_block(out, k, x[k], "%d x %d block %d" % (n, nblk, k))
        back = glc.decompress_batch(plan, out, n, nblk)
        assert torch.equal(back, d)


def test_compress_batch_zeros_instance(glc, cuda):
    """log-like blocks come back from the bucket sorter, and their MTF is redone under the mask with rank 0 counted by ballot:
    two waves' worth of spans of four per block"""
    import torch
    n, nblk = 131072, 65
    base = [datagen.log_bytes(n, seed=700 + s) for s in range(4)]
    x = np.stack([base[i % 4] for i in range(nblk)])
    for i in range(nblk):
        x[i, 100:108] = np.frombuffer(b"%08d" % i, dtype=np.uint8)          # no two blocks alike
    d = torch.from_numpy(x.reshape(-1).copy()).to(cuda)
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=nblk) as plan:
        out = glc.compress_batch(plan, d, n, nblk)
        plan.synchronize()
        assert plan.last_sort_stats()[0] > 0, "no block was handed on by the bucket sorter: the masked redo did not run"
        for k in range(0, nblk, 2):
            _check_block(out, k, x[k], "log block %d" % k)
        back = glc.decompress_batch(plan, out, n, nblk)
        assert torch.equal(back, d)
