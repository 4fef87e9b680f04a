"""k_mtf_encode's FULL form (every row of every wave a whole 4096-byte chunk: n a multiple of 4 x 4096) against the oracle.

The FULL form is launched only when a call has more than 2048 chunks in all (below that the rows of a wave are the quarters
of one chunk), so every case is many small blocks.  Three shapes take it -- one full wave per block, one full workgroup, a
second workgroup with one wave -- and three shapes next to them (one byte short, one byte over, a whole number of chunks
that is no multiple of four) must take the ragged form.

glcMtfBatch runs the instance without a histogram on exactly the bytes given, so its inputs are built for what fixed trip
counts, the unroll by four and the immediate offsets can get wrong: the previous occurrence of a symbol in the same batch
of 16, exactly one batch back, or straddling two (periods 15 / 16 / 17); across the re-base at every 1024-byte segment
boundary and in the batch that ends a segment (occurrences 1023 / 1024 / 1025 apart); in the first and the last batch of
a chunk only; always (one byte value: rank 0) and never within 256 positions (the cycle 0..255: rank 255, every
timestamp killed through the bitmap); with 16-byte-aligned and with odd input / output pointers.
glcCompressBatch runs the two instances with the histogram: Zipf and uniform blocks the plain one, log-like blocks that
the bucket sorter hands on the one that counts rank 0 with a ballot, there under a mask of the blocks to redo."""
import functools

import numpy as np
import pytest

import datagen
import oracle_lib as O

pytestmark = pytest.mark.gpu

FULL_SHAPES = [(16384, 516), (65536, 130), (81920, 104)]
RAGGED_SHAPES = [(16383, 516), (16385, 412), (28672, 300)]
CHUNK = 4096


def _spaced(n, d, rng):
    """six symbols that recur every d positions from different phases, over a background that never holds them"""
    x = rng.integers(0, 200, n, dtype=np.uint8)
    for k, phase in enumerate((0, 7, 15, 16, 1008, 1023)):
        x[phase::d] = 200 + k
    return x


def _ends_only(n, rng):
    """two symbols that occur in the first and in the last batch of every chunk and nowhere else"""
    x = rng.integers(0, 250, n, dtype=np.uint8)
    for c in range(0, n, CHUNK):
        for pos, sym in ((2, 255), (15, 254), (4080, 254), (4090, 255)):
            if c + pos < n:
                x[c + pos] = sym
    return x


KINDS = ["zipf", "uniform", "one_value", "cycle256", "period15", "period16", "period17", "apart1023", "apart1024",
         "apart1025", "ends_only"]


def _mtf_block(kind, n, i, zipf):
    rng = np.random.default_rng(1000 + i)
    pos = np.arange(n)
    if kind == "zipf":
        return zipf[(i // len(KINDS)) * n:(i // len(KINDS) + 1) * n]
    if kind == "uniform":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "one_value":
        return np.full(n, i & 255, dtype=np.uint8)
    if kind == "cycle256":
        return ((pos + i) & 255).astype(np.uint8)
    if kind.startswith("period"):
        return (((pos % int(kind[6:])) * 7 + i) & 255).astype(np.uint8)
    if kind.startswith("apart"):
        return _spaced(n, int(kind[5:]), rng) + np.uint8(i & 255)          # (wraps: the structure does not change)
    return _ends_only(n, rng) + np.uint8(i & 255)


@functools.lru_cache(maxsize=None)
def _mtf_case(n, nblk):
    """(input blocks, their MTF by the oracle): block i is of kind i mod 11, no two blocks alike"""
    zipf = datagen.zipf_bytes(n * (nblk // len(KINDS) + 1), seed=n + nblk)
    x = np.stack([_mtf_block(KINDS[i % len(KINDS)], n, i, zipf) for i in range(nblk)])
    want = np.stack([O.mtf(x[i]) for i in range(nblk)])
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("n,nblk", FULL_SHAPES + RAGGED_SHAPES)
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


def _check_block(out, k, x, what):
    want = O.compress(x)
    assert want["rc"] == 0
    nsub, stride = out["nsub"], out["stride"]
    assert int(out["bwt_index"][k].item()) == want["bwt_index"], what + ": BWT index"
    assert np.array_equal(out["hist"][256 * k: 256 * k + 256].cpu().numpy().view(np.uint32), want["hist"]), what + ": histogram"
    assert np.array_equal(out["offsets"][nsub * k: nsub * (k + 1)].cpu().numpy().view(np.uint32), want["offsets"]), what + ": offsets"
    size = int(out["size"][k].item())
    assert size == want["size"], what + ": size"
    got = out["words"][stride * k: stride * k + size].cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want["words"]), what + ": stream words"


@pytest.mark.parametrize("n,nblk", [(16384, 516), (65536, 130)])
def test_compress_batch_histogram_instance(glc, cuda, n, nblk):
    """Zipf and uniform blocks in turn; every third block (both kinds) and the last two against the oracle, every block decoded back"""
    import torch
    x = np.random.default_rng(n).integers(0, 256, (nblk, n), dtype=np.uint8)
    x[0::2] = datagen.zipf_bytes(n * (nblk // 2), seed=7 * n + nblk).reshape(nblk // 2, n)
    d = torch.from_numpy(x.reshape(-1).copy()).to(cuda)
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=nblk) as plan:
        out = glc.compress_batch(plan, d, n, nblk)
        plan.synchronize()
        for k in sorted(set(range(0, nblk, 3)) | {nblk - 2, nblk - 1}):
            _check_block(out, k, x[k], "%d x %d block %d" % (n, nblk, k))
        back = glc.decompress_batch(plan, out, n, nblk)
        assert torch.equal(back, d)


def test_compress_batch_zeros_instance(glc, cuda):
    """log-like blocks come back from the bucket sorter, and their MTF is redone under the mask with rank 0 counted by ballot"""
    import torch
    n, nblk = 65536, 130
    base = [datagen.log_bytes(n, seed=900 + s) for s in range(4)]
    x = np.stack([base[i % 4] for i in range(nblk)])
    for i in range(nblk):
        x[i, 100:108] = np.frombuffer(b"%08d" % i, dtype=np.uint8)          # no two blocks alike
    d = torch.from_numpy(x.reshape(-1).copy()).to(cuda)
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=nblk) as plan:
        out = glc.compress_batch(plan, d, n, nblk)
        plan.synchronize()
        assert plan.last_sort_stats()[0] > 0, "no block was handed on by the bucket sorter: the masked redo did not run"
        for k in range(nblk):
            _check_block(out, k, x[k], "log block %d" % k)
        back = glc.decompress_batch(plan, out, n, nblk)
        assert torch.equal(back, d)
