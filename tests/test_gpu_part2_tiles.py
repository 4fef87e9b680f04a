"""k_fs_part2's two tile bodies (bwt_bucket.hip): an inner tile runs without per-suffix guards, the first and the last tile
of a block with them.  Block lengths on every edge shape of an 8192-suffix tile (the batch form of 16 blocks or more) and of
a 4096-suffix one (15 blocks), each block's BWT and index checked bit-exactly against the oracle."""
import numpy as np
import pytest

import datagen
import oracle_lib as O

pytestmark = pytest.mark.gpu
TILE = 8192


def _bwt(glc, plan, torch, x, n, rows):
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.zeros(x.size, dtype=torch.uint8, device=d_in.device)
    d_idx = torch.zeros(rows, dtype=torch.int32, device=d_in.device)
    assert glc.lib().glcBwtBatch(plan.handle, d_in.data_ptr(), d_out.data_ptr(), d_idx.data_ptr(), n, rows) == 0
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_idx.cpu().numpy()


def _blocks(kind, n, rows, seed):
    rng = np.random.default_rng(seed)
    if kind == "zipf":
        return [datagen.zipf_bytes(n, seed=seed + i) for i in range(rows)]
    if kind == "uniform":
        return [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(rows)]
    # few symbols: four byte values, i.i.d.
    return [rng.choice(np.array([3, 70, 71, 200], dtype=np.uint8), n) for _ in range(rows)]


def _check(glc, ctx, cuda, kind, n, rows, seed):
    import torch
    blocks = _blocks(kind, n, rows, seed)
    with glc.Plan(ctx, glc.CUDPP_BWT, n, rows=rows) as plan:
        got, gidx = _bwt(glc, plan, torch, np.concatenate(blocks), n, rows)
    for i, blk in enumerate(blocks):
        want, widx = O.bwt(blk)
        assert int(gidx[i]) == widx, "%s n=%d rows=%d block %d: index" % (kind, n, rows, i)
        assert np.array_equal(got[i * n:(i + 1) * n], want), "%s n=%d rows=%d block %d: BWT" % (kind, n, rows, i)


@pytest.fixture(scope="module")
def ctx(glc, cuda):
    c = glc.Cudpp()
    yield c
    c.close()


# 8192 k + r: r = 0 (the last tile full, 16 bytes behind it past the end), 1, 15, 16, 17 (the first n whose second-last tile
# is inner), 8191; k = 3 puts an inner tile between the first and the last
@pytest.mark.parametrize("r", [0, 1, 15, 16, 17, 8191])
@pytest.mark.parametrize("kind", ["zipf", "uniform", "few"])
def test_tile_edges(glc, ctx, cuda, kind, r):
    _check(glc, ctx, cuda, kind, 3 * TILE + r, 16, 1000 + r)


@pytest.mark.parametrize("n", [TILE - 192, TILE + 15, 2 * TILE + 16])
def test_block_of_one_or_two_tiles(glc, ctx, cuda, n):
    """a block shorter than 8192 + 16 is its first and its last tile at once; 2 * 8192 + 16 ends exactly one tile's
    look-ahead past an edge"""
    _check(glc, ctx, cuda, "zipf", n, 16, 2000 + n)


@pytest.mark.parametrize("kind", ["zipf", "uniform", "few"])
def test_full_blocks(glc, ctx, cuda, kind):
    _check(glc, ctx, cuda, kind, 1 << 20, 16, 3000)


@pytest.mark.parametrize("n", [1 << 20, 5 * TILE + 17, TILE + 1])
def test_fifteen_blocks(glc, ctx, cuda, n):
    """fewer than 16 blocks: the 512-thread form with 4096-suffix tiles"""
    _check(glc, ctx, cuda, "zipf", n, 15, 4000 + n)
