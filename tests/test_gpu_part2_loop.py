"""k_fs_part2's tile loop (bwt_bucket.hip): a workgroup takes 16 consecutive tiles of 8192 suffixes (the batch form of 16
blocks or more) as at most one edge tile, a run of inner tiles that is a loop of its own -- a tile's stores and the next
tile's text are in flight across its back edge -- and one or two edge tiles.  Block lengths that put every such sequence
into one workgroup, a block flagged in the middle of a run, two calls back to back on one plan, and the 512-thread form
(4096-suffix tiles, four or one per workgroup); each block's BWT and index checked bit-exactly against the oracle."""
import numpy as np
import pytest

import datagen
import oracle_lib as O

pytestmark = pytest.mark.gpu
TILE = 8192


def _blocks(kind, n, rows, seed):
    rng = np.random.default_rng(seed)
    if kind == "zipf":
        return [datagen.zipf_bytes(n, seed=seed + i) for i in range(rows)]
    if kind == "uniform":
        return [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(rows)]
    # few symbols: four byte values, i.i.d.
    return [rng.choice(np.array([3, 70, 71, 200], dtype=np.uint8), n) for _ in range(rows)]


def _launch(glc, plan, torch, blocks, n):
    """one glcBwtBatch call, NOT synchronised: (output, indices) still on the device"""
    rows = len(blocks)
    d_in = torch.from_numpy(np.ascontiguousarray(np.concatenate(blocks))).cuda()
    d_out = torch.zeros(rows * n, dtype=torch.uint8, device=d_in.device)
    d_idx = torch.zeros(rows, dtype=torch.int32, device=d_in.device)
    assert glc.lib().glcBwtBatch(plan.handle, d_in.data_ptr(), d_out.data_ptr(), d_idx.data_ptr(), n, rows) == 0
    return d_in, d_out, d_idx


def _exact(blocks, n, got, gidx, what):
    for i, blk in enumerate(blocks):
        want, widx = O.bwt(blk)
        assert int(gidx[i]) == widx, "%s n=%d rows=%d block %d: index" % (what, n, len(blocks), i)
        assert np.array_equal(got[i * n:(i + 1) * n], want), "%s n=%d rows=%d block %d: BWT" % (what, n, len(blocks), i)


def _check(glc, ctx, kind, n, rows, seed):
    import torch
    blocks = _blocks(kind, n, rows, seed)
    with glc.Plan(ctx, glc.CUDPP_BWT, n, rows=rows) as plan:
        _, d_out, d_idx = _launch(glc, plan, torch, blocks, n)
        torch.cuda.synchronize()
        stats = plan.last_sort_stats()
    _exact(blocks, n, d_out.cpu().numpy(), d_idx.cpu().numpy(), kind)
    return stats


@pytest.fixture(scope="module")
def ctx(glc, cuda):
    c = glc.Cudpp()
    yield c
    c.close()


# tiles of a block of k 8192 + 17 bytes: 0 (edge), 1 .. k - 1 (inner), k (edge, 17 suffixes)
#   k = 4   one workgroup: the first edge tile, three inner tiles, the last edge tile -- stores and a prefetch pending across
#           two boundaries between inner tiles
#   k = 19  the second workgroup (tiles 16 .. 19) starts on an inner tile and ends on the block's last tile
#   k = 33  the second workgroup (tiles 16 .. 31) is inner tiles only, the third is the one edge tile 33 behind inner tile 32
@pytest.mark.parametrize("k", [4, 19, 33])
@pytest.mark.parametrize("kind", ["zipf", "uniform", "few"])
def test_runs_of_inner_tiles(glc, ctx, cuda, kind, k):
    _check(glc, ctx, kind, k * TILE + 17, 16, 5000 + k)


def test_block_flagged_inside_a_run(glc, ctx, cuda):
    """12 KiB of one byte value from offset 5 * 8192 in blocks 3 and 11: the suffixes of the run share one code, their bucket
    passes 4032 words in tile 5, and the workgroup leaves in the middle of its run of inner tiles with the text of tile 6 and
    its atomics in flight.  (Blocks of 8 * 8192 + 17 bytes: neither of the two starts on a 16-byte boundary, so the histogram
    pass's text probe has not looked at them.)  Exactly those two blocks go on to the sample sorter; all 16 are exact."""
    import torch
    n, rows = 8 * TILE + 17, 16
    blocks = _blocks("zipf", n, rows, 6000)
    for i in (3, 11):
        blocks[i] = blocks[i].copy()
        blocks[i][5 * TILE:5 * TILE + 12288] = 0x41
    with glc.Plan(ctx, glc.CUDPP_BWT, n, rows=rows) as plan:
        _, d_out, d_idx = _launch(glc, plan, torch, blocks, n)
        torch.cuda.synchronize()
        assert plan.last_sort_stats()[0] == 2, plan.last_sort_stats()
    _exact(blocks, n, d_out.cpu().numpy(), d_idx.cpu().numpy(), "zipf with a run")


def test_two_calls_back_to_back(glc, ctx, cuda):
    """two different inputs through one plan with no synchronise in between: the second call's result"""
    import torch
    n, rows = 4 * TILE + 17, 16
    first, second = _blocks("zipf", n, rows, 7000), _blocks("zipf", n, rows, 7100)
    with glc.Plan(ctx, glc.CUDPP_BWT, n, rows=rows) as plan:
        keep = _launch(glc, plan, torch, first, n)
        _, d_out, d_idx = _launch(glc, plan, torch, second, n)
        torch.cuda.synchronize()
    del keep
    _exact(second, n, d_out.cpu().numpy(), d_idx.cpu().numpy(), "second call")


@pytest.mark.parametrize("rows", [15, 3])
def test_512_thread_form(glc, ctx, cuda, rows):
    """fewer than 16 blocks: 4096-suffix tiles, four per workgroup (15 blocks) or one (3 blocks); 9 * 4096 + 17 bytes are the
    first edge tile, eight inner tiles and the last edge tile"""
    _check(glc, ctx, "zipf", 9 * 4096 + 17, rows, 8000 + rows)
