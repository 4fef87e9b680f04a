"""Chain groups of the doubling rounds (csrc/bwt_sa.hip, k_chain_*): a group whose members are an arithmetic progression
i_0, i_0 + d, ... over d-periodic text is ONE monotone chain -- ascending or descending by position, decided where its last two
members differ -- and gets its final order in one round instead of log2(stretch / depth) doubling rounds.  Blocks that only the
general sorter takes (two or more periodic regions, a periodic stretch inside ordinary data, a run of one byte, either direction
of the exit), BWT + index against the oracle (the suffix array of a block is unique: sa_app.cu:125-298 + compress_kernel.cuh:55-74),
with the periodic tier on and off.  Each call also reports what the rule did (glcPlanLastSortChains): chain groups taken
where periodic stretches reach the doubling rounds, candidates refused where progressions are not chains.  The suffix arrays
themselves, which the BWT hides inside a chain: tests/test_gpu_chains_sa.py."""
import numpy as np
import pytest

import chain_corpus as CC
import oracle_lib as O

pytestmark = pytest.mark.gpu


def _bwt_batch(glc, cuda, blocks, n, mode=0):
    import torch
    L = glc.lib()
    nb = len(blocks)
    d_in = torch.from_numpy(np.concatenate(blocks)).to(cuda)
    d_out = torch.zeros_like(d_in)
    d_idx = torch.full((nb,), -1, dtype=torch.int32, device=cuda)
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_BWT, n, rows=nb) as plan:
        plan.set_sorter(mode)
        assert L.glcBwtBatch(plan.handle, d_in.data_ptr(), d_out.data_ptr(), d_idx.data_ptr(), n, nb) == 0
        plan.synchronize()
        return (d_out.cpu().numpy().reshape(nb, n), d_idx.cpu().numpy(), plan.last_sort_stats(), plan.last_sort_periodic(),
                plan.last_sort_chains())


def _check(glc, cuda, blocks, n, what, modes=(0, 7)):
    """BWT + index of every block against the oracle with the periodic tier on (0) and off (7); returns the chain tallies
    (taken, refused) of every call by sorter mode"""
    wants = [O.bwt(x) for x in blocks]
    tallies = {}
    for mode in modes:                                        # the periodic tier on / off: what it leaves (or everything) is the general sorter's
        got, idx, (f1, f2), nper, tallies[mode] = _bwt_batch(glc, cuda, blocks, n, mode)
        for k, x in enumerate(blocks):
            want, widx = wants[k]
            assert int(idx[k]) == widx, (what, mode, k)
            assert np.array_equal(got[k], want), (what, mode, k, int(np.nonzero(got[k] != want)[0][0]))
    return tallies


@pytest.mark.parametrize("seed", range(4))
def test_two_and_more_periodic_regions(glc, cuda, seed):
    n = 1 << 17
    tallies = _check(glc, cuda, CC.region_blocks(seed, n), n, "regions")
    assert tallies[7][0] > 0, tallies                        # (periodic tier off: every block reaches the doubling rounds)


def test_periodic_stretches_and_runs_inside_ordinary_data(glc, cuda):
    n = 1 << 18
    tallies = _check(glc, cuda, CC.stretch_blocks(n), n, "stretches")
    assert tallies[0][0] > 0 and tallies[7][0] > 0, tallies


def test_either_direction_of_the_chain(glc, cuda):
    """the symbol behind the stretch smaller / larger than the one the period would continue with; the stretch ending the block"""
    n = 1 << 17
    tallies = _check(glc, cuda, CC.direction_blocks(n), n, "direction")
    assert tallies[7][0] > 0, tallies


def test_full_size_blocks_of_the_bench(glc, cuda):
    """bench.py's two_regions kinds at 1 MiB: two periodic halves, a 256 KiB stretch inside Zipf data"""
    n = 1 << 20
    h, z = CC.full_size_blocks(n)
    got, idx, (f1, f2), nper, (taken, refused) = _bwt_batch(glc, cuda, [h, z], n, 0)
    for k, x in enumerate((h, z)):
        want, widx = O.bwt(x)
        assert int(idx[k]) == widx and np.array_equal(got[k], want), k
    assert taken > 0, (taken, refused)


def test_progressions_that_are_not_chains(glc, cuda):
    """groups whose members ARE an arithmetic progression with a stride the chain pass tries (<= 4096) but whose text is not periodic
    over it: a 600-byte phrase every 2048 bytes with different random bytes in between; a periodic stretch with ONE byte changed in
    its middle (every residue class still has a member every d bytes across the defect); two stretches of one pattern a whole number
    of periods apart.  The verification must refuse them (plain doubling orders them) -- the bytes are the oracle's either way;
    also through the general sorter alone (1)."""
    n = 1 << 17
    tallies = _check(glc, cuda, CC.not_chain_blocks(n), n, "not chains", modes=(0, 7, 1))
    assert all(t[0] == 0 for t in tallies.values()), tallies   # (tests/chain_model.py: none of the three holds a chain, from any depth)
    assert tallies[1][1] > 0, tallies                           # the general sorter alone: the verification refused candidates


@pytest.mark.gpu_long
@pytest.mark.parametrize("seed", range(int(__import__("os").environ.get("GLC_MOSAIC_SEEDS", "6"))))
def test_random_mosaics_of_periodic_pieces(glc, cuda, seed):
    """blocks glued from random pieces -- periodic stretches of random period and alphabet, runs, random bytes, copies of earlier
    pieces -- through the general sorter alone (mode 1), the tiers' own choice (0) and with the periodic tier off (7)"""
    n, blocks = CC.large_mosaic_blocks(seed)
    for mode in (1, 0, 7):
        got, idx, _, _, _ = _bwt_batch(glc, cuda, blocks, n, mode)
        for k, x in enumerate(blocks):
            want, widx = O.bwt(x)
            assert int(idx[k]) == widx, (seed, mode, k)
            assert np.array_equal(got[k], want), (seed, mode, k, int(np.nonzero(got[k] != want)[0][0]))
