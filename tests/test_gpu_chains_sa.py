"""Chain groups of the general sorter's doubling rounds (csrc/bwt_sa.hip, k_chain_*) at the SUFFIX-ARRAY level.  Inside a
periodic stretch every member of a chain group has the same preceding symbol, so any order of a group's members -- the reverse
included -- gives the same BWT bytes; cudppSuffixArray returns the order itself and runs the same chain kernels.  Every result
is compared with the oracle's suffix array (tests/oracle_lib.py); where a single block is sorted by the general sorter alone
(sorters 1 and 2) the chain tallies of the call (glcPlanLastSortChains) must equal those of the CPU model of the rule
(tests/chain_model.py) exactly: candidates formed, chains taken, candidates refused."""
import hashlib
import os
import re

import numpy as np
import pytest

import chain_corpus as CC
import chain_model as M
import oracle_lib as O

pytestmark = pytest.mark.gpu

_SA, _BWT, _MODEL = {}, {}, {}


def _key(x):
    return hashlib.sha1(np.ascontiguousarray(x).tobytes()).hexdigest()


def _oracle_sa(x):
    k = _key(x)
    if k not in _SA:
        _SA[k] = O.suffix_array(x)
    return _SA[k]


def _oracle_bwt(x):
    k = _key(x)
    if k not in _BWT:
        _BWT[k] = O.bwt(x)
    return _BWT[k]


def _model(x, start, sched):
    k = (_key(x), start, sched)
    if k not in _MODEL:
        r = M.model_sa(x, *sched, start=start)
        _MODEL[k] = (r.taken, r.refused)
    return _MODEL[k]


START = {1: "text", 2: "isa"}                                  # sorter mode -> where the model's doubling starts


@pytest.fixture(scope="module")
def ctx(glc):
    with glc.Cudpp() as c:
        yield c


def _sa(glc, plan, x):
    """cudppSuffixArray of one block: (suffix array, chain tallies of the call); out[0] must be n"""
    import torch
    n = x.size
    d_in = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_out = torch.zeros(n + 1, dtype=torch.int32, device=d_in.device)
    assert glc.lib().cudppSuffixArray(plan.handle, d_in.data_ptr(), d_out.data_ptr(), n) == glc.CUDPP_SUCCESS
    got = d_out.cpu().numpy().view(np.uint32)
    assert got[0] == n
    return got[1:], plan.last_sort_chains()


def _check_sa(glc, plan, x, what, mode=None, sched=None):
    got, tally = _sa(glc, plan, x)
    want = _oracle_sa(x)
    if not np.array_equal(got, want):
        bad = np.nonzero(got != want)[0]
        raise AssertionError("%s: suffix array differs at %d of %d rows (first %d: got %d, want %d)" % (
            what, bad.size, x.size, bad[0], got[bad[0]], want[bad[0]]))
    if mode in START and sched is not None:
        assert tally == _model(x, START[mode], sched), (what, mode, tally, _model(x, START[mode], sched))
    return tally


def _bwt_batch(glc, blocks, n, mode, chains=None):
    import torch
    nb = len(blocks)
    d_in = torch.from_numpy(np.concatenate(blocks)).cuda()
    d_out = torch.zeros_like(d_in)
    d_idx = torch.full((nb,), -1, dtype=torch.int32, device=d_in.device)
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_BWT, n, rows=nb) as plan:
        plan.set_sorter(mode)
        if chains:
            plan.set_chains(*chains)
        assert glc.lib().glcBwtBatch(plan.handle, d_in.data_ptr(), d_out.data_ptr(), d_idx.data_ptr(), n, nb) == 0
        plan.synchronize()
        return (d_out.cpu().numpy().reshape(nb, n), d_idx.cpu().numpy(), plan.last_sort_periodic(), plan.last_sort_chains())


# ---------------------------------------------------------------------------------------------------------------------------
# the chain corpora of test_gpu_chains.py through cudppSuffixArray
# ---------------------------------------------------------------------------------------------------------------------------
DEFAULT = (M.CHAIN_MIN, M.CHAIN_ROUNDS)
CHAIN_CORPORA = [("regions%d" % k, x) for k, x in enumerate(CC.region_blocks(0))] + \
                [("stretch%d" % k, x) for k, x in enumerate(CC.stretch_blocks())] + \
                [("direction%d" % k, x) for k, x in enumerate(CC.direction_blocks())]


@pytest.mark.parametrize("mode", [0, 1, 2, 5, 6])
def test_chain_corpora_suffix_arrays(glc, ctx, mode):
    """regions, stretches inside data, both directions: exact suffix arrays, chains taken in every block (a suffix-array call
    never goes to the periodic tier: every one of these deep blocks reaches the doubling rounds)"""
    with glc.Plan(ctx, glc.CUDPP_SA, 1 << 18) as plan:
        plan.set_sorter(mode)
        for what, x in CHAIN_CORPORA:
            taken, refused = _check_sa(glc, plan, x, what, mode, DEFAULT if x.size <= (1 << 17) else None)
            assert taken > 0, (what, mode, taken, refused)


def test_full_size_blocks_suffix_arrays(glc, ctx):
    with glc.Plan(ctx, glc.CUDPP_SA, 1 << 20) as plan:
        for mode in (0, 1):
            plan.set_sorter(mode)
            for k, x in enumerate(CC.full_size_blocks()):
                taken, refused = _check_sa(glc, plan, x, "full%d" % k)
                assert taken > 0, (k, mode, taken, refused)


@pytest.mark.parametrize("mode", [0, 1, 2, 5, 6])
def test_progressions_that_are_not_chains_suffix_arrays(glc, ctx, mode):
    """a phrase every 2048 bytes, a periodic stretch with one byte changed, two stretches of one pattern far apart: nothing is
    taken, whichever tier and depth the doubling starts from; with the general sorter alone the phrase's progressions are
    candidates the verification refuses (the model: 596 of them), the defect's too (21)"""
    with glc.Plan(ctx, glc.CUDPP_SA, 1 << 17) as plan:
        plan.set_sorter(mode)
        for k, x in enumerate(CC.not_chain_blocks()):
            taken, refused = _check_sa(glc, plan, x, "not-chain%d" % k, mode, DEFAULT)
            assert taken == 0, (k, mode, taken, refused)
            if k <= 1 and mode in START:
                assert refused > 0, (k, mode, taken, refused)


# ---------------------------------------------------------------------------------------------------------------------------
# edges the kernels branch on, with a chain attempt in every round
# ---------------------------------------------------------------------------------------------------------------------------
EVERY = (1, M.ALL_ROUNDS)


def _edge_blocks():
    out = []
    for d in (1, 2, 15, 16, 17, 4095, 4096, 4097):
        n = max(16381, 3 * d + 2000)
        out.append(("d=%d to the end" % d, CC.stride_block(d, n, d), d <= 4096))
        out.append(("d=%d from 0" % d, CC.stride_block(d, n + 10, d + 1, ahead=0, tail=b"\x00\x01\x02"), d <= 4096))
        out.append(("d=%d defect last" % d, CC.stride_block(d, n + 3, d + 2, defect=1), d <= 4096))
        out.append(("d=%d defect second to last" % d, CC.stride_block(d, n + 7, d + 3, defect=2), d <= 4096))
    for copies in (2, 3):                                      # groups of L = 2 and 3 members (the u check needs L >= 3)
        for d in (64, 333, 4096):
            out.append(("%d copies of %d" % (copies, d), CC.repeats_block(16389, copies * 7 + d, copies, d), True))
    out.append(("16384 periodic", np.resize(np.frombuffer(b"abcab", dtype=np.uint8), 16384).copy(), True))
    return out


@pytest.mark.parametrize("mode", [1, 2])
def test_strides_lengths_and_ends(glc, ctx, mode):
    """strides 1 .. 4097 (nothing taken past CHAIN_DMAX = 4096), stretches that end at n (the direction walk runs off the
    block) or start at 0, defects in the last or second-to-last period, L = 2 / 3 groups, lengths around 16 K that are not
    multiples of 16; tallies equal the model's"""
    with glc.Plan(ctx, glc.CUDPP_SA, 20000) as plan:
        plan.set_sorter(mode)
        plan.set_chains(*EVERY)
        for what, x, chains in _edge_blocks():
            taken, refused = _check_sa(glc, plan, x, what, mode, EVERY)
            assert (taken > 0) == chains, (what, taken, refused)


def test_near_one_mib(glc, ctx):
    """a block of 2^20 - 3 bytes with a 17-periodic stretch up to its end and a run: chains taken.  One with a 4096-periodic
    stretch whose second-to-last period holds a defect: every residue class keeps a member past the defect until the depth
    passes it, and by then less than half of the block is live (no attempt past round 0): candidates refused, nothing taken.
    Tallies equal the model's with either schedule"""
    n = (1 << 20) - 3
    x = CC.stride_block(17, n, 5, ahead=400000)
    x[100000:160000] = 9
    y = CC.stride_block(4096, n, 6, ahead=600000, defect=2)
    scheds = (EVERY, DEFAULT)
    with glc.Plan(ctx, glc.CUDPP_SA, 1 << 20) as plan:
        plan.set_sorter(1)
        for what, b, chains in (("17 to the end", x, True), ("4096 with a defect", y, False)):
            model = [(r.taken, r.refused) for r in M.model_schedules(b, scheds)]
            for sched, want in zip(scheds, model):
                plan.set_chains(*sched)
                tally = _check_sa(glc, plan, b, what)
                assert tally == want, (what, sched, tally, want)
                assert (tally[0] > 0) == chains and (chains or tally[1] > 0), (what, sched, tally)


# ---------------------------------------------------------------------------------------------------------------------------
# the forced-attempt sweep: corpus mosaics and the model's adversarial blocks
# ---------------------------------------------------------------------------------------------------------------------------
SWEEP_N = (300, 1000, 4096, 4099, 16389, 65536)


def test_adversarial_blocks_suffix_arrays(glc, ctx):
    """the blocks on which a mutant of the rule is wrong (chain_model.ADVERSARIAL): exact, with the model's tallies"""
    with glc.Plan(ctx, glc.CUDPP_SA, 4096) as plan:
        for mode in (1, 2):
            plan.set_sorter(mode)
            plan.set_chains(*EVERY)
            for seed, x in M.adversarial_blocks():
                taken, refused = _check_sa(glc, plan, x, "adversarial seed %d" % seed, mode, EVERY)
                if mode == 1:
                    assert taken > 0, seed


def _mosaic_set(n, count, base):
    return [M.mosaic(base + k, n) for k in range(count)]


def test_forced_attempts_suffix_arrays(glc, ctx):
    """one block per call, every round allowed, sorters 1 and 2: corpus mosaics from a few hundred bytes to 64 KiB"""
    total = [0, 0]
    with glc.Plan(ctx, glc.CUDPP_SA, max(SWEEP_N)) as plan:
        plan.set_chains(*EVERY)
        for n in SWEEP_N:
            for k, x in enumerate(_mosaic_set(n, 12 if n <= 4099 else 4, 50000 + n)):
                for mode in (1, 2):
                    plan.set_sorter(mode)
                    t = _check_sa(glc, plan, x, "mosaic n=%d #%d" % (n, k), mode, EVERY if n <= 16389 else None)
                    total[0] += t[0]
                    total[1] += t[1]
    assert total[0] > 0 and total[1] > 0, total


@pytest.mark.parametrize("nb", [1, 3, 8, 20])
def test_forced_attempts_batched(glc, cuda, nb):
    """glcBwtBatch calls of 1, 3, 8 and 20 blocks (the radix histogram's shapes change at 2 and 8 blocks; the chain records,
    info words and verification cache sit at per-block offsets), every round allowed: BWT + index of every block"""
    taken = 0
    for n in (1000, 4099, 65536):
        calls = [(n, _mosaic_set(n, nb, 70000 + 100 * nb + n))]
        if nb == 1 and n == 1000:                              # the adversarial blocks, each a call of its own length
            calls += [(x.size, [x]) for _, x in M.adversarial_blocks()]
        for m, blocks in calls:
            got, idx, _, (t, r) = _bwt_batch(glc, blocks, m, 1, EVERY)
            taken += t
            for k, x in enumerate(blocks):
                want, widx = _oracle_bwt(x)
                assert int(idx[k]) == widx and np.array_equal(got[k], want), (nb, m, k)
    assert taken > 0, nb


# ---------------------------------------------------------------------------------------------------------------------------
# periodic blocks past the periodic tier's take
# ---------------------------------------------------------------------------------------------------------------------------
PER_TAKE = 256                                                 # csrc/glc_internal.h


def test_periodic_blocks_past_the_tiers_take(glc, cuda):
    """one call of PER_TAKE + 5 periodic blocks of 64 KiB + 123: the tier takes PER_TAKE of them, the general sorter the rest
    (with chains); every block's BWT and index are the oracle's"""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpu-lossless-compression_amd",
                            "csrc", "glc_internal.h")).read()
    assert int(re.search(r"PER_TAKE\s*=\s*(\d+)", src).group(1)) == PER_TAKE
    n = (1 << 16) + 123
    rng = np.random.default_rng(2024)
    kinds = []
    for p in (5, 61, 700, 3001):
        x = np.resize(rng.integers(0, 256, p, dtype=np.uint8), n).copy()
        x[n - 40:] = rng.integers(0, 256, 40, dtype=np.uint8)
        kinds.append(x)
    ab = np.resize(np.frombuffer(b"ab", dtype=np.uint8), n).copy()
    ab[-1] = 0
    kinds.append(ab)
    blocks = [kinds[k % len(kinds)] for k in range(PER_TAKE + 5)]
    got, idx, nper, (taken, refused) = _bwt_batch(glc, blocks, n, 0)
    assert nper == PER_TAKE, nper
    assert taken > 0, (taken, refused)
    wants = [_oracle_bwt(x) for x in kinds]
    for k in range(len(blocks)):
        want, widx = wants[k % len(kinds)]
        assert int(idx[k]) == widx and np.array_equal(got[k], want), k


@pytest.mark.gpu_long
@pytest.mark.parametrize("seed", range(8))
def test_forced_attempts_long_sweep(glc, ctx, seed):
    """more of the forced sweep: 200 mosaics per seed at the sweep's lengths, one block per call, sorters 1 and 2"""
    with glc.Plan(ctx, glc.CUDPP_SA, max(SWEEP_N)) as plan:
        plan.set_chains(*EVERY)
        for n in SWEEP_N:
            for k, x in enumerate(_mosaic_set(n, 40 if n <= 4099 else 10, 900000 + 10000 * seed + n)):
                for mode in (1, 2):
                    plan.set_sorter(mode)
                    _check_sa(glc, plan, x, "seed %d n=%d #%d" % (seed, n, k), mode, EVERY if n <= 16389 else None)
