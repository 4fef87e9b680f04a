"""GPU decoder for the cudppCompress stream.  The reference has
no GPU decoder; parity = round trip through the HIP encoder + HIP decoder, and
HIP decoder == oracle decoder (the gold decoder semantics of
test_compress.cpp:192-311) on streams produced by the ORACLE encoder."""
import numpy as np
import pytest

import datagen
import oracle_lib as O

pytestmark = pytest.mark.gpu


def _cases():
    rng = np.random.default_rng(17)
    return {
        "zipf_1m": datagen.zipf_bytes(1 << 20),
        "text_1m": datagen.text_bytes(1 << 20),
        "float_1m": datagen.float_bytes(1 << 20),
        "ref_vector_1m": O.glibc_rand_bytes(1 << 20, 255),
        "zeros_1m": np.zeros(1 << 20, dtype=np.uint8),
        "log_300001": datagen.log_bytes(300001),
        "one": np.array([9], dtype=np.uint8),
        "n_4097": rng.integers(0, 256, 4097, dtype=np.uint8),
        "two_symbols": rng.integers(0, 2, 70000, dtype=np.uint8),
        "ends_without_unique_min": np.frombuffer(b"abracadabra" * 3000, dtype=np.uint8),   # gold LF walk fails here
    }


@pytest.mark.parametrize("name", list(_cases().keys()))
def test_round_trip_and_oracle_stream(glc, cuda, name):
    import torch
    x = _cases()[name]
    n = x.size
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, max(n, 64), rows=1) as plan:
        d_in = torch.from_numpy(x.copy()).cuda()
        comp = glc.compress_batch(plan, d_in, n, 1)
        back = glc.decompress_batch(plan, comp, n, 1)
        plan.synchronize()
        assert np.array_equal(back.cpu().numpy(), x), name + ": HIP encode -> HIP decode"
        # decode a stream made by the oracle encoder
        r = O.compress(x)
        nsub, stride = comp["nsub"], comp["stride"]
        words = np.zeros(stride, dtype=np.uint32); words[: r["size"]] = r["words"]
        oc = dict(bwt_index=torch.tensor([r["bwt_index"]], dtype=torch.int32, device=cuda),
                  hist=torch.from_numpy(r["hist"].view(np.int32).copy()).cuda(),
                  offsets=torch.from_numpy(r["offsets"].view(np.int32).copy()).cuda(),
                  words=torch.from_numpy(words.view(np.int32)).cuda(), nsub=nsub, stride=stride)
        back2 = glc.decompress_batch(plan, oc, n, 1)
        plan.synchronize()
        assert np.array_equal(back2.cpu().numpy(), x), name + ": oracle encode -> HIP decode"


def test_batch_round_trip(glc, cuda):
    import torch
    n, nb = 1 << 19, 8
    blocks = [datagen.zipf_bytes(n, seed=i) for i in range(4)] + [datagen.text_bytes(n, seed=9), datagen.float_bytes(n),
                                                                 np.zeros(n, dtype=np.uint8), datagen.log_bytes(n)]
    x = np.concatenate(blocks)
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=nb) as plan:
        d_in = torch.from_numpy(x).cuda()
        comp = glc.compress_batch(plan, d_in, n, nb)
        back = glc.decompress_batch(plan, comp, n, nb)
        plan.synchronize()
        assert torch.equal(back, d_in)


@pytest.mark.parametrize("plan_n,n,nb", [(45537, 45537, 5), (70001, 4099, 3), (1 << 16, 65535, 4), (8191, 1, 7)])
def test_batch_round_trip_misaligned_rows(glc, cuda, plan_n, n, nb):
    """rows of odd length: every row but the first starts at an unaligned address inside the plan's
    scratch (vector paths must fall back), and n may be smaller than the plan's block size"""
    import torch
    rng = np.random.default_rng(plan_n + n)
    blocks = []
    for i in range(nb):
        kind = i % 3
        if kind == 0:
            blocks.append(datagen.zipf_bytes(n, seed=100 + i))
        elif kind == 1:
            blocks.append(rng.integers(0, 4, n, dtype=np.uint8))
        else:
            blocks.append(np.frombuffer((b"the quick brown fox " * (n // 20 + 1))[:n], dtype=np.uint8))
    x = np.concatenate(blocks)
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, plan_n, rows=nb) as plan:
        d_in = torch.from_numpy(x.copy()).cuda()
        comp = glc.compress_batch(plan, d_in, n, nb)
        back = glc.decompress_batch(plan, comp, n, nb)
        plan.synchronize()
        assert torch.equal(back, d_in)
        sizes = comp["size"].cpu().numpy()
        for b in range(nb):                                    # and every block equals the oracle's stream
            want = O.compress(blocks[b])
            got = comp["words"][b * comp["stride"]: b * comp["stride"] + int(sizes[b])].cpu().numpy().view(np.uint32)
            assert int(comp["bwt_index"][b].item()) == want["bwt_index"] and int(sizes[b]) == want["size"]
            assert np.array_equal(got, want["words"])


def test_pipelined_decode_calls(glc, cuda):
    """glcPlanSetPipelining on the decode side: Huffman + inverse MTF of call i+1 on the second stream
    while the inverse BWT of call i runs on the plan's stream; six back-to-back calls, outputs read
    through the plan's stream."""
    import torch
    n, nb, calls = 1 << 17, 4, 6
    batches = [np.concatenate([datagen.zipf_bytes(n, seed=3000 + 10 * c + b) if (b + c) % 2 else
                               datagen.text_bytes(n, seed=4000 + 10 * c + b) for b in range(nb)]) for c in range(calls)]
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=nb) as plan:
        comps = [glc.compress_batch(plan, torch.from_numpy(x).cuda(), n, nb) for x in batches]
        plan.synchronize()
        plan.set_pipelining(True)
        outs = [glc.decompress_batch(plan, c, n, nb) for c in comps]           # no sync in between
        plan.synchronize()
        for x, o in zip(batches, outs):
            assert np.array_equal(o.cpu().numpy(), x)
        plan.set_pipelining(False)
        back = glc.decompress_batch(plan, comps[2], n, nb)
        plan.synchronize()
        assert np.array_equal(back.cpu().numpy(), batches[2])


def test_corrupt_stream_is_reported_not_followed(glc, cuda):
    """row index, block offsets and block lengths are stream data: out-of-range values must not be
    dereferenced, and glcPlanSynchronize has to report them"""
    import torch
    n = 1 << 16
    x = datagen.zipf_bytes(n, seed=3)
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=1) as plan:
        comp = glc.compress_batch(plan, torch.from_numpy(x).cuda(), n, 1)
        plan.synchronize()
        for what in ("index", "offset", "length", "hist_wrap", "hist_sum"):
            bad = {k: (v.clone() if hasattr(v, "clone") else v) for k, v in comp.items()}
            if what == "hist_wrap":
                bad["hist"][5] = 1 << 23                           # would wrap the tree builder's count << 9 | slot key
            elif what == "hist_sum":
                bad["hist"][7] += 3                                # counts that do not add up to n
            elif what == "index":
                bad["bwt_index"][0] = n + 12345
            elif what == "offset":
                bad["offsets"][3] = 0x7FFFFFF0
            else:
                bad["words"][int(comp["offsets"][2].item())] = 0x7FFFFFFF
            glc.decompress_batch(plan, bad, n, 1)
            with pytest.raises(glc.CudppError):
                plan.synchronize()
        back = glc.decompress_batch(plan, comp, n, 1)           # the plan is still usable
        plan.synchronize()
        assert np.array_equal(back.cpu().numpy(), x)


# the live profile of one compress and one decompress call of two 8192-byte Zipf blocks (none flagged: no tier behind the
# bucket sorter runs): every bracket once, n * rows units each.  Counts from a run of this test on commit 7cea40a's library.
PROFILE_UNITS = 8192.0 * 2
PROFILE_LAUNCHES = {
    "k_fs_hist": 1, "k_fs_part": 1, "k_fs_sort": 1, "k_mtf_chunk_lists+k_mtf_scan_lists": 1, "k_mtf_encode": 1,
    "k_huff_build": 1, "k_huff_pack": 1,
    "k_dec_prepare+k_dec_huff": 1, "k_imtf_pos": 1, "k_imtf_scan+k_imtf_apply": 1, "k_ibwt_hist+k_rs_scan+k_ibwt_lf": 1,
    "k_ibwt_walk": 1, "k_ibwt_rank+k_ibwt_emit": 1,
}


@pytest.mark.parametrize("pipelined", [False, True])
def test_profile_counts_of_one_call_each_way(glc, cuda, pipelined):
    import ctypes as C
    import torch
    n, nb = 8192, 2
    x = np.concatenate([datagen.zipf_bytes(n, seed=61), datagen.zipf_bytes(n, seed=62)])
    d_in = torch.from_numpy(x).cuda()
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=nb) as plan:
        comp = glc.compress_batch(plan, d_in, n, nb)              # a finished stream for the decode call to read
        plan.synchronize()
        assert plan.last_flagged_blocks() == 0
        plan.set_pipelining(pipelined)
        plan.enable_timing(3)
        again = glc.compress_batch(plan, d_in, n, nb)
        back = glc.decompress_batch(plan, comp, n, nb)
        plan.synchronize()
        assert torch.equal(back, d_in) and torch.equal(again["size"], comp["size"])
        prof = plan.kernel_profiles()
        lost = (C.c_ulonglong * 2)()
        assert glc.lib().glcPlanKernelProfileLost(plan.handle, lost) == glc.CUDPP_SUCCESS
        ms = plan.last_timing()
        assert {k: v["launches"] for k, v in prof.items()} == PROFILE_LAUNCHES
        assert all(v["units"] == PROFILE_UNITS * v["launches"] for v in prof.values())
        assert tuple(lost) == (0, 0)
        assert len(ms) == 4 and all(np.isfinite(v) and v >= 0 for v in ms)
        if pipelined:                                             # the total is the sum of the three spans, in float32 as the library adds them
            assert ms[3] == float(np.float32(np.float32(np.float32(ms[0]) + np.float32(ms[1])) + np.float32(ms[2])))
