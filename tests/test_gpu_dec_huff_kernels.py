"""Each Huffman decode kernel on its own (-m gpu): k_dec_huff (one wave per 4096-symbol sub-block) and k_dec_huff_lanes (one
lane per sub-block; by default only calls of 32768 sub-blocks and more reach it), forced with glcPlanSetHuffDecoder and run
through glcHuffmanDecodeBatch on streams of the ORACLE encoder over chosen symbol arrays (dec_huff_inputs.py).  The
expected output is the symbol array itself.  The lane kernel has its own word ring, prefetch, refill rule and store path:
the inputs hold ragged last sub-blocks, sub-blocks of a word or two, rows at odd strides, the compact layout, codes past
the 12-bit table as the rule, the longest codes a block can have, and corrupt streams."""
import functools

import numpy as np
import pytest

import datagen
import dec_huff_inputs as D
import oracle_lib as O

MODES = (1, 2)                                               # glcPlanSetHuffDecoder: 1 k_dec_huff, 2 k_dec_huff_lanes
GUARD = 64                                                   # bytes behind the output that must stay as they were
SINGLE = list(D.single_block_cases().keys())


@functools.lru_cache(maxsize=None)
def _single():
    """name -> (symbols, the oracle's stream), built once for the CPU test and both modes"""
    return {k: (v, D.encode(v)) for k, v in D.single_block_cases().items()}


def _strided(glc, cuda, streams, n):
    """the dict glc.huffman_decode_batch / glc.decompress_batch read, from one oracle stream per block"""
    import torch
    nblk, nsub, stride = len(streams), (n + D.SUB - 1) // D.SUB, glc.compressed_stride_words(n)
    words = np.zeros(nblk * stride, dtype=np.uint32)
    for b, r in enumerate(streams):
        assert r["rc"] == 0 and r["size"] <= stride
        words[b * stride:b * stride + r["size"]] = r["words"]
    out = dict(hist=torch.from_numpy(np.concatenate([r["hist"] for r in streams]).view(np.int32).copy()).to(cuda),
               offsets=torch.from_numpy(np.concatenate([r["offsets"] for r in streams]).view(np.int32).copy()).to(cuda),
               words=torch.from_numpy(words.view(np.int32)).to(cuda), nsub=nsub, stride=stride)
    if "bwt_index" in streams[0]:
        out["bwt_index"] = torch.tensor([r["bwt_index"] for r in streams], dtype=torch.int32, device=cuda)
    return out


def _decode_symbols(glc, cuda, plan, comp, n, nblk):
    """glcHuffmanDecodeBatch into a buffer with a guard behind it; the symbols, after the guard was seen intact"""
    import torch
    buf = torch.full((nblk * n + GUARD,), 0xA5, dtype=torch.uint8, device=cuda)
    glc.huffman_decode_batch(plan, comp, n, nblk, d_sym=buf)
    plan.synchronize()
    got = buf.cpu().numpy()
    assert np.all(got[nblk * n:] == 0xA5), "the kernel wrote behind the last row"
    return got[:nblk * n]


def test_the_inputs_have_the_properties_they_are_there_for():
    """CPU: what each input is meant to put in front of the kernels, measured on the oracle's stream"""
    cases = _single()
    fib = D.describe(*cases["fib_longest_codes"])
    assert cases["fib_longest_codes"][0].size == 832038
    assert fib["max_len"] == 27 and fib["eof_len"] == 27
    assert np.array_equal(fib["lens"][:27], [27] + list(range(26, 0, -1)))
    assert int((fib["sym_lens"] > D.LUT_BITS).sum()) == 2582
    # the first aligned group of 16 symbols, the 16 rarest: 389 bits = 12.2 words (group_of_14_words below has more)
    assert fib["group_bits"][0] == 389 and fib["group_bits"].max() == 389
    assert set((fib["sub_words"] % 16).tolist()) == set(range(16))          # every residue, so 0, 1 and 15
    # sub-block 1 ends in its long codes: the last word of its stream is followed by the zero fill
    assert np.all(fib["sym_lens"][2 * D.SUB - D.FIB_LONG_PER_SUB:2 * D.SUB] > D.LUT_BITS)
    # sub-blocks of fewer than 16 words (the lane kernel's first fetch zero-fills) and of 16 to 31 (its second one does)
    words = np.concatenate([D.describe(*c)["sub_words"] for c in cases.values()])
    assert np.any(words < 16) and np.any((words >= 16) & (words < 32))
    assert D.describe(*cases["size_1"])["sub_words"].tolist() == [1]
    five = D.describe(*cases["last_sub_block_of_5"])["sub_words"]
    assert five.size == 3 and 1 <= five[-1] <= 2
    assert 16 <= D.describe(*cases["last_sub_block_of_100"])["sub_words"][-1] < 32
    assert D.describe(*cases["uniform_256"])["max_len"] <= D.LUT_BITS        # every code inside the table
    sym, k = D.skewed_sub_block()
    sk = D.describe(*cases["skewed_sub_block"])
    assert np.array_equal(sym, cases["skewed_sub_block"][0])
    assert (sk["sym_lens"][k * D.SUB:(k + 1) * D.SUB] > D.LUT_BITS).mean() > 0.5
    assert 1300 < sk["sub_words"][k] <= 1536
    assert D.describe(*cases["one_symbol_and_255_others"])["max_len"] == 9   # (why skewed_sub_block has a symbol per sub-block)
    assert D.describe(*cases["code_of_28_bits"])["max_len"] == 28
    # the refill rule ("16 symbols take at most 14 words"): no case runs a ring refilled at 16 words and below dry or
    # over its 32 words, one group takes the 14, and refilling at 12 and below would have it start on 13
    for name, c in cases.items():
        left, taken = D.ring_model(D.describe(*c)["sym_lens"])
        assert left.min() >= 0 and (left + taken).max() <= 32 and taken.max() <= 14, name
    top = D.describe(*cases["group_of_14_words"])
    assert top["group_bits"].max() == 422 and top["max_len"] == 27
    assert D.ring_model(top["sym_lens"])[1].max() == 14
    assert D.ring_model(top["sym_lens"], 13)[0].min() >= 0 and D.ring_model(top["sym_lens"], 12)[0].min() < 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SINGLE)
def test_single_block(glc, cuda, name, mode):
    sym, r = _single()[name]
    n = sym.size
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=1) as plan:
        plan.set_huff_decoder(mode)
        got = _decode_symbols(glc, cuda, plan, _strided(glc, cuda, [r], n), n, 1)
    bad = np.flatnonzero(got != sym)
    assert bad.size == 0, "%s, mode %d: %d symbols differ, the first at %d (sub-block %d, symbol %d of it)" % (
        name, mode, bad.size, bad[0], bad[0] // D.SUB, bad[0] % D.SUB)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("plan_n,n,nblk", D.batch_cases())
def test_batches_at_odd_strides(glc, cuda, plan_n, n, nblk, mode):
    """rows 1 and 2 start unaligned: at stride n in glcHuffmanDecodeBatch's output, at the plan's n inside glcDecompressBatch"""
    blocks = D.batch_blocks(n, nblk)
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, plan_n, rows=nblk) as plan:
        plan.set_huff_decoder(mode)
        got = _decode_symbols(glc, cuda, plan, _strided(glc, cuda, [D.encode(b) for b in blocks], n), n, nblk)
        assert np.array_equal(got, np.concatenate(blocks)), "glcHuffmanDecodeBatch"
        full = [O.compress(b) for b in blocks]
        back = glc.decompress_batch(plan, _strided(glc, cuda, full, n), n, nblk)
        plan.synchronize()
        assert np.array_equal(back.cpu().numpy(), np.concatenate(blocks)), "glcDecompressBatch"


@pytest.mark.gpu
def test_the_modes_and_the_default_give_the_same_bytes(glc, cuda):
    """one plan through modes 0, 1, 2 and back; a mode that does not exist is refused and changes nothing"""
    sym, r = _single()["size_45537"]
    n = sym.size
    L = glc.lib()
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=1) as plan, \
            glc.Plan(ctx, glc.CUDPP_MTF, n, rows=1) as mtf_plan:
        comp = _strided(glc, cuda, [r], n)
        for mode in (0, 1, 2, 0):
            plan.set_huff_decoder(mode)
            for bad in (-1, 3, 100):
                assert L.glcPlanSetHuffDecoder(plan.handle, bad) == glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION
            assert np.array_equal(_decode_symbols(glc, cuda, plan, comp, n, 1), sym), mode
        assert L.glcPlanSetHuffDecoder(0, 1) == glc.CUDPP_ERROR_INVALID_HANDLE
        assert L.glcPlanSetHuffDecoder(mtf_plan.handle, 1) == glc.CUDPP_ERROR_INVALID_PLAN
        assert L.glcHuffmanDecodeBatch(mtf_plan.handle, 0, 0, 1, 0, 1, 0, n, 1) == glc.CUDPP_ERROR_INVALID_PLAN
        assert L.glcHuffmanDecodeBatch(plan.handle, 0, 0, 1, 0, 1, 0, n + 1, 1) == glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION
        assert L.glcHuffmanDecodeBatch(plan.handle, 0, 0, 1, 0, 1, 0, n, 2) == glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (2, 1))
def test_compact_layout_round_trip(glc, cuda, mode):
    """a round trip of test_gpu_compact.py again under each kernel: in the compact layout a block's words start wherever
    the one before ended, 4-byte aligned under the lane kernel's 16-byte loads; pipelined and not"""
    import torch
    n, kinds = 40961, ["zipf", "float", "zipf"]
    gens = {"zipf": datagen.zipf_bytes, "float": datagen.float_bytes}
    x = np.concatenate([gens[k](n, seed=11 + i) for i, k in enumerate(kinds)])
    d_in = torch.from_numpy(x).to(cuda)
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=len(kinds)) as plan:
        got = glc.compress_batch_compact(plan, d_in, n, len(kinds))
        plan.synchronize()
        plan.set_huff_decoder(mode)
        back = glc.decompress_batch_compact(plan, got, n, len(kinds))
        plan.synchronize()
        assert torch.equal(back, d_in)
        plan.set_pipelining(True)
        back2 = glc.decompress_batch_compact(plan, got, n, len(kinds))
        plan.synchronize()
        plan.set_pipelining(False)
        assert torch.equal(back2, d_in)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (2, 1))
def test_corrupt_stream_is_reported_not_followed(glc, cuda, mode):
    """the five manipulations of test_gpu_decode.py under each kernel: reported at synchronize, and the plan decodes the
    good stream afterwards.  (The lane kernel clamps offsets and lengths as the wave kernel does; its ring is indexed
    modulo 32 whatever a stream's codes add up to.)"""
    import torch
    n = 1 << 16
    x = datagen.zipf_bytes(n, seed=3)
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=1) as plan:
        comp = glc.compress_batch(plan, torch.from_numpy(x).cuda(), n, 1)
        plan.synchronize()
        plan.set_huff_decoder(mode)
        for what in ("index", "offset", "length", "hist_wrap", "hist_sum"):
            bad = {k: (v.clone() if hasattr(v, "clone") else v) for k, v in comp.items()}
            if what == "hist_wrap":
                bad["hist"][5] = 1 << 23
            elif what == "hist_sum":
                bad["hist"][7] += 3
            elif what == "index":
                bad["bwt_index"][0] = n + 12345
            elif what == "offset":
                bad["offsets"][3] = 0x7FFFFFF0
            else:
                bad["words"][int(comp["offsets"][2].item())] = 0x7FFFFFFF
            glc.decompress_batch(plan, bad, n, 1)
            with pytest.raises(glc.CudppError):
                plan.synchronize()
            if what != "index":                                   # the same through the stage's own entry
                glc.huffman_decode_batch(plan, bad, n, 1)
                with pytest.raises(glc.CudppError):
                    plan.synchronize()
        back = glc.decompress_batch(plan, comp, n, 1)
        plan.synchronize()
        assert np.array_equal(back.cpu().numpy(), x)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (2, 1))
def test_compact_offsets_that_leave_the_array(glc, cuda, mode):
    import torch
    n, nblk = 1 << 16, 3
    x = np.concatenate([datagen.zipf_bytes(n, seed=11 + i) for i in range(nblk)])
    d_in = torch.from_numpy(x).to(cuda)
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=nblk) as plan:
        out = glc.compress_batch_compact(plan, d_in, n, nblk)
        plan.synchronize()
        plan.set_huff_decoder(mode)
        total = int(out["block_off"][nblk].item())
        for bad in ([0, total + 5, total + 9, total + 20], [0, 900, 400, total]):
            comp = dict(out)
            comp["words"] = out["words"][:total]
            comp["block_off"] = torch.tensor(bad, dtype=torch.int64, device=cuda)
            glc.decompress_batch_compact(plan, comp, n, nblk)
            with pytest.raises(glc.CudppError):
                plan.synchronize()
        back = glc.decompress_batch_compact(plan, out, n, nblk)
        plan.synchronize()
        assert torch.equal(back, d_in)
