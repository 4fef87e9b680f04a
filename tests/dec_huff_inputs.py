"""Symbol arrays for the two Huffman decode kernels (test_gpu_dec_huff_kernels.py): built for what the lane kernel's word
ring, refill rule and store tail, and both kernels' walk past the 12-bit table, can get wrong.  The streams come from the
oracle encoder; `describe` measures on the CPU the properties the arrays are there for."""
import numpy as np

import oracle_lib as O

SUB = 4096                                                   # symbols per sub-block (HUFF_BLOCK)
LUT_BITS = 12                                                # DEC_LUT_BITS of csrc/decode.hip
SIZES = (1, 15, 16, 17, 4095, 4096, 4097, 8192 + 15, 8192 + 16, 8192 + 17, 45537, 1 << 20)
FIB_COUNTS = 27
FIB_LONG_PER_SUB = 160
SKEW_HEAVY, SKEW_HEAVY_COUNT = 8, 200


def zipf_symbols(n, seed):
    """MTF-like bytes: small values frequent, every value possible"""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, 257)
    return rng.choice(256, size=n, p=p / p.sum()).astype(np.uint8)


def fib_longest_codes():
    """Counts 1, 2, 3, 5, 8, ... over 27 symbols (n = 832038): the tree is a chain, code lengths 27, 26, ..., 1 (EOF: 27;
    code_of_28_bits below goes one further).  The 2582 symbols with codes of 13 bits or more are laid out longest first, 160
    at the START of each sub-block -- the first aligned group of 16 symbols costs 389 bits -- except in sub-block 1, where
    they go at its END, so that long codes run into the zero-filled tail of the stream.  The rest is shuffled."""
    counts = [1, 2]
    while len(counts) < FIB_COUNTS:
        counts.append(counts[-1] + counts[-2])
    counts = np.array(counts, dtype=np.int64)                # symbol s has counts[s]: lengths 27 - s (s = 0 and EOF: 27)
    n = int(counts.sum())
    lens = FIB_COUNTS - np.arange(FIB_COUNTS)
    lens[0] = FIB_COUNTS
    is_long = lens > LUT_BITS
    longs = np.repeat(np.arange(FIB_COUNTS, dtype=np.uint8)[is_long], counts[is_long])      # longest first
    rest = np.repeat(np.arange(FIB_COUNTS, dtype=np.uint8)[~is_long], counts[~is_long])
    rest = np.random.default_rng(832038).permutation(rest)
    out = np.empty(n, dtype=np.uint8)
    taken = np.zeros(n, dtype=bool)
    for k in range((longs.size + FIB_LONG_PER_SUB - 1) // FIB_LONG_PER_SUB):
        part = longs[k * FIB_LONG_PER_SUB:(k + 1) * FIB_LONG_PER_SUB]
        at = k * SUB if k != 1 else 2 * SUB - part.size
        out[at:at + part.size] = part
        taken[at:at + part.size] = True
    out[~taken] = rest
    return out


def skewed_sub_block():
    """A 64 KiB block: 15 sub-blocks of one symbol each and one sub-block spread over the others, so that in that sub-block
    codes past the 12-bit table are the rule and its word count comes near HUFF_MAX_WORDS.  (With ONE symbol in all 15
    sub-blocks that symbol takes half of the code space in one bit and the 255 others share the rest at about 9 bits: no
    spread gets the bulk of a sub-block past 12 bits.  With a symbol per constant sub-block, 15 codes of 4 bits leave a
    sixteenth of the code space to 241 symbols.)  The spread: 8 symbols 200 times each and the other 233 about 11 times
    each -- 13 bits; an even spread over all 241, 17 times each, gets codes of exactly 12 bits, all inside the table.
    Measured with the oracle: 55 % of the sub-block past 12 bits, 1407 of the 1536 words a sub-block may take."""
    const = np.repeat(np.arange(15, dtype=np.uint8), SUB)
    heavy = np.repeat(np.arange(15, 15 + SKEW_HEAVY, dtype=np.uint8), SKEW_HEAVY_COUNT)
    light_syms = np.arange(15 + SKEW_HEAVY, 256, dtype=np.uint8)
    light = np.resize(light_syms, SUB - heavy.size)
    spread = np.random.default_rng(65536).permutation(np.concatenate([heavy, light]))
    # the spread sub-block in the middle (sub-block 7): its neighbours' streams sit on both sides of its words
    return np.concatenate([const[:7 * SUB], spread, const[7 * SUB:]]), 7


def chain_histogram(rare, first):
    """`rare` symbols that occur once, one that occurs `first` times, then every count the least that keeps the tree a chain
    above them (more than the chain weighs so far: the tree rule takes a leaf before a composite of the same count); what is
    left of 2^20 goes to the last symbol"""
    h = [1] * rare + [first]
    below, total = sum(h) + 1 - first, sum(h) + 1              # (+ 1: the EOF leaf)
    while True:
        c = max(h[-1], below + 1)
        if sum(h) + c > 1 << 20:
            break
        h.append(c)
        below, total = total, total + c
    h[-1] += (1 << 20) - sum(h)
    return np.array(h, dtype=np.int64)


def group_of_14_words():
    """The most a group of 16 symbols was found to cost: 15 symbols that occur once under a chain (n = 2^20) get 27 and 26
    bits, the next one 24 -- 422 bits, against 389 for the 16 rarest of the Fibonacci counts.  With a 22-bit code just
    before it the group starts with few bits in hand and takes 14 words, the number the lane kernel's refill rule is
    written for; it sits where a ring refilled at 12 words and below has 13 (found by search with ring_model; any
    threshold from 13 to 16 serves every stream).  Sub-block 1, groups 41 on."""
    h = chain_histogram(15, 8)
    left = h.copy()
    left[:15] = 0
    left[15] -= 1
    left[16] -= 1
    perm = np.random.default_rng(1).permutation(np.repeat(np.arange(h.size, dtype=np.uint8), left))
    pre, others = perm[:SUB - 17], perm[SUB - 17:]
    at = 16 * 41 - 1
    sub = np.concatenate([pre[:at], [16], np.arange(16), pre[at:]]).astype(np.uint8)
    return np.concatenate([others[:SUB], sub, others[SUB:]])


def code_of_28_bits():
    """4 symbols that occur once and one that occurs 4 times under a chain: n = 2^20 reaches codes of 28 bits, one more than
    the Fibonacci counts.  The rare symbols open sub-block 2."""
    h = chain_histogram(4, 4)
    left = h.copy()
    left[:5] = 0
    perm = np.random.default_rng(28).permutation(np.repeat(np.arange(h.size, dtype=np.uint8), left))
    rare = np.repeat(np.arange(5, dtype=np.uint8), h[:5])
    return np.concatenate([perm[:2 * SUB], rare, perm[2 * SUB:]])


def ring_model(sym_lens, threshold=16):
    """The lane kernel's word ring on the code lengths of one block, per sub-block: 32 words, two taken at the start, 16
    more before a group of 16 symbols whenever `threshold` or fewer are left; a word is taken when 32 bits or fewer are
    in hand.  Returns (words in the ring after each group, words each group took), [sub-block][group]; a negative count is
    a ring run dry.  (Before symbol i the kernel has taken floor(bits of the symbols before i / 32) words past the first two.)"""
    L = np.concatenate([sym_lens, np.zeros(-sym_lens.size % SUB, dtype=np.int64)]).reshape(-1, SUB)
    before_last = np.cumsum(L, axis=1)[:, 14::16]                # bits consumed before the last symbol of each group
    taken = np.diff(before_last // 32, axis=1, prepend=0)
    have = np.full(L.shape[0], 30, dtype=np.int64)
    left = np.empty_like(taken)
    for g in range(taken.shape[1]):
        have = have + np.where(have <= threshold, 16, 0) - taken[:, g]
        left[:, g] = have
    return left, taken


def single_block_cases():
    """name -> symbols, one block each"""
    rng = np.random.default_rng(20261020)
    cases = {"size_%d" % n: zipf_symbols(n, seed=n) for n in SIZES}
    cases["constant"] = np.full(3 * SUB + 100, 200, dtype=np.uint8)                  # one symbol + EOF: codes of one bit
    cases["two_symbols"] = rng.integers(0, 2, 5 * SUB + 77).astype(np.uint8) * 255
    cases["uniform_256"] = rng.integers(0, 256, 1 << 16).astype(np.uint8)            # every code inside the table
    cases["last_sub_block_of_5"] = zipf_symbols(2 * SUB + 5, seed=5)
    cases["last_sub_block_of_100"] = zipf_symbols(SUB + 100, seed=100)               # 16 to 31 words
    # 15 sub-blocks of ONE symbol, one spread over the 255 others: the symbol takes half of the code space, the others 9 bits
    cases["one_symbol_and_255_others"] = np.concatenate([np.zeros(15 * SUB, dtype=np.uint8),
                                                         rng.permutation(np.resize(np.arange(1, 256, dtype=np.uint8), SUB))])
    cases["skewed_sub_block"] = skewed_sub_block()[0]
    cases["fib_longest_codes"] = fib_longest_codes()
    cases["group_of_14_words"] = group_of_14_words()
    cases["code_of_28_bits"] = code_of_28_bits()
    return cases


def batch_cases():
    """(plan n, n, nblk): rows at odd strides -- rows 1 and 2 start unaligned"""
    return [(4099, 4099, 3), (70001, 4099, 3), (45537, 45537, 3), (65535, 65535, 3)]


def batch_blocks(n, nblk):
    return [zipf_symbols(n, seed=7 * n + b) if b != 1 else np.random.default_rng(n).integers(0, 256, n).astype(np.uint8)
            for b in range(nblk)]


def encode(sym):
    """the oracle's stream of one block; rc must be 0 (every sub-block within the format's 1536 words)"""
    r = O.huff_encode(sym)
    assert r["rc"] == 0, "the case is mis-built: a sub-block overflows the format"
    return r


def describe(sym, r=None):
    """what the stream of `sym` looks like: code lengths, bits per aligned group of 16 symbols, words per sub-block"""
    r = r or encode(sym)
    _, lens, _ = O.huff_codes(r["hist"])
    L = lens[sym].astype(np.int64)
    pad = np.concatenate([L, np.zeros(-L.size % 16, dtype=np.int64)])
    # groups of 16 are aligned inside a sub-block: 4096 is a multiple of 16
    group_bits = pad.reshape(-1, 16).sum(axis=1)
    words = r["words"][r["offsets"]].astype(np.int64)
    return dict(lens=lens, sym_lens=L, max_len=int(L.max()), eof_len=int(lens[256]), group_bits=group_bits, sub_words=words)
