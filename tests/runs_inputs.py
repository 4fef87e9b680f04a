"""Inputs of the runs-mode tests (CPU and GPU) and of the golden fixture."""
import numpy as np

import datagen

# 333 bytes over "abcd" whose BWT has no two equal neighbours, so the MTF bytes hold no zero: a kind-4 record with nB = 0
# (found by a hill climb on the number of equal neighbours; checked by the tests that use it)
NO_ZERO_BLOCK = np.frombuffer(
    b"ddaadccadcaabdaacccccabccbddaccdbcbaabdcbdbbddcbacbdacdbaadcabcdbbabacadcadbcbcddcaddcbcacdbbcbbddcdcadacbcabbbbdbdaddbabaddb"
    b"daaabbcbddccbabddcaadbcdacdbccbadacddddadccbccaccacdadbacacacdababcaacbadddaaaccbaaaaddabbbaaacaacdaccaadabcdaacddbdcdadbda"
    b"bacdcccaabbaacadbdbdcbbbccdabcbbcdcbaadbbcacccadbadbddbadabbcbbbacbbdcddccddabdadbbdc", dtype=np.uint8)
assert NO_ZERO_BLOCK.size == 333

SPLIT_SIZES = (1, 2, 255, 256, 257, 1000, 4096, 70001)
SPLIT_DENSITIES = (0.0, 0.5, 0.97, 1.0)


def density_segment(n, density, seed=0):
    """n bytes of which about `density` are zero (all of them at 1, none at 0)"""
    rng = np.random.default_rng(1000 * n + int(100 * density) + seed)
    x = rng.integers(1, 256, n).astype(np.uint8)
    x[rng.random(n) < density] = 0
    return x


def page(n=4096):
    return datagen.text_bytes(n, seed=11)


def container_inputs(block_len, rows=4):
    """{name: bytes} for a writer plan of this shape: text and log of two frames and a ragged tail, a page repeated, zeros, a
    one-byte tail behind whole frames, the empty input"""
    whole = rows * block_len
    n = 2 * whole + block_len // 3 + 1 if block_len <= 4096 else whole + block_len // 3 + 1
    rep = np.tile(page(min(4096, block_len)), n // min(4096, block_len) + 1)[:n]
    return {"text": datagen.text_bytes_fast(n, seed=21), "log": datagen.log_bytes(n, seed=22), "page": rep,
            "zeros": np.zeros(n, np.uint8), "tail1": np.concatenate([datagen.text_bytes_fast(whole, seed=23), [np.uint8(0)]]).astype(np.uint8),
            "empty": np.zeros(0, np.uint8)}
