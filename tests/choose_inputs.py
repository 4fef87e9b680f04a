"""Inputs of the CHOOSE codec's tests (CPU and GPU) and of its golden fixture: blocks by name, and streams whose super-frames come
out as the writer's cases -- all BWT, all order-0, alternating block by block, two runs -- with a ragged tail."""
import numpy as np

import datagen

KINDS = ("text", "logs", "zipf", "zipf15", "noise", "float", "zeros90", "flat")
BWT_KINDS = ("text", "logs")


def block(kind, n, seed):
    if kind == "text":
        return datagen.text_bytes_fast(n, seed=seed)
    if kind == "logs":
        return datagen.log_bytes(n, seed=seed)
    if kind == "zipf":
        return datagen.zipf_bytes(n, seed=seed)
    if kind == "zipf15":
        return datagen.zipf_bytes(n, seed=seed, s=1.5)
    if kind == "float":
        return datagen.float_bytes(n + 3, seed=seed)[:n]
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "flat":                                          # every byte value equally often: order-0 gains nothing, so raw
        return rng.permutation(np.arange(n, dtype=np.int64) & 255).astype(np.uint8)
    assert kind == "zeros90"                                    # 90 % scattered zeros, the rest uniform in 1 .. 15
    return np.where(rng.random(n) < 0.9, 0, rng.integers(1, 16, n)).astype(np.uint8)


def stream(n, layout, tail, seed=1):
    """the blocks named by `layout` (n bytes each) and a tail of (kind, bytes), as one read-only array"""
    parts = [block(k, n, seed + 7 * i) for i, k in enumerate(layout)]
    if tail:
        parts.append(block(tail[0], tail[1], seed + 1000))
    x = np.concatenate(parts)
    x.setflags(write=False)
    return x


# rows = 8: a super-frame that is all BWT, one that is all order-0, one that alternates, one of four blocks in two runs; the tail
# of 1235 bytes is below the rule's minimum length
EIGHT = (("text",) * 4 + ("logs",) * 4 + ("zipf", "noise", "zeros90", "zipf15", "float", "flat", "noise", "zipf") +
         ("text", "zipf") * 4 + ("logs", "text", "zipf", "noise"))
EIGHT_WANT = (8 + 4 + 2, 8 + 4 + 2 + 1, 1 + 1 + 8 + 2 + 1)       # blocks to BWT, to order-0 (the tail with them), frames


def container_input(n=8192):
    return stream(n, EIGHT, ("logs", 1235))
