"""Seeded generators of typed arrays as little-endian bytes, for the container's byte-plane shuffle filter: the kinds of data a
lossless back end for numeric arrays meets (tools/bench_container.py --data, tests/golden/make_container_v2_gold.py)."""
import numpy as np

import datagen

KINDS = {"float32": 4, "smooth32": 4, "smooth64": 8, "quant16": 2}     # name -> element bytes


def _field(count, seed, dtype):
    """a smooth field: a slow sine plus a random walk of small steps"""
    rng = np.random.Generator(np.random.Philox(key=seed))
    t = np.arange(count, dtype=np.float64)
    return (100.0 * np.sin(t * (2.0 * np.pi / 5000.0)) + np.cumsum(rng.standard_normal(count) * 0.01)).astype(dtype)


def typed_bytes(kind, n, seed=0x5eed0010):
    """n bytes of `kind`: float32 ~ N(0,1) (datagen.float_bytes), a smooth float32 / float64 field, or uint16 quantisation
    codes, Laplace-distributed around 512"""
    elem = KINDS[kind]
    count = (n + elem - 1) // elem
    if kind == "float32":
        return datagen.float_bytes(n, seed=seed)
    if kind == "smooth32":
        a = _field(count, seed, np.float32)
    elif kind == "smooth64":
        a = _field(count, seed, np.float64)
    else:
        rng = np.random.Generator(np.random.Philox(key=seed))
        a = np.clip(np.rint(512.0 + rng.laplace(0.0, 6.0, count)), 0, 65535).astype(np.uint16)
    return a.view(np.uint8)[:n].copy()
