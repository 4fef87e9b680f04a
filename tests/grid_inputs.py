"""Row-major gridded inputs for the 2-D predictor of the container's filter (INTEGRATION.md 4b "Delta: grid", format version 12),
each from one np.random.Generator(np.random.Philox(key=...)) per call, as little-endian bytes, at any row width W in elements.

  img16     uint16: a 12-bit image, 2048 + 1200 sin(x / 40) cos(y / 55) + 500 sin((x + 2 y) / 90) + N(0, 3), clipped to [0, 4095]
  field32   float32: a simulation field, 300 + 10 f(x, y) + N(0, 1e-3) with f = sin(x / 120) cos(y / 75) + 0.3 sin((x - y) / 31)
  walk32    int32: a 2-D random walk, the running sum along both axes of steps uniform in [-3, 3]"""
import numpy as np

KINDS = {"img16": 2, "field32": 4, "walk32": 4}                 # name -> elem


def grid_bytes(kind, n, width, seed=0x961d):
    """n bytes of `kind` in rows of `width` elements (whole rows, then cut to n)"""
    elem = KINDS[kind]
    rng = np.random.Generator(np.random.Philox(key=seed))
    rows = n // (elem * width) + 1
    y, x = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    if kind == "img16":
        s = 2048 + 1200 * np.sin(x / 40) * np.cos(y / 55) + 500 * np.sin((x + 2 * y) / 90)
        a = np.clip(np.rint(s + rng.normal(0, 3, s.shape)), 0, 4095).astype("<u2")
    elif kind == "field32":
        f = np.sin(x / 120) * np.cos(y / 75) + 0.3 * np.sin((x - y) / 31)
        a = (300 + 10 * f + rng.normal(0, 1e-3, f.shape)).astype("<f4")
    elif kind == "walk32":
        a = np.cumsum(np.cumsum(rng.integers(-3, 4, (rows, width)), axis=0), axis=1).astype("<i4")
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)[:n].copy()
