"""Row-major volumes for the 3-D predictor of the container's filter (INTEGRATION.md 4b "Delta: volume", format version 17), as
little-endian bytes at any row width W and plane stride S in elements; S need not be a multiple of W (the last row of a plane is
then short: element i lies at z = i // S, y = i % S // W, x = i % S % W).  Noise comes from one
np.random.Generator(np.random.Philox(key=...)) per call.

With f(x, y, z) = sin(x / 30) cos(y / 19) sin(z / 11 + 1) + 0.3 sin((x - y + 2 z) / 13):

  smooth32  float32: 700 + 100 f                       (within [512, 1024): one exponent, so the bit patterns are linear in the value)
  smooth64  float64: 700 + 100 f
  round32   float32: 700 + 100 f rounded to 1e-2
  ct16      int16: rint(10000 + 8000 f), no noise
  ct16n     int16: rint(10000 + 8000 f + N(0, 30))      a noisy stack: every further difference doubles the noise variance
  series    series_datagen's ts64: no volume at all

The amplitudes are chosen so that on the inputs called SMOOTH the 2-D residual, about A / (30 * 19) for an amplitude A, stands
well above the rounding of the values (0.29 of the last kept digit per value, 0.58 over the 2-D predictor's four terms, 0.82 over
the 3-D predictor's eight): there the 3-D residual, a further factor 1 / 11 smaller, is what the coder sees, and the third
difference pays.  On ct16n the noise stands above both residuals and the third difference only adds to it."""
import numpy as np

KINDS = {"smooth32": 4, "smooth64": 8, "round32": 4, "ct16": 2, "ct16n": 2, "series": 8}       # name -> elem
SMOOTH = ("smooth32", "smooth64", "round32", "ct16")
STRIDES = ((64, 4096), (50, 2057))                               # (W, S): a small volume of whole rows; S no multiple of W (41 rows and 7)


def field(n_elems, width, plane):
    i = np.arange(n_elems, dtype=np.int64)
    z, r = i // plane, i % plane
    y, x = (r // width).astype(np.float64), (r % width).astype(np.float64)
    z = z.astype(np.float64)
    return np.sin(x / 30) * np.cos(y / 19) * np.sin(z / 11 + 1) + 0.3 * np.sin((x - y + 2 * z) / 13)


def vol_bytes(kind, n, width, plane, seed=0x3d17):
    """n bytes of `kind` laid out in rows of `width` and planes of `plane` elements"""
    elem = KINDS[kind]
    if kind == "series":
        import series_datagen
        return np.ascontiguousarray(series_datagen.series_bytes("ts64", n))
    m = n // elem + 1
    f = field(m, width, plane)
    if kind == "smooth32":
        a = (700 + 100 * f).astype("<f4")
    elif kind == "smooth64":
        a = (700 + 100 * f).astype("<f8")
    elif kind == "round32":
        a = np.round(700 + 100 * f, 2).astype("<f4")
    elif kind == "ct16":
        a = np.rint(10000 + 8000 * f).astype("<i2")
    elif kind == "ct16n":
        rng = np.random.Generator(np.random.Philox(key=seed))
        a = np.rint(10000 + 8000 * f + rng.normal(0, 30, m)).astype("<i2")
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)[:n].copy()
