"""Integer series for the container filter's delta mode (format version 4): the inputs the mode is for, from
one np.random.Generator(np.random.Philox(key=7)) per call, as little-endian bytes.

  ts64    int64 timestamps: the running sum of steps uniform in [900, 1100)
  ids32   sorted uint32 ids drawn uniformly from [0, 2^31)
  ctr32   uint32 counters: the running sum of Poisson(3) increments
  adc16   12-bit ADC samples in uint16: 2048 + 1500 sin(2 pi t / 700) + N(0, 3), rounded and clipped to [0, 4095]"""
import numpy as np

KINDS = ("ts64", "ids32", "ctr32", "adc16")
ELEM = {"ts64": 8, "ids32": 4, "ctr32": 4, "adc16": 2}


def series_bytes(kind, n):
    """n bytes (n // ELEM[kind] elements) of the series `kind`"""
    rng = np.random.Generator(np.random.Philox(key=7))
    if kind == "ts64":
        x = np.cumsum(rng.integers(900, 1100, n // 8)).astype("<i8")
    elif kind == "ids32":
        x = np.sort(rng.integers(0, 2 ** 31, n // 4)).astype("<u4")
    elif kind == "ctr32":
        x = np.cumsum(rng.poisson(3, n // 4)).astype("<u4")
    elif kind == "adc16":
        t = np.arange(n // 2)
        x = np.clip(np.rint(2048 + 1500 * np.sin(2 * np.pi * t / 700) + rng.normal(0, 3, n // 2)), 0, 4095).astype("<u2")
    else:
        raise ValueError(kind)
    return x.view(np.uint8)
