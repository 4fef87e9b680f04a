"""Interleaved-channel inputs for the lagged, folded delta of the container's filter (INTEGRATION.md 4b "Delta: lag and fold",
format version 11), each from one np.random.Generator(np.random.Philox(key=...)) per call, as little-endian bytes.  A frame of C
channels is C consecutive elements, so the element C places back is the same channel's previous sample.

  stereo16   2 x int16: two sines of different period and phase, amplitude 9000, plus N(0, 20)
  adc16x8    8 x uint16: eight 12-bit ADC channels, 2048 + A_c sin(2 pi t / P_c) + N(0, 3), clipped to [0, 4095]
  xyz32      3 x float32: a point walking through space, each coordinate a random walk of N(0, 0.001) steps from its own offset
  cplx64     complex64 (2 x float32): a slowly rotating phasor of slowly varying amplitude plus N(0, 1e-4)
  i32x4      4 x int32: four counters of different rates, the running sums of steps uniform in [-r_c, r_c]
For the fold alone (lag 1): series_datagen's adc16 and typed_datagen's smooth32."""
import numpy as np

KINDS = {"stereo16": (2, 2), "adc16x8": (2, 8), "xyz32": (4, 3), "cplx64": (4, 2), "i32x4": (4, 4)}     # name -> (elem, channels)
FOLD_ONLY = {"adc16": 2, "smooth32": 4}                                                                 # name -> elem (lag 1)


def lag_bytes(kind, n, seed=0x1a6):
    """n bytes of `kind` (whole frames of all channels, then cut to n)"""
    elem, ch = KINDS[kind]
    rng = np.random.Generator(np.random.Philox(key=seed))
    frames = n // (elem * ch) + 1
    t = np.arange(frames, dtype=np.float64)
    if kind == "stereo16":
        cols = [9000 * np.sin(2 * np.pi * t / 441 + 0.3) + rng.normal(0, 20, frames), 9000 * np.sin(2 * np.pi * t / 613 + 1.1) + rng.normal(0, 20, frames)]
        a = np.rint(np.stack(cols, axis=1)).astype("<i2")
    elif kind == "adc16x8":
        cols = [2048 + (200 + 150 * c) * np.sin(2 * np.pi * t / (500 + 130 * c) + c) + rng.normal(0, 3, frames) for c in range(8)]
        a = np.clip(np.rint(np.stack(cols, axis=1)), 0, 4095).astype("<u2")
    elif kind == "xyz32":
        a = (np.array([10.0, -250.0, 3000.0]) + np.cumsum(rng.normal(0, 0.001, (frames, 3)), axis=0)).astype("<f4")
    elif kind == "cplx64":
        z = (1.0 + 0.2 * np.sin(2 * np.pi * t / 9000)) * np.exp(2j * np.pi * t / 4000)
        a = np.stack([z.real + rng.normal(0, 1e-4, frames), z.imag + rng.normal(0, 1e-4, frames)], axis=1).astype("<f4")
    elif kind == "i32x4":
        cols = [np.cumsum(rng.integers(-r, r + 1, frames)) for r in (3, 40, 500, 6000)]
        a = np.stack(cols, axis=1).astype("<i4")
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)[:n].copy()


def fold_bytes(kind, n):
    """n bytes of a single-channel series whose differences change sign"""
    import series_datagen
    import typed_datagen
    if kind == "adc16":
        return np.ascontiguousarray(series_datagen.series_bytes("adc16", n))
    return np.frombuffer(typed_datagen.typed_bytes(kind, n), np.uint8).copy()
