"""8-bit sample inputs for the container's byte predictor (INTEGRATION.md 4b "Delta: bytes", format version 15), each from one
np.random.Generator(np.random.Philox(key=...)) per call, as bytes.

  grey8(width)   a greyscale image in rows of `width` pixels: clip(rint(128 + 60 sin(x / 40) cos(y / 55) + 25 sin((x + 2 y) / 90)
                 + col[x] + N(0, 1)), 0, 255), col the mean-removed running sum of `width` steps uniform in [-6, 6]: a fixed column
                 pattern, as a detector's or a scanner's
  rgb8(width)    three such channels interleaved (row stride 3 * width bytes), their (offset, amplitude, px, py) (128, 60, 40, 55),
                 (100, 50, 23, 31) and (160, 40, 67, 19), each with its own column pattern
  stereo8        two interleaved u8 channels: sines of periods 441 and 613, amplitude 100 around 128, plus N(0, 1)
  text, noise    datagen's text and choose_inputs' noise: what the predictor is not for"""
import numpy as np

import choose_inputs
import datagen

CHANNELS = ((128, 60, 40, 55), (100, 50, 23, 31), (160, 40, 67, 19))


def _channel(rng, rows, width, off, amp, px, py):
    y, x = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    col = np.cumsum(rng.uniform(-6, 6, width))
    col -= col.mean()
    s = off + amp * np.sin(x / px) * np.cos(y / py) + 25 * np.sin((x + 2 * y) / 90) + col[None, :]
    return np.clip(np.rint(s + rng.normal(0, 1, s.shape)), 0, 255).astype(np.uint8)


def grey8(n, width, seed=0xb17e):
    """n bytes of the greyscale image in rows of `width` (whole rows, then cut to n)"""
    rng = np.random.Generator(np.random.Philox(key=seed))
    return _channel(rng, n // width + 1, width, *CHANNELS[0]).reshape(-1)[:n].copy()


def rgb8(n, width, seed=0xb17f):
    """n bytes of the RGB image in rows of `width` pixels, 3 * width bytes"""
    rng = np.random.Generator(np.random.Philox(key=seed))
    rows = n // (3 * width) + 1
    return np.stack([_channel(rng, rows, width, *c) for c in CHANNELS], axis=2).reshape(-1)[:n].copy()


def stereo8(n, seed=0xb180):
    rng = np.random.Generator(np.random.Philox(key=seed))
    frames = n // 2 + 1
    t = np.arange(frames, dtype=np.float64)
    cols = [128 + 100 * np.sin(2 * np.pi * t / p) + rng.normal(0, 1, frames) for p in (441, 613)]
    return np.clip(np.rint(np.stack(cols, axis=1)), 0, 255).astype(np.uint8).reshape(-1)[:n].copy()


def text(n):
    return np.ascontiguousarray(datagen.text_bytes_fast(n))


def noise(n, seed=0xb181):
    return np.ascontiguousarray(choose_inputs.block("noise", n, seed))
