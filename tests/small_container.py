"""One small container input and every encoder setting of the container with the CPU model that writes its bytes, shared by
test_gpu_scratch_fill.py and test_gpu_call_history.py.  The shape is the plain-C rigs' scaled down -- plan n = 4096, rows 4,
nine blocks and a ragged tail of 1203 bytes: two full frames, a frame of one block, the tail -- and the blocks are chosen so
that every mode writes the record kind it exists for.  Pure numpy and the models: no GPU."""
import functools

import numpy as np

import ans_model
import auto_model
import choose_model
import container_model as M
import datagen
import dedup_model
import filter_auto_model
import grid_model
import lag_model
import runs_model
import sparse_model

N, ROWS, TAIL = 4096, 4, 1203
CHOOSE = 4                                                   # GLC_CONTAINER_CODEC_CHOOSE


@functools.lru_cache(maxsize=None)
def data():
    rng = np.random.default_rng(5)
    text = datagen.text_bytes(N, seed=1)
    ramp = (np.arange(N // 2, dtype=np.uint16) * 3 + 7).view(np.uint8)
    skew = np.where(rng.random(N) < 0.9, 0, rng.integers(1, 256, N)).astype(np.uint8)    # scattered: rANS beats the chunk mask
    parts = [text, datagen.zipf_bytes(N, seed=2), np.zeros(N, np.uint8), text,            # frame 0: a zero block, a repeated block
             rng.integers(0, 256, N, dtype=np.uint8), ramp, datagen.log_bytes(N, seed=3), datagen.float_bytes(N, seed=4),
             skew, datagen.text_bytes(TAIL, seed=10)]
    x = np.concatenate(parts)
    x.setflags(write=False)
    return x


def _settings(glc, plan, codec=0, elem=0, delta=False, mode=None, lag=None, grid=None, filter_auto=False):
    glc.container_set_shuffle(plan, elem)
    glc.container_set_codec(plan, codec)
    if mode:
        getattr(glc, "container_set_" + mode)(plan, 1)
    if delta:
        glc.container_set_delta(plan, 1)
    if lag:
        glc.container_set_delta_lag(plan, *lag)
    if grid:
        glc.container_set_delta_grid(plan, *grid)
    if filter_auto:
        glc.container_set_filter_auto(plan, 1)


# name -> (the settings of a plan that writes and reads it, the model's writer, a record kind the stream must hold or None)
CONFIGS = {
    "bwt": (dict(), lambda x: M.write(x, N, ROWS), M.HUFF),
    "bwt_runs": (dict(mode="runs"), lambda x: runs_model.write(x, N, ROWS), 4),
    "huff0": (dict(codec=1), lambda x: M.write(x, N, ROWS, 0, 1), 2),
    "sparse": (dict(codec=1, mode="sparse"), lambda x: sparse_model.write(x, N, ROWS), 3),
    "ans": (dict(codec=1, mode="ans"), lambda x: ans_model.write(x, N, ROWS), 5),
    "auto": (dict(codec=1, mode="auto"), lambda x: auto_model.write(x, N, ROWS), 5),
    "dedup": (dict(codec=1, mode="dedup"), lambda x: dedup_model.write(x, N, ROWS), 6),
    "choose": (dict(codec=CHOOSE), lambda x: choose_model.write(x, N, ROWS), None),
    "bwt_shuffle4": (dict(elem=4), lambda x: M.write(x, N, ROWS, 4), None),
    "huff0_shuffle4": (dict(codec=1, elem=4), lambda x: M.write(x, N, ROWS, 4, 1), None),
    "bwt_delta": (dict(elem=4, delta=True), lambda x: M.write(x, N, ROWS, 4, 0, delta=True), None),
    "huff0_delta": (dict(codec=1, elem=4, delta=True), lambda x: M.write(x, N, ROWS, 4, 1, delta=True), None),
    "lag": (dict(codec=1, mode="auto", elem=2, delta=True, lag=(2, 1)), lambda x: lag_model.write(x, N, ROWS, 2, 2, 1), None),
    "grid": (dict(codec=1, mode="auto", elem=2, delta=True, grid=(64, 0)), lambda x: grid_model.write(x, N, ROWS, 2, 64, 0), None),
    "filter_auto": (dict(codec=1, mode="auto", filter_auto=True), lambda x: filter_auto_model.write(x, N, ROWS), None),
}


def configure(glc, plan, name, pipelined=False):
    plan.set_pipelining(pipelined)
    _settings(glc, plan, **CONFIGS[name][0])
    return plan


@functools.lru_cache(maxsize=None)
def want(name):
    """the model's container of data() under the setting `name`, computed once per process"""
    return CONFIGS[name][1](data())
