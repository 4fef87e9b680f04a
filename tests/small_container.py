"""One small container input and every encoder setting of the container with the CPU model that writes its bytes, shared by
test_gpu_scratch_fill.py and test_gpu_call_history.py.  The shape is the plain-C rigs' scaled down -- plan n = 4096, rows 4,
nine blocks and a ragged tail of 1203 bytes: two full frames, a frame of one block, the tail -- and the blocks are chosen so
that every mode writes the record kind it exists for.

On that input the filter rules of formats 13, 14 and 16 pick what format 10 picks -- no lag above 1, no width, no byte
candidate -- so those settings, and the hand-set byte predictor of format 15, have a second table, FILTERS: each entry with its own
plan shape, the input its feature exists for and the expected container (the golden fixtures; the byte-delta model).
entry(name) answers for the names of both tables.  Pure numpy and the models: no GPU."""
import functools
import os

import numpy as np

import ans_model
import auto_model
import choose_model
import container_model as M
import datagen
import dedup_model
import byte_delta_inputs
import byte_delta_model
import filter_auto_model
import filter_byte_inputs
import filter_byte_model
import filter_grid_inputs
import filter_grid_model
import filter_lag_inputs
import filter_lag_model
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


def _settings(glc, plan, codec=0, elem=0, delta=False, mode=None, lag=None, grid=None, filter_auto=False, filter_lag=False,
              filter_grid=False, filter_byte=False, byte_delta=None):
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
    if filter_lag:
        glc.container_set_filter_lag(plan, 1)
    if filter_grid:
        glc.container_set_filter_grid(plan, 1)
    if filter_byte:
        glc.container_set_filter_byte(plan, 1)
    if byte_delta:
        glc.container_set_byte_delta(plan, *byte_delta)


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


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BIG_N, BIG_ROWS, BIG_TAIL = 65536, 4, 3001                   # the shape of the 64 KiB entries; byte_delta: one full frame and this tail
_FILTER_AUTO = dict(codec=1, mode="auto", filter_auto=True)


def _fixture(name):
    return lambda: open(os.path.join(GOLDEN, name), "rb").read()


def _byte_delta_input(kind):
    x = (byte_delta_inputs.rgb8(BIG_N * BIG_ROWS + BIG_TAIL, 427) if kind == "rgb8" else
         byte_delta_inputs.grey8(BIG_N * BIG_ROWS + BIG_TAIL, 721))
    return x


# name -> (plan n, plan rows, the settings, the input, the expected container, the model's reader).  byte_delta is the hand-set
# predictor at (lag 3, stride 1281) on an RGB image 427 wide, byte_delta_lag at (1, 0) on a greyscale image
FILTERS = {
    "filter_lag": (filter_lag_inputs.N, filter_lag_inputs.ROWS, dict(_FILTER_AUTO, filter_lag=True), filter_lag_inputs.mixed_stream,
                   _fixture("filter_lag_v13_container.bin"), filter_lag_model.read),
    "filter_grid": (filter_grid_inputs.N, filter_grid_inputs.ROWS, dict(_FILTER_AUTO, filter_lag=True, filter_grid=True),
                    filter_grid_inputs.mixed_stream, _fixture("filter_grid_v14_container.bin"), filter_grid_model.read),
    "filter_byte": (filter_byte_inputs.N, filter_byte_inputs.ROWS, dict(_FILTER_AUTO, filter_lag=True, filter_grid=True, filter_byte=True),
                    filter_byte_inputs.mixed_stream, _fixture("filter_byte_v16_container.bin"), filter_byte_model.read),
    "byte_delta": (BIG_N, BIG_ROWS, dict(codec=1, mode="auto", byte_delta=(3, 1281)), lambda: _byte_delta_input("rgb8"),
                   lambda: byte_delta_model.write(_byte_delta_input("rgb8"), BIG_N, BIG_ROWS, 3, 1281), byte_delta_model.read),
    "byte_delta_lag": (BIG_N, BIG_ROWS, dict(codec=1, mode="auto", byte_delta=(1, 0)), lambda: _byte_delta_input("grey8"),
                       lambda: byte_delta_model.write(_byte_delta_input("grey8"), BIG_N, BIG_ROWS, 1, 0), byte_delta_model.read),
}
ALL = tuple(CONFIGS) + tuple(FILTERS)


def reset(glc, plan):
    """every container setting back to a new plan's, innermost first (off is always legal): what lets one plan go from one
    name of the tables to another"""
    glc.container_set_filter_byte(plan, 0)
    glc.container_set_filter_grid(plan, 0)
    glc.container_set_filter_lag(plan, 0)
    glc.container_set_byte_delta(plan, 0, 0)
    glc.container_set_filter_auto(plan, 0)
    glc.container_set_delta_grid(plan, 0, 0)
    glc.container_set_delta_lag(plan, 1, 0)
    for off in (glc.container_set_dedup, glc.container_set_auto, glc.container_set_ans, glc.container_set_sparse,
                glc.container_set_runs, glc.container_set_delta, glc.container_set_shuffle):
        off(plan, 0)
    glc.container_set_codec(plan, 0)


def configure(glc, plan, name, pipelined=False):
    plan.set_pipelining(pipelined)
    _settings(glc, plan, **(CONFIGS[name][0] if name in CONFIGS else FILTERS[name][2]))
    return plan


@functools.lru_cache(maxsize=None)
def want(name):
    """the model's container of data() under the setting `name`, computed once per process"""
    return CONFIGS[name][1](data())


@functools.lru_cache(maxsize=None)
def entry(name):
    """(plan n, plan rows, the input, the expected container) of a name of either table, made once per process"""
    if name in CONFIGS:
        return N, ROWS, data(), want(name)
    n, rows, _, make, expect, _ = FILTERS[name]
    x = make()
    x.setflags(write=False)
    return n, rows, x, expect()
