"""Several plans, each driven by its own host thread on its own stream (-m gpu).

INTEGRATION.md promises it and bench.py --enc-threads / --dec-threads relies on it, and no other test has two plans in flight at
once.  Three Python threads start behind a barrier; each has its own Cudpp, plan and torch.cuda.Stream and does eight rounds
of encode, compare with the model's bytes, decode, compare (the library's calls release the GIL, so the three really overlap):

  1. a plan of n = 65536 on four text and four Zipf blocks, against the oracle
  2. the small container under auto, then dedup, then bwt_runs, the setting switched between rounds
  3. the mixed stream of format 16 against its fixture

Whatever process-wide state the library has -- pinned staging, lazily made tables, the kernels' first launches -- is shared by the
three; a result that depends on it differs from its model."""
import functools
import threading
import time

import numpy as np
import pytest

import datagen
import oracle_lib as O
import small_container as S
import stream_rig as R

pytestmark = pytest.mark.gpu
ROUNDS, JOIN_SECONDS = 8, 60
N = 65536


@functools.lru_cache(maxsize=None)
def _blocks():
    b = [datagen.text_bytes(N, seed=500 + i) for i in range(4)] + [datagen.zipf_bytes(N, seed=510 + i) for i in range(4)]
    return b, [O.compress(x) for x in b]


def _batch_rounds(glc, stream, pipelined, stop):
    import torch
    blocks, wants = _blocks()
    x = np.concatenate(blocks)
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, N, rows=len(blocks)) as plan:
        plan.set_stream(stream.cuda_stream)
        plan.set_pipelining(pipelined)
        d_in = torch.from_numpy(x.copy()).cuda()
        for rnd in range(ROUNDS):
            if stop.is_set():                                  # (the test has given up: start nothing more on the GPU)
                break
            out = glc.compress_batch(plan, d_in, N, len(blocks))
            plan.synchronize()
            got = R.to_host(out)
            for i, w in enumerate(wants):
                size = int(got["size"][i])
                assert size == w["size"] and int(got["bwt_index"][i]) == w["bwt_index"], (rnd, i)
                assert np.array_equal(got["words"][i * got["stride"]:i * got["stride"] + size].view(np.uint32), w["words"]), (rnd, i)
                assert np.array_equal(got["hist"][i * 256:(i + 1) * 256].view(np.uint32), w["hist"]), (rnd, i)
            back = glc.decompress_batch(plan, out, N, len(blocks))
            plan.synchronize()
            assert np.array_equal(R.to_host(back), x), rnd
        stream.synchronize()


def _container_rounds(names):
    def rounds(glc, stream, pipelined, stop):
        import torch
        n, rows = S.entry(names[0])[:2]
        with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, n, rows=rows) as plan:
            plan.set_stream(stream.cuda_stream)
            for rnd in range(ROUNDS):
                if stop.is_set():
                    break
                name = names[rnd % len(names)]
                _, _, x, want = S.entry(name)
                S.reset(glc, plan)
                S.configure(glc, plan, name, pipelined)
                c = glc.container_compress(plan, torch.from_numpy(x.copy()).cuda())
                assert R.to_host(c).tobytes() == want, (rnd, name)
                assert np.array_equal(R.to_host(glc.container_decompress(plan, c, cap=x.size)), x), (rnd, name)
                assert glc.container_last_error(plan) == (0, -1, -1)
            stream.synchronize()
    return rounds


SETS = (_batch_rounds, _container_rounds(("auto", "dedup", "bwt_runs")), _container_rounds(("filter_byte",)))


@pytest.mark.parametrize("pipelined", [False, True], ids=["serial", "pipelined"])
def test_three_plans_on_three_threads(glc, cuda, pipelined):
    import torch
    _blocks()                                                  # (the expected values, before the clock of the join starts)
    for name in ("auto", "dedup", "bwt_runs", "filter_byte"):
        S.entry(name)
    barrier = threading.Barrier(len(SETS), timeout=JOIN_SECONDS)
    errors = [None] * len(SETS)
    stop = threading.Event()                                   # set when the test gives up: the workers check it between rounds

    def run(i):
        try:
            torch.cuda.set_device(cuda)
            stream = torch.cuda.Stream()
            with torch.cuda.stream(stream):
                barrier.wait()
                SETS[i](glc, stream, pipelined, stop)
        except BaseException as e:                             # (reported by the main thread)
            errors[i] = e
            stop.set()                                         # (one failed: the others need not go on)

    threads = [threading.Thread(target=run, args=(i,), daemon=True) for i in range(len(SETS))]
    for t in threads:
        t.start()
    deadline = time.monotonic() + JOIN_SECONDS                 # one limit for the three together
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    alive = [i for i, t in enumerate(threads) if t.is_alive()]
    if alive:
        stop.set()
    assert not alive, "threads %r did not finish within %d s: nothing more is started on the GPU here" % (alive, JOIN_SECONDS)
    torch.cuda.synchronize()
    for i, e in enumerate(errors):
        if e is not None:
            raise AssertionError("thread %d (%s) failed: %r" % (i, SETS[i].__name__, e)) from e
