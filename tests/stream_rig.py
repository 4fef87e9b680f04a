"""A rig that shows on which stream a call's work ran, for test_gpu_caller_streams.py and test_gpu_plan_threads.py.

On the null stream a launch, memset or copy that forgot its stream argument is invisible, and so is a host wait inside a call
that promises only to enqueue.  behind_the_gate() makes the target call on a non-blocking torch.cuda.Stream S, the plan set to
it, so that either mistake changes the bytes that come back or trips one of two events:

  1. prime      the call once on input A, waited for: every allocation is made (the measured call frees nothing) and A's
                intermediates lie in the library's scratch
  2. blocker    a device delay on the legacy default stream and an event behind it: a stage the library puts on stream 0
                cannot run until long after the results have been read
  3. gate       the input buffers hold a decoy D (B's bytes, every one flipped); on S a delay, an event, then the copy of
                the real input B over D: a stage that runs anywhere but behind S reads D, or A's leftovers
  4. the call   for an enqueue-only entry the gate's event must not have completed on return
  5. fetch      the outputs to the host on S, and S alone synchronised
  6. the blocker's event must still not have completed
  7. the device synchronised

S comes from independent_stream(): the runtime multiplexes streams onto a few in-order hardware queues, and a stream that shares
the null stream's queue would run behind the blocker whatever the library does.

A completed blocker or gate event FAILS the test -- something synchronised against the null stream, or the delays are too short
for this machine -- it never skips and never passes.  The caller compares what comes back with the CPU model's bytes for B.

The delay is torch.cuda._sleep, one workgroup that spins (the library's kernels run beside it), calibrated once per process
with events: no clock rate is assumed.  The sizes come from profiles/caller_streams.md: the gate is at least ten times the
slowest enqueue-only call's host time, the blocker the gate plus ten times the target call's wall time (ten times: the margin
for host scheduling on a shared machine), capped at one second so that a stage that does wait for the null stream costs a
second and not a hang."""
import functools

import numpy as np

# profiles/caller_streams.md: the slowest enqueue-only helper call took 0.08 ms of host time (the gate: 250 times that); the
# slowest target call's wall time by group, on the null stream without the rig
GATE_MS = 20.0
BLOCKER_CAP_MS = 1000.0
TARGET_MS = {"small": 8.5, "container": 9.5, "all_tiers": 105.5}    # ("small" takes in the container rows on the 4 KiB plans)


def blocker_ms(group):
    return min(BLOCKER_CAP_MS, GATE_MS + 10.0 * TARGET_MS[group])


@functools.lru_cache(maxsize=None)
def cycles_per_ms():
    """spin cycles of torch.cuda._sleep per millisecond, from the slope between two event-timed spins"""
    import torch
    assert hasattr(torch.cuda, "_sleep"), "this torch build has no torch.cuda._sleep"

    def timed(cycles):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    timed(1000)                                                # (the kernel's first launch loads its code object)
    lo, hi = 1_000_000, 11_000_000
    t_lo = min(timed(lo) for _ in range(3))
    t_hi = min(timed(hi) for _ in range(3))
    assert t_hi > t_lo > 0, "torch.cuda._sleep does not scale with its argument: %r ms, %r ms" % (t_lo, t_hi)
    return (hi - lo) / (t_hi - t_lo)


def delay(ms):
    """a spin of `ms` milliseconds queued on the current stream"""
    import torch
    torch.cuda._sleep(int(ms * cycles_per_ms()))


def decoy(b):
    """B with every byte flipped: same shape and type, equal to B nowhere"""
    return (~np.ascontiguousarray(b).view(np.uint8)).view(b.dtype).reshape(b.shape)


def to_host(out):
    """tensors -> numpy arrays through dicts, lists and tuples; copies run on the current stream and wait for it alone"""
    import torch
    if isinstance(out, torch.Tensor):
        return out.cpu().numpy()
    if isinstance(out, dict):
        return {k: to_host(v) for k, v in out.items()}
    if isinstance(out, (list, tuple)):
        return type(out)(to_host(v) for v in out)
    return out


def independent_stream(tries=16):
    """A torch.cuda.Stream whose work demonstrably runs while the null stream spins.  The runtime multiplexes the streams of a
    priority onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 by default), each strictly in order: a stream that happens to share
    the null stream's queue runs behind the blocker whatever the library does, and every run on it would end with the blocker
    completed.  So candidates are probed -- a short spin on the null stream, a marker on the candidate, which must complete
    before the spin does -- until one passes.  (The library's own side streams have the lowest priority, and with it hardware
    queues of their own.)"""
    import time
    import torch
    null = torch.cuda.default_stream()
    x = torch.zeros(1, device="cuda")
    cycles_per_ms()
    torch.cuda.synchronize()
    for _ in range(tries):
        s = torch.cuda.Stream()
        with torch.cuda.stream(null):
            delay(5.0)
            spun = torch.cuda.Event()
            spun.record(null)
        with torch.cuda.stream(s):
            x.add_(1)
            marker = torch.cuda.Event()
            marker.record(s)
        t0 = time.perf_counter()
        while not marker.query() and time.perf_counter() - t0 < 2e-3:
            pass
        beside = marker.query() and not spun.query()
        torch.cuda.synchronize()
        if beside:
            return s
    raise AssertionError("none of %d fresh streams ran beside the null stream: the rig cannot work here" % tries)


def shut_gate(stream, d_in, d_b):
    """step 3, on the current stream `stream`: the delay, the gate's event behind it, then the copies of the real inputs d_b over
    the decoys in d_in.  Returns the event: while it has not completed, nothing queued behind it has run."""
    import torch
    delay(GATE_MS)
    gate = torch.cuda.Event()
    gate.record(stream)
    for d, s in zip(d_in, d_b):
        d.copy_(s, non_blocking=True)
    return gate


def behind_the_gate(stream, call, a, b, group="small", enqueue_only=False, fetch=to_host, prime=None):
    """The protocol of the module's docstring.  `a` and `b` are lists of numpy arrays, the call's inputs for the priming and
    for the measured run (A may differ from B in size); call(*device tensors) makes the target call under
    torch.cuda.stream(stream) and returns its outputs, which fetch() brings to the host.  Returns what fetch() made of the
    measured call's outputs.  prime: what step 1 runs instead of call(*a), for calls whose input is host memory (nothing to
    gate: the call takes no arguments, and the priming call is one on another input)."""
    import torch
    up = lambda x: torch.from_numpy(np.array(x, copy=True)).cuda()
    null = torch.cuda.default_stream()
    assert stream.cuda_stream != 0 and null.cuda_stream == 0
    cycles_per_ms()                                            # (calibrated before anything is queued)
    with torch.cuda.stream(stream):
        fetch(prime() if prime else call(*[up(x) for x in a]))   # 1
        d_b = [up(x) for x in b]
        d_in = [up(decoy(x)) for x in b]
        stream.synchronize()
        blocked = torch.cuda.Event()
        with torch.cuda.stream(null):                          # 2
            delay(blocker_ms(group))
            blocked.record(null)
        gate = shut_gate(stream, d_in, d_b)                    # 3
        out = call(*d_in)                                      # 4
        gate_open = gate.query()
        got = fetch(out)                                       # 5
        stream.synchronize()
        blocker_done = blocked.query()                         # 6
    torch.cuda.synchronize()                                   # 7
    assert not blocker_done, ("the null-stream blocker of %g ms had completed when the results were read: something waited for "
                              "the null stream, or the delays are too short here -- this run proved nothing" % blocker_ms(group))
    if enqueue_only:
        assert not gate_open, ("the gate of %g ms on the caller's stream had opened when the enqueue-only call returned: the "
                               "call waited on the host, or the gate is too short here -- this run proved nothing" % GATE_MS)
    return got
