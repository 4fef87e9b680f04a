"""The inverse MTF on its own (-m gpu): glcMtfInverseBatch (k_imtf_pos_deque, k_imtf_scan, k_imtf_apply) against the
oracle's inverse MTF on CHOSEN index sequences.  Every byte string is a valid MTF sequence, and inside the decoder the
kernels only ever see MTF bytes of real BWT output, where the patterns below barely occur: index 255 at every step (every
entry comes out of the far half of the position deque, the count of its near half reaches 256), indices on the bitmap-word
boundaries, small indices that hit entries put at the front earlier in the same batch of 16 steps (the patch of the word
the next step has already loaded), lanes of one wave with different data and different chunk lengths."""
import functools

import numpy as np
import pytest

import oracle_lib as O

CHUNK = 4096                                                 # IMTF_CHUNK of csrc/decode.hip: MTF bytes per lane
SIZES = (1, 15, 16, 17, 255, 256, 257, 511, 512, 4095, 4096, 4097, 8191, CHUNK * 64, CHUNK * 64 + 1, CHUNK * 65 + 100, 1 << 20)
EVERY_INPUT_AT = (4097, CHUNK * 2 + 7)
EVERY_SIZE_WITH = ("const_255", "uniform")
GUARD = 64


def _zipf(n, rng):
    p = 1.0 / np.arange(1, 257) ** 1.2
    return rng.choice(256, size=n, p=p / p.sum())


def _const(k):
    return lambda n, rng: np.full(n, k)


INPUTS = {"const_%d" % k: _const(k) for k in (0, 1, 255, 15, 16, 63, 64, 127, 128, 191, 192, 254)}
INPUTS.update({
    "ramp_16": lambda n, rng: np.arange(n) % 16,                             # inside a batch of 16 steps: index = step
    "ramp_16_plus_1": lambda n, rng: np.arange(n) % 16 + 1,                  # ... and step + 1
    "alt_0_1": lambda n, rng: np.arange(n) % 2,
    "const_2": _const(2),
    "alt_255_0": lambda n, rng: np.where(np.arange(n) % 2 == 0, 255, 0),
    "far_then_random": lambda n, rng: np.concatenate([np.full(256, 255), rng.integers(0, 256, max(n, 256) - 256)])[:n],
    "uniform": lambda n, rng: rng.integers(0, 256, n),
    "random_0_3": lambda n, rng: rng.integers(0, 4, n),
    "zipf": _zipf,
})
# a chunk of each of the others in turn: the 64 lanes of a wave work on different data
INPUTS["patchwork"] = lambda n, rng: np.concatenate(
    [INPUTS[k](CHUNK, rng) for _, k in zip(range((n + CHUNK - 1) // CHUNK), _cycle())])[:n]


def _cycle():
    names = [k for k in INPUTS if k != "patchwork"]
    while True:
        yield from names


@functools.lru_cache(maxsize=None)
def case(name, n):
    """(MTF bytes, what the oracle makes of them), computed once per (input, size)"""
    x = np.ascontiguousarray(INPUTS[name](n, np.random.default_rng([n, len(name)])), dtype=np.uint8)
    assert x.size == n
    want = O.imtf(x)
    x.setflags(write=False); want.setflags(write=False)
    return x, want


def _pairs():
    out = [(k, n) for k in INPUTS for n in EVERY_INPUT_AT]
    out += [(k, n) for k in EVERY_SIZE_WITH for n in SIZES]
    # the index-against-step patterns and divergent lanes at a full wave, at a second wave with one live lane, and more
    out += [(k, n) for k in ("ramp_16", "ramp_16_plus_1", "patchwork") for n in (CHUNK * 64, CHUNK * 64 + 1, CHUNK * 65 + 100)]
    out += [("patchwork", 1 << 20), ("far_then_random", 8191), ("alt_255_0", CHUNK * 64 + 1)]
    return sorted(set(out), key=lambda p: (p[1], p[0]))


def list_model(x):
    """the inverse MTF in ten lines, independent of the oracle"""
    lst = list(range(256))
    out = []
    for j in x.tolist():
        c = lst.pop(j)
        out.append(c)
        lst.insert(0, c)
    return np.array(out, dtype=np.uint8)


def test_the_oracle_agrees_with_a_list_model():
    for name in INPUTS:
        for n in (1, 16, 257, 4097, 8191):
            x, want = case(name, n)
            assert np.array_equal(want, list_model(x)), (name, n)


def test_the_inputs_hold_the_patterns():
    x, _ = case("patchwork", CHUNK * 64)
    assert len({x[c * CHUNK:(c + 1) * CHUNK].tobytes() for c in range(64)}) >= len(INPUTS) - 1
    for name, first in (("ramp_16", 0), ("ramp_16_plus_1", 1)):
        x, _ = case(name, 4097)
        assert np.array_equal(x[:32], (np.arange(32) % 16) + first)
    x, _ = case("far_then_random", 4097)
    assert np.all(x[:256] == 255) and len(set(x[256:].tolist())) > 200


@pytest.fixture(scope="module")
def plan(glc, cuda):
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_COMPRESS, 1 << 20, rows=3) as p:
        yield p


def _inverse(glc, cuda, plan, x, n, nblk):
    import torch
    buf = torch.full((nblk * n + GUARD,), 0xA5, dtype=torch.uint8, device=cuda)
    glc.mtf_inverse_batch(plan, torch.from_numpy(np.array(x)).to(cuda), n, nblk, d_out=buf)
    plan.synchronize()
    got = buf.cpu().numpy()
    assert np.all(got[nblk * n:] == 0xA5), "the kernels wrote behind the last row"
    return got[:nblk * n]


@pytest.mark.gpu
@pytest.mark.parametrize("name,n", _pairs(), ids=["%s-%d" % p for p in _pairs()])
def test_single_block(glc, cuda, plan, name, n):
    x, want = case(name, n)
    got = _inverse(glc, cuda, plan, x, n, 1)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s, n = %d: %d bytes differ, the first at %d (chunk %d, step %d of it, index %d)" % (
        name, n, bad.size, bad[0], bad[0] // CHUNK, bad[0] % CHUNK, x[bad[0]])


@pytest.mark.gpu
@pytest.mark.parametrize("n", (4099, 70001))
@pytest.mark.parametrize("names", (("uniform", "const_255", "ramp_16_plus_1"), ("patchwork", "zipf", "alt_255_0")))
def test_batches_of_unaligned_rows_with_different_inputs(glc, cuda, plan, n, names):
    """rows 1 and 2 start at odd addresses (no 16-byte loads or stores), and each row holds another input"""
    rows = [case(k, n) for k in names]
    got = _inverse(glc, cuda, plan, np.concatenate([r[0] for r in rows]), n, len(rows))
    for b, (k, (_, want)) in enumerate(zip(names, rows)):
        assert np.array_equal(got[b * n:(b + 1) * n], want), (k, b)


@pytest.mark.gpu
def test_entry_checks(glc, cuda, plan):
    L = glc.lib()
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_MTF, 4096, rows=1) as mtf_plan:
        assert L.glcMtfInverseBatch(0, 0, 0, 4096, 1) == glc.CUDPP_ERROR_INVALID_HANDLE
        assert L.glcMtfInverseBatch(mtf_plan.handle, 0, 0, 4096, 1) == glc.CUDPP_ERROR_INVALID_PLAN
        assert L.glcMtfInverseBatch(plan.handle, 0, 0, 0, 1) == glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION
        assert L.glcMtfInverseBatch(plan.handle, 0, 0, (1 << 20) + 1, 1) == glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION
        assert L.glcMtfInverseBatch(plan.handle, 0, 0, 4096, 4) == glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION


@pytest.mark.gpu
def test_mtf_then_inverse_on_the_gpu_is_the_identity(glc, cuda, plan):
    """glcMtfBatch then glcMtfInverseBatch, 1 MiB of uniform bytes: the forward kernel's output has every index"""
    import torch
    n = 1 << 20
    x, _ = case("uniform", n)
    d_in = torch.from_numpy(np.array(x)).to(cuda)
    d_mtf = torch.empty_like(d_in)
    with glc.Cudpp() as ctx, glc.Plan(ctx, glc.CUDPP_MTF, n, rows=1) as fwd:
        assert glc.lib().glcMtfBatch(fwd.handle, d_in.data_ptr(), d_mtf.data_ptr(), n, 1) == 0
        fwd.synchronize()
    assert np.array_equal(d_mtf.cpu().numpy(), O.mtf(x))
    back = glc.mtf_inverse_batch(plan, d_mtf, n, 1)
    plan.synchronize()
    assert torch.equal(back, d_in)
