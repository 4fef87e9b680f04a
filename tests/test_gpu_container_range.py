"""Range reads of the container on the MI355X (-m gpu): for five writer settings the device, host and file forms of
glcContainerReadRange* return exactly x[a:a + c] for ranges at every edge the format has, with guards intact and the run statistics
of the model (tests/range_model.py); the golden fixtures of every format version are read in ranges; damage in one frame fails the
reads that touch it, with the full decode's triple, and no other; the index calls refuse what the full decode refuses, with the
same result and triple, on all three feeds; the file form touches only the stream header and the overlapped frames."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

import container_model as M
import datagen
import range_model as R
import series_datagen
import sparse_model as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ILLEGAL, UNKNOWN = 2, 9999
N = 4096
GUARD = 64
# name -> (codec, elem, delta, sparse, rows, input)
SETTINGS = {
    "bwt": (0, 0, False, False, 4, lambda n: datagen.text_bytes_fast(n)),
    "bwt_shuffle4": (0, 4, False, False, 4, lambda n: series_datagen.series_bytes("ctr32", n + 3)[:n]),
    "huff0": (1, 0, False, False, 4, lambda n: datagen.zipf_bytes(n)),
    "huff0_delta8": (1, 8, True, False, 8, lambda n: series_datagen.series_bytes("ts64", n + 7)[:n]),
    "huff0_sparse_delta2": (1, 2, True, True, 4, lambda n: series_datagen.series_bytes("adc16", n + 1)[:n]),
}


@pytest.fixture(scope="module")
def ctx(glc, cuda):
    c = glc.Cudpp()
    yield c
    c.close()


def _gpu(x):
    import torch
    return torch.from_numpy(np.array(np.frombuffer(bytes(x), np.uint8) if isinstance(x, (bytes, bytearray)) else x, dtype=np.uint8, copy=True)).cuda()


def _plan(glc, ctx, codec=1, elem=0, delta=False, sparse=True, rows=4):
    plan = glc.Plan(ctx, glc.CUDPP_COMPRESS, N, rows=rows)
    glc.container_set_shuffle(plan, elem)
    glc.container_set_codec(plan, codec)
    if delta:
        glc.container_set_delta(plan, 1)
    if sparse:
        glc.container_set_sparse(plan, 1)
    return plan


_MADE = {}


def _made(glc, ctx, name):
    """(input, container bytes) of a setting, written once by the GPU and checked against the model's reader"""
    if name not in _MADE:
        codec, elem, delta, sparse, rows, gen = SETTINGS[name]
        x = np.ascontiguousarray(gen(2 * rows * N + 2 * N + 777), dtype=np.uint8)
        assert x.size == 2 * rows * N + 2 * N + 777
        with _plan(glc, ctx, codec, elem, delta, sparse, rows) as plan:
            c = glc.container_compress(plan, _gpu(x)).cpu().numpy().tobytes()
        assert np.array_equal(S.read(c), x)
        assert [(f["nb"], f["blk_len"]) for f in M.layout(c)["frames"]] == [(rows, N), (rows, N), (2, N), (1, 777)]
        _MADE[name] = (x, c)
    return _MADE[name]


def _format(c):
    version, flags, _, elem = struct.unpack("<HHII", c[4:16])
    return version, flags, elem


def _ranges(x, rows, elem):
    L, F = x.size, rows * N
    e = max(elem, 1)
    return [(0, 0), (L // 2, 0), (0, 1), (L - 1, 1), (0, L), (N - 3, 7), (F - 5, 11), (2 * F - 5, 11), (2 * F + 2 * N - 5, 11),
            (L - 500, 300), (L - 3, 3), (12345, 6789), (2048 * e - 1, 2), (F + 2048 * e - 1, 2), (F + 2048 * e + 1, 1)]


def _frame_sizes(c):
    lay = M.layout(c)
    starts = [f["start"] for f in lay["frames"]] + [lay["trailer"]]
    return [starts[i + 1] - starts[i] for i in range(len(lay["frames"]))]


def _want_stats(c, a, n):
    """(frames, blocks, bytes) the model expects of a read of [a, a + n)"""
    frames = [(f["nb"], f["blk_len"]) for f in M.layout(c)["frames"]]
    nf, nblk = R.stats_of(frames, a, n, *_format(c))
    if n == 0:
        return 0, 0, 0
    fetched, pos = 32, 0
    for (nb, bl), size in zip(frames, _frame_sizes(c)):
        if max(a, pos) < min(a + n, pos + nb * bl):
            fetched += size
        pos += nb * bl
    return nf, nblk, fetched


def _read_guarded(glc, plan, ix, d_c, a, n, cuda, shift=3):
    """a device read into the middle of a guarded buffer, at an odd address; returns the bytes"""
    import torch
    buf = torch.full((GUARD + shift + n + GUARD,), 0xCD, dtype=torch.uint8, device=cuda)
    out = glc.container_read_range(plan, ix, d_c, a, n, out=buf[GUARD + shift: GUARD + shift + n] if n else buf[GUARD + shift: GUARD + shift + 1])
    h = buf.cpu().numpy()
    assert (h[:GUARD + shift] == 0xCD).all() and (h[GUARD + shift + n:] == 0xCD).all(), (a, n)
    assert out.numel() == n
    return h[GUARD + shift: GUARD + shift + n]


# --- 1. the three forms return the range, for every setting ---------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETTINGS))
def test_ranges_equal_slices_of_the_input(glc, ctx, cuda, tmp_path, name):
    codec, elem, delta, sparse, rows, _ = SETTINGS[name]
    x, c = _made(glc, ctx, name)
    d_c = _gpu(c)
    path = tmp_path / "c.glcb"
    path.write_bytes(c)
    with _plan(glc, ctx, rows=rows) as plan:
        with glc.container_index(plan, d_c) as ix:
            version, flags, el = _format(c)
            assert ix.info() == (x.size, N, 4, version, flags, el) and el == elem
            assert glc.container_last_error(plan) == (0, -1, -1)
            for a, n in _ranges(x, rows, elem):
                got = _read_guarded(glc, plan, ix, d_c, a, n, cuda)
                assert np.array_equal(got, x[a:a + n]), (name, a, n)
                assert glc.container_last_error(plan) == (0, -1, -1)
                assert glc.container_last_range_stats(plan) == _want_stats(c, a, n), (name, a, n)
            glc.container_read_range(plan, ix, d_c, 1000, 100)
            st = glc.container_last_range_stats(plan)
            assert st[0] == 1 and 32 < st[2] < len(c)             # a small read fetches less than the container
        # the host and file forms, each with an index of its own feed
        some = [(0, x.size), (rows * N - 5, 11), (x.size - 500, 300)]
        hc = np.frombuffer(c, np.uint8)
        with glc.container_index_host(plan, hc) as ixh, glc.container_index_file(plan, str(path)) as ixf:
            assert ixh.info() == ixf.info() == (x.size, N, 4, version, flags, el)
            for a, n in some:
                out = np.full(GUARD + n + GUARD, 0xCD, np.uint8)
                glc.container_read_range_host(plan, ixh, hc, a, n, out=out[GUARD:])
                assert np.array_equal(out[GUARD:GUARD + n], x[a:a + n]) and (out[:GUARD] == 0xCD).all() and (out[GUARD + n:] == 0xCD).all()
                assert glc.container_last_range_stats(plan) == _want_stats(c, a, n)
                out = np.full(GUARD + n + GUARD, 0xCD, np.uint8)
                glc.container_read_range_file(plan, ixf, str(path), a, n, out=out[GUARD:])
                assert np.array_equal(out[GUARD:GUARD + n], x[a:a + n]) and (out[:GUARD] == 0xCD).all() and (out[GUARD + n:] == 0xCD).all()
                assert glc.container_last_range_stats(plan) == _want_stats(c, a, n)
            # an index is an index: the one built from the file serves the device read
            assert np.array_equal(glc.container_read_range(plan, ixf, d_c, 77, 4321).cpu().numpy(), x[77:77 + 4321])
        # the full decode on the same plan still is what it was
        assert np.array_equal(glc.container_decompress(plan, d_c).cpu().numpy(), x)


def test_golden_fixtures_are_read_in_ranges(glc, ctx, cuda):
    for fn in ("container_v1.bin", "container_v2_f32.bin", "container_v3_mixed.bin", "container_v4_series.bin", "container_v5_sparse.bin"):
        gold = open(os.path.join(GOLDEN, fn), "rb").read()
        x = S.read(gold)
        d_c = _gpu(gold)
        L = x.size
        with _plan(glc, ctx, rows=2) as plan, glc.container_index(plan, d_c) as ix:
            assert ix.info()[0] == L and ix.info()[2] == len(M.layout(gold)["frames"])
            for a, n in [(0, L), (1, L - 2), (L - 1, 1), (N - 1, 2), (L // 3 | 1, 4097), (L - 700, 700), (min(2048 * 8, L - 2) - 1, 2)]:
                assert np.array_equal(_read_guarded(glc, plan, ix, d_c, a, n, cuda), x[a:a + n]), (fn, a, n)
                assert glc.container_last_range_stats(plan) == _want_stats(gold, a, n), (fn, a, n)
            hc = np.frombuffer(gold, np.uint8)
            assert np.array_equal(glc.container_read_range_host(plan, ix, hc, 5, L - 9), x[5:L - 4])


# --- 2. selectivity --------------------------------------------------------------------------------------------------------
def _full_decode_verdict(glc, plan, cont, cap):
    """(result, LastError) of glcContainerDecompressDevice on these bytes"""
    import torch
    d = _gpu(cont)
    out = torch.zeros(max(cap, 8), dtype=torch.uint8, device=d.device)
    d_len = torch.zeros(1, dtype=torch.int64, device=d.device)
    rc = glc._ct().glcContainerDecompressDevice(plan.handle, d.data_ptr(), d.numel(), out.data_ptr(), cap, d_len.data_ptr())
    return rc, glc.container_last_error(plan)


@pytest.mark.parametrize("name", ["bwt", "huff0_delta8"])
def test_damage_fails_the_reads_that_touch_it_and_no_other(glc, ctx, cuda, name):
    rows = SETTINGS[name][4]
    x, c = _made(glc, ctx, name)
    lay = M.layout(c)
    fr2 = lay["frames"][2]
    F = rows * N
    with _plan(glc, ctx, rows=rows) as plan:
        # a payload byte of frame 2, block 1
        s, e, _ = fr2["records"][1]
        bad = bytearray(c)
        bad[(s + e) // 2] ^= 0x20
        t0, t1 = fr2["tables"]
        tab = bytearray(c)
        tab[(t0 + t1) // 2] ^= 0x01
        for cont, want in ((bytes(bad), (3, 2, 1)), (bytes(tab), (2, 2, -1))):
            assert _full_decode_verdict(glc, plan, cont, x.size) == (UNKNOWN, want)
            d_c = _gpu(cont)
            with glc.container_index(plan, d_c) as ix:           # the index does not look at tables or records
                assert np.array_equal(_read_guarded(glc, plan, ix, d_c, 100, F - 200, cuda), x[100:F - 100])
                assert np.array_equal(_read_guarded(glc, plan, ix, d_c, F - 1, F + 1, cuda), x[F - 1:2 * F])
                assert glc.container_last_error(plan) == (0, -1, -1)
                for a, n in ((2 * F + 10, 5), (2 * F - 1, 2), (0, x.size), (2 * F + N + 1, 1)):       # (the last: block 1 alone, or block 0 alone)
                    with pytest.raises(glc.CudppError) as err:
                        glc.container_read_range(plan, ix, d_c, a, n)
                    assert err.value.code == UNKNOWN and glc.container_last_error(plan) == want, (a, n)
                with pytest.raises(glc.CudppError):
                    glc.container_read_range_host(plan, ix, np.frombuffer(cont, np.uint8), 2 * F + 10, 5)
                assert glc.container_last_error(plan) == want
                assert np.array_equal(glc.container_read_range(plan, ix, d_c, x.size - 777, 777).cpu().numpy(), x[-777:])
        # crc_all: a partial read cannot check it and does not -- the documented limit, asserted so that it is deliberate
        t = lay["trailer"]
        tr = bytearray(c[t:t + 12])
        tr[8] ^= 0x01
        cont = c[:t] + bytes(tr) + struct.pack("<I", zlib.crc32(bytes(tr)))
        assert _full_decode_verdict(glc, plan, cont, x.size) == (UNKNOWN, (4, -1, -1))
        d_c = _gpu(cont)
        with glc.container_index(plan, d_c) as ix:
            assert np.array_equal(glc.container_read_range(plan, ix, d_c, 0, x.size).cpu().numpy(), x)
            assert glc.container_last_error(plan) == (0, -1, -1)


# --- 3. the index refuses what the full decode refuses ----------------------------------------------------------------------
def _index_verdicts(glc, plan, cont, tmp_path):
    """[(result, LastError)] of the three index calls on these bytes; an index that was built is freed"""
    L = glc._ct()
    out = []
    d = _gpu(cont)
    h = np.frombuffer(cont, np.uint8)
    path = tmp_path / "idx.glcb"
    path.write_bytes(cont)
    for call in (lambda p: L.glcContainerIndexDevice(plan.handle, d.data_ptr(), d.numel(), p),
                 lambda p: L.glcContainerIndex(plan.handle, h.ctypes.data, h.size, p),
                 lambda p: L.glcContainerIndexFile(plan.handle, os.fsencode(str(path)), p)):
        p = C.c_void_p(None)
        rc = call(C.byref(p))
        out.append((rc, glc.container_last_error(plan)))
        assert (rc == 0) == bool(p.value)
        L.glcContainerIndexFree(p)
    return out


def test_index_failures_are_the_full_decodes(glc, ctx, cuda, tmp_path):
    x, c = _made(glc, ctx, "huff0_sparse_delta2")
    x1, c1 = _made(glc, ctx, "bwt")
    lay = M.layout(c1)
    magic = bytearray(c1)
    magic[lay["frames"][1]["start"]] ^= 0x01
    nb_zero = bytearray(c1)
    nb_zero[lay["frames"][2]["start"] + 4: lay["frames"][2]["start"] + 8] = struct.pack("<I", 0)
    cases = [("cut before the trailer", c1[:-20], (5, 3, -1)), ("cut inside frame 1", c1[:lay["frames"][1]["start"] + 40], (5, 1, -1)),
             ("cut inside the stream header", c1[:40], (5, -1, -1)), ("a bad frame magic", bytes(magic), (2, 1, -1)),
             ("nb = 0", bytes(nb_zero), (2, 2, -1)), ("stray bytes behind the trailer", c1 + b"\0" * 8, (1, 4, -1)),
             ("a bad stream magic", b"X" + c1[1:], (1, -1, -1))]
    with _plan(glc, ctx, rows=4) as plan:
        for what, cont, want in cases:
            full = _full_decode_verdict(glc, plan, cont, x1.size)
            assert full == (UNKNOWN, want), what
            assert _index_verdicts(glc, plan, cont, tmp_path) == [full] * 3, what
        assert _index_verdicts(glc, plan, c1, tmp_path) == [(0, (0, -1, -1))] * 3
    with _plan(glc, ctx, sparse=False, rows=4) as plan:              # a version-4 reader
        full = _full_decode_verdict(glc, plan, c, x.size)
        assert full == (UNKNOWN, (1, -1, -1))
        assert _index_verdicts(glc, plan, c, tmp_path) == [full] * 3
        with _plan(glc, ctx, rows=4) as reader, glc.container_index(reader, _gpu(c)) as ix:
            with pytest.raises(glc.CudppError) as err:              # ... also with an index another plan built
                glc.container_read_range(plan, ix, _gpu(c), 0, 10)
            assert err.value.code == UNKNOWN and glc.container_last_error(plan) == (1, -1, -1)
    with glc.Plan(ctx, glc.CUDPP_COMPRESS, 2048, rows=4) as small:   # a plan whose n is below the blocks' length
        full = _full_decode_verdict(glc, small, c1, x1.size)
        assert full[0] == ILLEGAL
        assert _index_verdicts(glc, small, c1, tmp_path) == [full] * 3


def test_argument_rules(glc, ctx, cuda):
    import torch
    rng = np.random.default_rng(3)
    # every byte value 16 times in every block: all code lengths 8, so every block is raw with the sparse mode on (version 5)
    # and off (version 3), and the two containers have one length
    x = np.concatenate([rng.permutation(np.repeat(np.arange(256, dtype=np.uint8), 16)) for _ in range(3)])
    with _plan(glc, ctx, codec=1, sparse=True) as pa, _plan(glc, ctx, codec=1, sparse=False) as pb:
        ca, cb = glc.container_compress(pa, _gpu(x)), glc.container_compress(pb, _gpu(x))
        assert {k for f in M.layout(ca.cpu().numpy().tobytes())["frames"] for _, _, k in f["records"]} == {M.RAW}
        assert ca.numel() == cb.numel() and _format(ca.cpu().numpy().tobytes()) != _format(cb.cpu().numpy().tobytes())
        with glc.container_index(pa, ca) as ixa:
            out = torch.full((x.size + GUARD,), 0xCD, dtype=torch.uint8, device=cuda)
            # a stale index: another container of equal length
            with pytest.raises(glc.CudppError) as err:
                glc.container_read_range(pa, ixa, cb, 0, 10, out=out)
            assert err.value.code == UNKNOWN and glc.container_last_error(pa) == (1, -1, -1)
            # a range past the end, a container of another length, no index
            for a, n in ((0, x.size + 1), (x.size, 1), (x.size + 1, 0), (1 << 63, 1 << 63), (5, (1 << 64) - 1)):
                rc = glc._ct().glcContainerReadRangeDevice(pa.handle, ixa.ptr, ca.data_ptr(), ca.numel(), a, n, out.data_ptr())
                assert rc == ILLEGAL, (a, n)
            with pytest.raises(glc.CudppError) as err:
                glc.container_read_range(pa, ixa, ca[:-8], 0, 10, out=out)
            assert err.value.code == ILLEGAL
            with pytest.raises(glc.CudppError) as err:
                glc.container_read_range(pa, None, ca, 0, 10, out=out)
            assert err.value.code == ILLEGAL
            assert bool((out == 0xCD).all())
            assert glc.container_read_range(pa, ixa, ca, x.size, 0).numel() == 0           # nothing, at the very end
            assert np.array_equal(glc.container_read_range(pa, ixa, ca, 0, 10, out=out).cpu().numpy(), x[:10])
            assert bool((out[10:] == 0xCD).all())
        # an empty input: an index of no frames, and a read of nothing
        empty = glc.container_compress(pa, _gpu(x[:0]))
        assert empty.numel() == 48
        with glc.container_index(pa, empty) as ix0, glc.container_index_host(pa, empty.cpu().numpy()) as ix0h:
            assert ix0.info()[:3] == ix0h.info()[:3] == (0, N, 0)
            assert glc.container_read_range(pa, ix0, empty, 0, 0).numel() == 0
            assert glc.container_last_range_stats(pa) == (0, 0, 0)
            with pytest.raises(glc.CudppError) as err:
                glc.container_read_range(pa, ix0, empty, 0, 1)
            assert err.value.code == ILLEGAL
        glc._ct().glcContainerIndexFree(None)                       # NULL is fine


# --- 4. what the file form touches ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bwt_shuffle4", "huff0_sparse_delta2"])
def test_the_file_form_reads_the_header_and_the_overlapped_frames_only(glc, ctx, cuda, tmp_path, name):
    rows = SETTINGS[name][4]
    x, c = _made(glc, ctx, name)
    lay = M.layout(c)
    starts = [f["start"] for f in lay["frames"]] + [lay["trailer"]]
    F = rows * N
    intact = tmp_path / "intact.glcb"
    intact.write_bytes(c)
    with _plan(glc, ctx, rows=rows) as plan, glc.container_index_file(plan, str(intact)) as ix:
        for a, n, frames in ((10, 100, [0]), (F - 3, 6, [0, 1]), (2 * F + 5, 2 * N + 100, [2, 3]), (x.size - 1, 1, [3])):
            blank = bytearray(b"\xff" * len(c))
            blank[:32] = c[:32]
            blank[lay["trailer"]:] = c[lay["trailer"]:]
            for f in frames:
                blank[starts[f]:starts[f + 1]] = c[starts[f]:starts[f + 1]]
            path = tmp_path / "blank.glcb"
            path.write_bytes(bytes(blank))
            assert np.array_equal(glc.container_read_range_file(plan, ix, str(path), a, n), x[a:a + n]), (a, n)
            assert glc.container_last_range_stats(plan)[0] == len(frames)
            assert np.array_equal(glc.container_read_range_host(plan, ix, np.frombuffer(bytes(blank), np.uint8), a, n), x[a:a + n])
            d_blank = _gpu(bytes(blank))
            assert np.array_equal(glc.container_read_range(plan, ix, d_blank, a, n).cpu().numpy(), x[a:a + n])
