"""The container's three decode entry points -- device buffers, host pointers, files -- share one walk over a stream's frames
(decode_walk in csrc/container_api.cpp); this fails if they ever stop agreeing.  For a container of each format version with a
full frame, a short frame and a tail, valid and broken in every part a walk looks at, the three return the same code and leave
the same (what, frame, block), which is also what the model's reader (tests/container_model.py) raises, and the same bytes for
the valid stream."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import container_model as M
import datagen
import series_datagen
import typed_datagen

pytestmark = pytest.mark.gpu

N, ROWS = 4096, 2
LENGTH = 3 * N + 3                                             # frames of 2 blocks, 1 block and a 3-byte tail
UNKNOWN = 9999
# version -> (elem, codec, delta) of the writer, and the input
WRITERS = {1: (0, 0, False), 2: (4, 0, False), 3: (2, 1, False), 4: (8, 1, True)}


def _input(version):
    if version == 1:
        return datagen.text_bytes(LENGTH, seed=7)
    if version == 4:
        return series_datagen.series_bytes("ts64", LENGTH + 8)[:LENGTH].copy()
    return typed_datagen.typed_bytes({2: "smooth32", 3: "quant16"}[version], LENGTH, seed=7)


def _flip(c, pos):
    b = bytearray(c)
    b[pos] ^= 0x20
    return bytes(b)


def _cases(c):
    """[(name, container)]: the valid stream and one fault in each part a walk looks at"""
    lay = M.layout(c)
    f0, f1, f2 = lay["frames"]
    assert [(f["nb"], f["blk_len"]) for f in (f0, f1, f2)] == [(2, N), (1, N), (1, 3)]
    s, e, _ = f0["records"][0]
    h = c[:16] + struct.pack("<Q", LENGTH + 1)
    return [("valid", c), ("stream header", _flip(c, 5)), ("frame 1 tables", _flip(c, f1["tables"][0] + 700)),
            ("frame 0 record", _flip(c, (s + e) // 2)), ("trailer", _flip(c, lay["trailer"] + 6)), ("last byte cut", c[:-1]),
            ("cut in frame 1", c[:f1["start"] + 40]),
            ("total + 1", h + struct.pack("<II", zlib.crc32(h), 0) + c[32:])]      # (the header CRC made right again)


def _model(cont):
    try:
        return M.read(cont)
    except M.ContainerError as e:
        return e.what, e.frame, e.block


@pytest.fixture(scope="module")
def plan(glc, cuda):
    ctx = glc.Cudpp()
    p = glc.Plan(ctx, glc.CUDPP_COMPRESS, N, rows=ROWS)
    yield p
    p.close()
    ctx.close()


def _device(glc, plan, cont, cap, tmp_path):
    import torch
    c = torch.from_numpy(np.frombuffer(cont, np.uint8).copy()).cuda()
    out = torch.empty(cap, dtype=torch.uint8, device=c.device)
    d_len = torch.zeros(1, dtype=torch.int64, device=c.device)
    rc = glc._ct().glcContainerDecompressDevice(plan.handle, c.data_ptr(), c.numel(), out.data_ptr(), cap, d_len.data_ptr())
    return rc, glc.container_last_error(plan), out[:int(d_len.item())].cpu().numpy().tobytes() if rc == glc.CUDPP_SUCCESS else None


def _host(glc, plan, cont, cap, tmp_path):
    a = np.frombuffer(cont, np.uint8).copy()
    out = np.zeros(cap, dtype=np.uint8)
    n = C.c_ulonglong(0)
    rc = glc._ct().glcContainerDecompress(plan.handle, a.ctypes.data, a.size, out.ctypes.data, cap, C.byref(n))
    return rc, glc.container_last_error(plan), out[:n.value].tobytes() if rc == glc.CUDPP_SUCCESS else None


def _file(glc, plan, cont, cap, tmp_path):
    src, dst = tmp_path / "in.glc", tmp_path / "out.bin"
    src.write_bytes(cont)
    rc = glc._ct().glcContainerDecompressFile(plan.handle, str(src).encode(), str(dst).encode())
    return rc, glc.container_last_error(plan), dst.read_bytes() if rc == glc.CUDPP_SUCCESS else None


@pytest.mark.parametrize("version", [1, 2, 3, 4])
def test_the_three_decode_entry_points_agree_with_each_other_and_the_model(glc, plan, version, tmp_path):
    elem, codec, delta = WRITERS[version]
    x = _input(version)
    c = M.write(x, N, ROWS, elem, codec, delta)
    assert struct.unpack("<HHII", c[4:16]) == (version, int(delta), N, elem)
    for name, cont in _cases(c):
        want = _model(cont)
        got = [entry(glc, plan, cont, LENGTH + 8, tmp_path) for entry in (_device, _host, _file)]
        print("version %d, %s: model %s, device / host / file %s" % (
            version, name, "decodes" if name == "valid" else want, [(rc, err) for rc, err, _ in got]))
        rcs, errs, outs = zip(*got)
        assert rcs[0] == rcs[1] == rcs[2], (version, name, rcs)
        assert errs[0] == errs[1] == errs[2], (version, name, errs)
        if name == "valid":
            assert rcs[0] == glc.CUDPP_SUCCESS and errs[0] == (0, -1, -1)
            assert outs[0] == outs[1] == outs[2] == x.tobytes() == want.tobytes()
        else:
            assert rcs[0] == UNKNOWN and errs[0] == want, (version, name, errs[0], want)
