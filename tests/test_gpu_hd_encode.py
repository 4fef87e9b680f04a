"""Row f3 encoded on the device (include/glc_hd.h: glcHdHistogramDevice, glcHdBuildTableDevice, glcHdEncodeDevice).

The histogram equals np.bincount, the table equals glcHdBuildTable's (and the reference's decoder-table layout built
from it), the stream equals glcHdEncodeHost's word for word and the oracle's bit-serial decoder reads it back; the
device-only round trip histogram -> table -> encode -> decode returns the input."""
import os

import numpy as np
import pytest

import hd_table_model as M
import oracle_lib as O
import test_hd

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_cuhd_gold.npz"))
GOLD_CASES = [str(c) for c in GOLD["cases"]]


def _dev(a, cuda, offset=0):
    """a uint8 cuda tensor holding `a`, starting `offset` bytes into a larger allocation"""
    import torch
    buf = torch.empty(a.size + offset + 16, dtype=torch.uint8, device=cuda)
    v = buf[offset:offset + a.size]
    v.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)))
    return v


def _hist(glc, d):
    import torch
    h = torch.full((256,), -12345, dtype=torch.int64, device=d.device)      # garbage: the call must overwrite it
    glc.hd_histogram_device(d, d_hist=h)
    torch.cuda.synchronize()
    return h.cpu().numpy().view(np.uint64)


def _tables(glc, hist, cuda):
    import torch
    d_hist = torch.from_numpy(np.asarray(hist, dtype=np.uint64).view(np.int64).copy()).to(cuda)
    return glc.hd_build_table_device(d_hist)


def _encode(glc, d, lens, codes, cuda, cap=None):
    """device encode with a host table uploaded; returns the stream as uint32 numpy"""
    import torch
    d_l = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.uint8)).to(cuda)
    d_c = torch.from_numpy(np.ascontiguousarray(codes, dtype=np.uint16).view(np.int16)).to(cuda)
    units, n = glc.hd_encode_device(d, d_l, d_c, cap_units=cap)
    torch.cuda.synchronize()
    return units[:int(n.item())].cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ histogram
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 4095, 4096, 4097, (1 << 20) + 3])
@pytest.mark.parametrize("offset", [0, 1, 2, 3, 7, 15])
def test_histogram_equals_bincount(glc, cuda, n, offset):
    a = np.random.default_rng(n * 31 + offset).binomial(255, 0.5, n).astype(np.uint8)
    assert np.array_equal(_hist(glc, _dev(a, cuda, offset)), np.bincount(a, minlength=256))


def test_histogram_large_and_degenerate(glc, cuda):
    import torch
    n = 300 * (1 << 20) + 5
    a = np.random.default_rng(3).integers(0, 256, n, dtype=np.uint8)
    assert np.array_equal(_hist(glc, _dev(a, cuda, 3)), np.bincount(a, minlength=256))
    del a
    torch.cuda.empty_cache()
    one = np.full(1_000_003, 0xAB, dtype=np.uint8)
    assert np.array_equal(_hist(glc, _dev(one, cuda, 1)), np.bincount(one, minlength=256))
    every = np.tile(np.arange(256, dtype=np.uint8), 4099)
    assert np.array_equal(_hist(glc, _dev(every, cuda, 2)), np.bincount(every, minlength=256))


# ---------------------------------------------------------------------------------------------------------------- table
def _all_table_histograms():
    import test_cpu_hd_table_model as T
    return [h for _, h in T.NAMED] + M.random_histograms()


def test_device_table_equals_host_builder(glc, cuda):
    import torch
    hs = _all_table_histograms()
    assert len(hs) >= 2000
    H = torch.from_numpy(np.stack(hs).view(np.int64)).to(cuda)
    N = len(hs)
    lens = torch.empty((N, 256), dtype=torch.uint8, device=cuda)
    codes = torch.empty((N, 256), dtype=torch.int16, device=cuda)
    tabs = torch.empty((N, 4096), dtype=torch.uint8, device=cuda)
    L = glc.lib()
    for i in range(N):
        assert L.glcHdBuildTableDevice(H[i].data_ptr(), lens[i].data_ptr(), codes[i].data_ptr(), tabs[i].data_ptr(), None) == 1
    torch.cuda.synchronize()
    gl, gc, gt = lens.cpu().numpy(), codes.cpu().numpy().view(np.uint16), tabs.cpu().numpy()
    for i, h in enumerate(hs):
        wl, wc = glc.hd_build_table(h)
        assert np.array_equal(gl[i], wl), i
        assert np.array_equal(gc[i], wc), i
        assert np.array_equal(gt[i], M.decoder_table(wl, wc)), i


def test_device_table_empty_and_without_decoder_table(glc, cuda):
    import torch
    lens, codes, tab = _tables(glc, np.zeros(256, dtype=np.uint64), cuda)
    torch.cuda.synchronize()
    assert not lens.any() and not codes.any() and not tab.any()
    h = np.bincount(test_hd.binomial_bytes(4096, 9), minlength=256)
    d_hist = torch.from_numpy(h.astype(np.int64)).to(cuda)
    lens, codes, tab = glc.hd_build_table_device(d_hist, table=False)
    torch.cuda.synchronize()
    wl, wc = glc.hd_build_table(h)
    assert tab is None and np.array_equal(lens.cpu().numpy(), wl) and np.array_equal(codes.cpu().numpy().view(np.uint16), wc)


# --------------------------------------------------------------------------------------------------------------- encode
def _encode_cases():
    cases = [(name, data, None) for name, data in test_hd.CASES]
    rng = np.random.default_rng(44)
    for i, h in enumerate(M.random_histograms()[:50]):
        present = np.nonzero(h)[0]
        p = h.astype(np.float64) / float(h.astype(np.float64).sum())
        d = np.concatenate([present.astype(np.uint8), rng.choice(256, int(rng.integers(1, 60_000)), p=p).astype(np.uint8)])
        cases.append(("random_%d" % i, rng.permutation(d), h))           # table of the histogram, not of the data
    for n in (4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 65535, 65536, 65537):
        cases.append(("binomial_%d" % n, test_hd.binomial_bytes(n, n), None))
    # 8-bit codes: n % 4 == 0 gives a stream of whole units, the others do not
    for n in (4096, 4097, 4098, 4099, 65536, 65539):
        cases.append(("uniform8_%d" % n, np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8), np.ones(256)))
    return cases


ENCODE = _encode_cases()


@pytest.mark.parametrize("name,data,hist", ENCODE, ids=[c[0] for c in ENCODE])
def test_device_stream_equals_host_stream(glc, cuda, name, data, hist):
    h = np.bincount(data, minlength=256).astype(np.uint64) if hist is None else np.asarray(hist, dtype=np.uint64)
    lens, codes = glc.hd_build_table(h)
    want = glc.hd_encode_host(data, lens, codes)
    for off in ((0, 1, 3, 7) if data.size < 100_000 else (0, 5)):
        got = _encode(glc, _dev(data, cuda, off), lens, codes, cuda)
        assert np.array_equal(got, want), (name, off)
    assert np.array_equal(O.hd_decode(got, lens, codes, data.size), data)
    bits = int(np.sum(np.bincount(data, minlength=256).astype(np.uint64) * lens.astype(np.uint64)))
    assert got.size == (bits + 31) // 32 + 1


def test_device_stream_past_2_to_32_bits(glc, cuda):
    """about 540 MiB of uniform bytes with 8-bit codes: 4.5 * 2^30 bits, so the tile offsets need 64 bits.  With a flat
    histogram the canonical code of a byte is the byte, so the stream is the input read as big-endian units."""
    import torch
    n = 540 * (1 << 20) + 3
    d = torch.randint(0, 256, (n,), dtype=torch.uint8, device=cuda)
    lens, codes = glc.hd_build_table(np.ones(256, dtype=np.uint64))
    assert (lens == 8).all() and np.array_equal(codes, np.arange(256))
    d_l = torch.from_numpy(lens).to(cuda)
    d_c = torch.from_numpy(codes.view(np.int16)).to(cuda)
    units, nu = glc.hd_encode_device(d, d_l, d_c)
    torch.cuda.synchronize()
    assert int(nu.item()) == (8 * n + 31) // 32 + 1
    nfull = n // 4
    b = d[:4 * nfull].view(nfull, 4).to(torch.int64)
    want = (b[:, 0] << 24) | (b[:, 1] << 16) | (b[:, 2] << 8) | b[:, 3]
    got = units[:nfull].to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(got, want)
    tail = d[4 * nfull:].cpu().numpy()
    last = 0
    for i, v in enumerate(tail):
        last |= int(v) << (24 - 8 * i)
    assert int(units[nfull].item()) & 0xFFFFFFFF == last and int(units[nfull + 1].item()) == 0


@pytest.mark.parametrize("name", GOLD_CASES)
def test_reference_table_gives_reference_units(glc, cuda, name):
    """the reference's own lens / codes (tests/golden/ref_cuhd_gold.npz) on its symbols: every unit of the reference's
    stream, except the unused low bits of the last data unit, which the reference fills from its last codeword and this
    library leaves zero"""
    sym = test_hd._ref_symbols(name)
    lens, codes = GOLD[name + "_lens"], GOLD[name + "_codes"].astype(np.uint16)
    ref = GOLD[name + "_units"].astype(np.uint32)
    got = _encode(glc, _dev(sym, cuda), lens, codes, cuda)
    assert got.size == ref.size
    bits = int(np.sum(np.bincount(sym, minlength=256).astype(np.uint64) * lens.astype(np.uint64)))
    last, used = (bits - 1) // 32, bits - 32 * ((bits - 1) // 32)
    keep = np.uint32((0xFFFFFFFF << (32 - used)) & 0xFFFFFFFF)
    assert np.array_equal(got[:last], ref[:last])
    assert got[last] == ref[last] & keep and got[last] & ~keep == 0
    assert np.array_equal(got[last + 1:], ref[last + 1:])


# ------------------------------------------------------------------------------------------------ device-only round trip
def _device_round_trip(glc, cuda, data, offset=0):
    import torch
    L = glc.lib()
    d = _dev(data, cuda, offset)
    d_hist = glc.hd_histogram_device(d)
    d_lens, d_codes, d_tab = glc.hd_build_table_device(d_hist)
    units, nu = glc.hd_encode_device(d, d_lens, d_codes)
    n_units = int(nu.item())                                   # the only host read of the round trip
    assert n_units > 0
    work = torch.empty(L.glcHdWorkBytes(n_units), dtype=torch.uint8, device=cuda)
    out = torch.empty(max(1, data.size), dtype=torch.uint8, device=cuda)
    assert L.glcHdDecodeDeviceTableOnDevice(units.data_ptr(), n_units, d_tab.data_ptr(), out.data_ptr(), data.size,
                                            work.data_ptr(), None) == 1
    torch.cuda.synchronize()
    assert np.array_equal(out[:data.size].cpu().numpy(), data)
    lens, codes = d_lens.cpu().numpy(), d_codes.cpu().numpy().view(np.uint16)
    back = glc.hd_decode_device(units[:n_units], lens, codes, data.size)
    torch.cuda.synchronize()
    assert np.array_equal(back.cpu().numpy(), data)
    return units[:n_units].cpu().numpy().view(np.uint32), lens, codes


@pytest.mark.parametrize("name,data,hist", ENCODE[:8] + ENCODE[-18:], ids=[c[0] for c in ENCODE[:8] + ENCODE[-18:]])
def test_device_only_round_trip(glc, cuda, name, data, hist):
    units, lens, codes = _device_round_trip(glc, cuda, data, offset=data.size % 7)
    assert np.array_equal(units, glc.hd_encode_host(data, lens, codes))


def test_device_only_round_trip_multi_chunk(glc, cuda):
    data = test_hd.binomial_bytes(40_000_003, 3)
    units, lens, codes = _device_round_trip(glc, cuda, data)
    assert units.size > 512 * 8192                              # the decoder walks more than one chunk
    assert np.array_equal(units, glc.hd_encode_host(data, lens, codes))


# ------------------------------------------------------------------------------------------------------------- failures
SENTINEL = 0x5A5AA5A5


def _encode_fails(glc, cuda, data, lens, codes, cap):
    import torch
    d_l = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.uint8)).to(cuda)
    d_c = torch.from_numpy(np.ascontiguousarray(codes, dtype=np.uint16).view(np.int16)).to(cuda)
    units = torch.full((cap + 64,), SENTINEL, dtype=torch.int32, device=cuda)
    _, nu = glc.hd_encode_device(_dev(data, cuda), d_l, d_c, cap_units=cap, d_units=units)
    torch.cuda.synchronize()
    assert int(nu.item()) == 0
    assert (units.cpu().numpy().view(np.uint32) == SENTINEL).all()


def test_failures_write_nothing(glc, cuda):
    data = test_hd.binomial_bytes(100_000, 5)
    lens, codes = glc.hd_build_table(np.bincount(data, minlength=256))
    need = glc.hd_encode_host(data, lens, codes).size
    _encode_fails(glc, cuda, data, lens, codes, need - 1)
    ok = _encode(glc, _dev(data, cuda), lens, codes, cuda, cap=need)                 # exactly enough
    assert ok.size == need
    other = np.bincount(data[data != data[77_777]], minlength=256)                  # a table without data[77_777]
    l2, c2 = glc.hd_build_table(other)
    _encode_fails(glc, cuda, data, l2, c2, need + 100)
    l3 = lens.copy()
    l3[data[4097]] = 12                                                             # longer than 11 bits
    _encode_fails(glc, cuda, data, l3, codes, need + 100)


def test_argument_checks(glc, cuda):
    import torch
    L = glc.lib()
    d = torch.zeros(64, dtype=torch.uint8, device=cuda)
    p = d.data_ptr()
    w = torch.empty(L.glcHdEncodeWorkBytes(64), dtype=torch.uint8, device=cuda)
    assert L.glcHdHistogramDevice(None, 5, p, None) == 0
    assert L.glcHdHistogramDevice(p, 5, None, None) == 0
    assert L.glcHdHistogramDevice(p, 1 << 40, p, None) == 0
    assert L.glcHdBuildTableDevice(None, p, p, None, None) == 0
    assert L.glcHdBuildTableDevice(p, None, p, None, None) == 0
    assert L.glcHdBuildTableDevice(p, p, None, None, None) == 0
    args = [p, 64, p, p, p, 64, p, w.data_ptr(), None]
    for i in (0, 2, 3, 4, 6, 7):
        a = list(args)
        a[i] = None
        assert L.glcHdEncodeDevice(*a) == 0, i
    a = list(args)
    a[1] = 1 << 40
    assert L.glcHdEncodeDevice(*a) == 0
    assert L.glcHdEncodeBound(0) == 1 and L.glcHdEncodeBound(3) == 3 and L.glcHdEncodeBound(1 << 20) == 11 * (1 << 15) + 1
    torch.cuda.synchronize()


def test_empty_input_writes_the_pad_unit(glc, cuda):
    import torch
    lens, codes = glc.hd_build_table(np.ones(256, dtype=np.uint64))
    units = torch.full((4,), 7, dtype=torch.int32, device=cuda)
    _, nu = glc.hd_encode_device(torch.empty(0, dtype=torch.uint8, device=cuda), torch.from_numpy(lens).to(cuda),
                                 torch.from_numpy(codes.view(np.int16)).to(cuda), d_units=units)
    torch.cuda.synchronize()
    assert int(nu.item()) == 1 and units.cpu().tolist() == [0, 7, 7, 7]


# -------------------------------------------------------------------------------------------------------------- streams
def test_two_streams_in_flight_and_repeatable(glc, cuda):
    import torch
    a = test_hd.binomial_bytes(3_000_001, 21)
    b = np.minimum(np.random.default_rng(22).zipf(1.3, 2_000_003) - 1, 255).astype(np.uint8)
    want = []
    for x in (a, b):
        lens, codes = glc.hd_build_table(np.bincount(x, minlength=256))
        want.append((glc.hd_encode_host(x, lens, codes), torch.from_numpy(lens).to(cuda), torch.from_numpy(codes.view(np.int16)).to(cuda)))
    da, db = _dev(a, cuda), _dev(b, cuda, 1)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    L = glc.lib()
    wa = torch.empty(L.glcHdEncodeWorkBytes(a.size), dtype=torch.uint8, device=cuda)     # one work buffer per stream
    wb = torch.empty(L.glcHdEncodeWorkBytes(b.size), dtype=torch.uint8, device=cuda)
    res = []
    for _ in range(3):
        ua, na = glc.hd_encode_device(da, want[0][1], want[0][2], stream=s1, work=wa)
        ub, nb = glc.hd_encode_device(db, want[1][1], want[1][2], stream=s2, work=wb)
        res.append((ua, na, ub, nb))
    torch.cuda.synchronize()
    for ua, na, ub, nb in res:
        assert np.array_equal(ua[:int(na.item())].cpu().numpy().view(np.uint32), want[0][0])
        assert np.array_equal(ub[:int(nb.item())].cpu().numpy().view(np.uint32), want[1][0])
