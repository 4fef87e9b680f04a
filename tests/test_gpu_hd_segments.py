"""The batched order-0 Huffman kernels on the MI355X (-m gpu), alone, against the host encoder: glcHdSegmentsTablesDevice,
glcHdSegmentsEncodeDevice and glcHdSegmentsDecodeDevice (include/glc_hd.h) on segment sets that mix lengths 0 .. 1 MiB at odd
offsets and data kinds; canaries around every unit range and every output segment; the skip mask; thousands of segments in
one call; two encodes on two streams."""
import numpy as np
import pytest

import datagen

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 31, 4095, 4096, 4097, 70000, 1 << 20]
KINDS = ["zipf", "text", "one", "two", "uniform"]
CANARY_WORD = -1515870811                                      # 0xA5A5A5A5 as int32
CANARY_BYTE = 0xEE
GAP_UNITS = 3


def _data(kind, n, seed):
    if n == 0:
        return np.zeros(0, np.uint8)
    if kind == "zipf":
        return datagen.zipf_bytes(n, seed=seed)
    if kind == "text":
        return datagen.text_bytes_fast(n, seed=seed)
    if kind == "one":
        return np.full(n, 7 + seed % 200, np.uint8)
    if kind == "two":
        return np.where(np.random.default_rng(seed).random(n) < 0.9, 3, 250).astype(np.uint8)
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).astype(np.uint8)


def _segment_set(which):
    """(segments, offsets): every length with a data kind, the pairing rotated by `which`, at odd byte offsets"""
    segs = [_data(KINDS[(i + which) % len(KINDS)], n, 100 * which + i) for i, n in enumerate(LENGTHS)]
    segs += [_data(KINDS[(i + which + 2) % len(KINDS)], n, 100 * which + 50 + i) for i, n in enumerate(LENGTHS[1:6])]
    offs, cur = [], 1
    for i, s in enumerate(segs):
        offs.append(cur)
        cur += s.size + 1 + 2 * (i % 7)                         # odd gaps: every start has another alignment
    return segs, offs, cur + 5


def _host_stream(glc, seg):
    """(hist, lens, codes, units) the host makes for one segment; an empty one is the pad unit alone with an all-zero table"""
    hist = np.bincount(seg, minlength=256).astype(np.uint64)
    if seg.size == 0:
        return hist, np.zeros(256, np.uint8), np.zeros(256, np.uint16), np.zeros(1, np.uint32)
    lens, codes = glc.hd_build_table(hist)
    return hist, lens, codes, glc.hd_encode_host(seg, lens, codes)


def _upload(cuda, segs, offs, total):
    import torch
    buf = np.full(total, 0x5A, np.uint8)
    for s, o in zip(segs, offs):
        buf[o:o + s.size] = s
    return torch.from_numpy(buf).to(cuda)


@pytest.mark.parametrize("which", [0, 1, 3])
def test_tables_streams_skip_and_decode_against_the_host(glc, cuda, which):
    import torch
    segs, offs, total = _segment_set(which)
    count, max_len = len(segs), 1 << 20
    d_in = _upload(cuda, segs, offs, total)
    d_off, d_len = glc._i64(cuda, offs), glc._i64(cuda, [s.size for s in segs])
    hist, lens, codes, nunits = glc.hd_segments_tables(d_in, d_off, d_len, max_len)
    torch.cuda.synchronize()
    host = [_host_stream(glc, s) for s in segs]
    for i, (h, l, c, u) in enumerate(host):
        assert np.array_equal(hist[i].cpu().numpy().view(np.uint32), h.astype(np.uint32)), i
        assert np.array_equal(lens[i].cpu().numpy(), l), i
        assert np.array_equal(codes[i].cpu().numpy().view(np.uint16), c), i
        assert int(nunits[i]) == u.size, (i, int(nunits[i]), u.size)
    # unit ranges with canary words between them and behind the last one
    uoff, cur = [], GAP_UNITS
    for h in host:
        uoff.append(cur)
        cur += h[3].size + GAP_UNITS
    d_uoff = glc._i64(cuda, uoff)
    skip = np.zeros(count, np.int32)
    skip[[2, 5, count - 1]] = 1
    for use_skip in (False, True):
        d_units = torch.full((cur,), CANARY_WORD, dtype=torch.int32, device=cuda)
        d_skip = torch.from_numpy(skip).to(cuda) if use_skip else None
        glc.hd_segments_encode(d_in, d_off, d_len, max_len, lens, codes, nunits, d_units, d_uoff, d_skip=d_skip)
        torch.cuda.synchronize()
        got = d_units.cpu().numpy().view(np.uint32)
        want = np.full(cur, 0xA5A5A5A5, np.uint32)
        for i, h in enumerate(host):
            if not (use_skip and skip[i]):
                want[uoff[i]:uoff[i] + h[3].size] = h[3]
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (use_skip, bad[:8], [i for i in range(count) if uoff[i] <= bad[0]][-1])
    # decode: canary bytes around every output segment
    ooff, ocur = [], 3
    for s in segs:
        ooff.append(ocur)
        ocur += s.size + 5
    d_out = torch.full((ocur,), CANARY_BYTE, dtype=torch.uint8, device=cuda)
    glc.hd_segments_decode(d_units, d_uoff, nunits, hist, d_out, glc._i64(cuda, ooff), d_len, max_len, d_skip=d_skip)
    torch.cuda.synchronize()
    want = np.full(ocur, CANARY_BYTE, np.uint8)
    for i, s in enumerate(segs):
        if not skip[i]:
            want[ooff[i]:ooff[i] + s.size] = s
    assert np.array_equal(d_out.cpu().numpy(), want)


def test_capacity_leaves_a_segment_that_would_pass_it_alone(glc, cuda):
    import torch
    segs = [_data("zipf", 5000, 1), _data("text", 9000, 2), _data("zipf", 4096, 3)]
    offs, total = [0, 5001, 14002], 18100
    d_in = _upload(cuda, segs, offs, total)
    d_off, d_len = glc._i64(cuda, offs), glc._i64(cuda, [s.size for s in segs])
    hist, lens, codes, nunits = glc.hd_segments_tables(d_in, d_off, d_len, 9000)
    host = [_host_stream(glc, s)[3] for s in segs]
    uoff = np.concatenate([[0], np.cumsum([h.size for h in host])]).astype(np.int64)
    cap = int(uoff[2]) - 1                                      # segment 1 ends one unit past it, segment 2 lies behind it
    d_units = torch.full((int(uoff[3]) + 4,), CANARY_WORD, dtype=torch.int32, device=cuda)
    glc.hd_segments_encode(d_in, d_off, d_len, 9000, lens, codes, nunits, d_units, glc._i64(cuda, uoff[:3]), cap_units=cap)
    torch.cuda.synchronize()
    got = d_units.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:host[0].size], host[0]) and bool((got[host[0].size:] == 0xA5A5A5A5).all())


def test_thousands_of_segments_in_one_call(glc, cuda):
    import torch
    count, seg = 2304, 64 << 10
    g = torch.Generator(device=cuda)
    g.manual_seed(5)
    d_in = (torch.rand(count * seg, device=cuda, generator=g).pow(4) * 256).to(torch.uint8)     # skewed bytes
    d_in[7 * seg:9 * seg] = 65                                   # two one-symbol segments
    d_off = torch.arange(count, dtype=torch.int64, device=cuda) * seg
    d_len = torch.full((count,), seg, dtype=torch.int64, device=cuda)
    hist, lens, codes, nunits = glc.hd_segments_tables(d_in, d_off, d_len, seg)
    bits = (hist.to(torch.int64) * lens.to(torch.int64)).sum(1)
    assert torch.equal(nunits, (bits + 31) // 32 + 1)
    assert torch.equal(hist.to(torch.int64).sum(1), d_len)
    uoff = torch.cumsum(nunits, 0) - nunits
    total = int(nunits.sum())
    d_units = torch.full((total + 2,), CANARY_WORD, dtype=torch.int32, device=cuda)
    work = glc.hd_segments_work(count, seg, cuda)
    glc.hd_segments_encode(d_in, d_off, d_len, seg, lens, codes, nunits, d_units, uoff, cap_units=total, work=work)
    torch.cuda.synchronize()
    assert bool((d_units[total:] == CANARY_WORD).all())
    x = d_in.cpu().numpy()
    for i in (0, 7, 8, 1000, count - 1):                        # word for word against the host, for a sample
        h = _host_stream(glc, x[i * seg:(i + 1) * seg])
        assert np.array_equal(lens[i].cpu().numpy(), h[1])
        assert np.array_equal(d_units[int(uoff[i]):int(uoff[i]) + int(nunits[i])].cpu().numpy().view(np.uint32), h[3]), i
    d_out = torch.full((count * seg + 16,), CANARY_BYTE, dtype=torch.uint8, device=cuda)
    glc.hd_segments_decode(d_units, uoff, nunits, hist, d_out, d_off, d_len, seg, work=work)
    torch.cuda.synchronize()
    assert torch.equal(d_out[:count * seg], d_in) and bool((d_out[count * seg:] == CANARY_BYTE).all())


def test_two_encodes_on_two_streams_equal_one_after_the_other(glc, cuda):
    import torch
    sets = []
    for which in (0, 2):
        segs, offs, total = _segment_set(which)
        d_in = _upload(cuda, segs, offs, total)
        d_off, d_len = glc._i64(cuda, offs), glc._i64(cuda, [s.size for s in segs])
        hist, lens, codes, nunits = glc.hd_segments_tables(d_in, d_off, d_len, 1 << 20)
        uoff = torch.cumsum(nunits, 0) - nunits
        sets.append((d_in, d_off, d_len, lens, codes, nunits, uoff, int(nunits.sum())))
    torch.cuda.synchronize()

    def run(streams):
        outs, works = [], []
        for (d_in, d_off, d_len, lens, codes, nunits, uoff, total), st in zip(sets, streams):
            d_units = torch.full((total,), CANARY_WORD, dtype=torch.int32, device=cuda)
            torch.cuda.synchronize()
            works.append(glc.hd_segments_encode(d_in, d_off, d_len, 1 << 20, lens, codes, nunits, d_units, uoff, stream=st))
            outs.append(d_units)
            if st is None:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        return outs

    serial = run([None, None])
    overlapped = run([torch.cuda.Stream(device=cuda), torch.cuda.Stream(device=cuda)])
    for a, b in zip(serial, overlapped):
        assert torch.equal(a, b)
