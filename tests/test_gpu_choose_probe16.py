"""k_ch_probe16, the one-pass bigram probe for segments of up to 65 536 bytes (csrc/choose.hip), on the MI355X (-m gpu): the four
words {S2, SR, SC, M} of glcBigramProbeSegments against tests/choose_model.stats, exactly -- at L = 0, 1, 2, 3, 2047, 2048, 4101,
65535 and 65536 through the new kernel and at 65537 through k_ch_probe (max_len picks the kernel), with the segments starting on
a 16-byte boundary and 3 bytes behind one, over noise, text, one byte value (a cell of 65 534 at L = 65536: the largest a 16-bit
half holds here), two alternating values and a block of zeros with a few other bytes; several segments in one call with max_len
cutting the longer ones; the output rows pre-filled with 0xA5."""
import numpy as np
import pytest

import choose_inputs as CI
import choose_model as CM

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 3, 2047, 2048, 4101, 65535, 65536)
SPAN = 65568                                                      # bytes a content has: 65537 behind a start of up to 19, rounded up to 16
FILL = 0xA5A5A5A5A5A5A5A5 - (1 << 64)


def _contents():
    rng = np.random.default_rng(16)
    sparse = np.zeros(SPAN, np.uint8)
    sparse[rng.integers(0, SPAN, 40)] = rng.integers(1, 256, 40)
    return {"noise": rng.integers(0, 256, SPAN, dtype=np.uint8), "text": CI.block("text", SPAN, 3),
            "one": np.full(SPAN, 0x41, np.uint8), "two": np.tile(np.array([7, 200], np.uint8), SPAN // 2), "sparse": sparse}


@pytest.fixture(scope="module")
def data(cuda):
    """(host bytes, device bytes, {name: offset}): the contents back to back, each on a 16-byte boundary"""
    import torch
    c = _contents()
    host = np.concatenate(list(c.values()))
    return host, torch.from_numpy(host).cuda(), {k: i * SPAN for i, k in enumerate(c)}


_WANT = {}


def _want(host, off, L):
    if (off, L) not in _WANT:
        _WANT[(off, L)] = CM.stats(host[off:off + L])
    return _WANT[(off, L)]


def _run(glc, data, segs, max_len):
    """the probe over segs [(offset, length)] in one call, into rows pre-filled with 0xA5; checked against the model"""
    import torch
    host, dev, _ = data
    stats = torch.full((len(segs) + 1, 4), FILL, dtype=torch.int64, device=dev.device)
    got = glc.bigram_probe_segments(dev, [o for o, _ in segs], [n for _, n in segs], max_len=max_len, stats=stats)
    torch.cuda.synchronize()
    rows = [tuple(int(v) for v in r) for r in got.cpu().tolist()]
    for (o, n), r in zip(segs, rows):
        assert r == _want(host, o, min(n, max_len)), (o, n, max_len)
    assert [int(v) for v in stats[len(segs)].cpu().tolist()] == [FILL] * 4      # nothing behind the last row
    return rows


def test_the_largest_cell_is_what_a_half_holds():
    assert CM.stats(np.full(65536, 0x41, np.uint8)) == (65534 * 65533,) * 3 + (65534,) and 65534 < 1 << 16


@pytest.mark.parametrize("start", [0, 3])
def test_every_length_and_content_through_the_one_pass_kernel(glc, data, start):
    _, _, at = data
    segs = [(at[k] + start, L) for k in at for L in LENGTHS]
    rows = _run(glc, data, segs, 65536)
    one = rows[list(at).index("one") * len(LENGTHS) + LENGTHS.index(65536)]
    assert one == (65534 * 65533,) * 3 + (65534,)


@pytest.mark.parametrize("start", [0, 3])
def test_65537_is_still_right_through_the_two_pass_kernel(glc, data, start):
    _, _, at = data
    _run(glc, data, [(at[k] + start, L) for k in at for L in (65537, 65536, 4101)], 65537)


def test_max_len_cuts_the_longer_segments(glc, data):
    _, _, at = data
    for max_len in (4101, 2048, 65536, 3, 2):
        _run(glc, data, [(at[k] + s, L) for k in at for s, L in ((0, 65537), (3, 5000), (16, 2047), (19, 1 << 40))], max_len)


def test_the_two_kernels_agree_on_the_same_segments(glc, data):
    _, _, at = data
    segs = [(at[k] + s, L) for k in at for s in (0, 3) for L in (3, 2048, 4101, 65536)]
    assert _run(glc, data, segs, 65536) == _run(glc, data, segs, 65537)
