"""CPU suite (-m "not gpu"): pins the oracle to the committed golden vectors that
came from the reference's own gold routine, checks the domain's size-independent
properties on the oracle, and checks the C-ABI library without touching a GPU."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import datagen
import oracle_lib as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLD)
import make_ref_live_gold as LG  # noqa: E402  (the inputs of ref_live_gold.npz)

# what the reference's own CPU routines produced on LG's inputs (tests/golden/make_ref_live_gold.py): the "live" tests below
# check the oracle against it everywhere, and run the routines again where oracle/_ref was built
LIVE = np.load(os.path.join(GOLD, "ref_live_gold.npz"))


@pytest.fixture(scope="module")
def small():
    return np.load(os.path.join(GOLD, "ref_gold_small.npz"))


@pytest.fixture(scope="module")
def kats():
    return np.load(os.path.join(GOLD, "stream_kats.npz"))


# ---------------------------------------------------------------- golden ----
@pytest.mark.parametrize("n", [39, 128, 256, 512, 513, 1000, 1024, 1025, 32768, 45537, 65536])
def test_suffix_array_matches_reference_gold(small, n):
    assert np.array_equal(O.suffix_array(small["sa_in_%d" % n]), small["sa_out_%d" % n])


@pytest.mark.parametrize("n", [39, 128, 1000, 1025, 45537, 65536])
def test_bwt_and_mtf_match_reference_gold(small, n):
    x = small["bwt_in_%d" % n]
    b, idx = O.bwt(x)
    assert idx == int(small["bwt_idx_%d" % n][0])
    assert np.array_equal(b, small["bwt_out_%d" % n])
    assert np.array_equal(O.mtf(x), small["mtf_of_in_%d" % n])


def test_textbook_strings(small):
    for name, s in (("mississippi", b"mississippi"), ("banana", b"banana")):
        assert np.array_equal(O.suffix_array(s), small["str_%s_sa" % name])
        b, idx = O.bwt(s)
        assert np.array_equal(b, small["str_%s_bwt" % name]) and idx == int(small["str_%s_idx" % name][0])
    assert bytes(O.bwt(b"mississippi")[0]) == b"pssmipissii"


def test_reference_1m_vectors_known_answers():
    """reference gold on the reference's own 1 MiB test inputs"""
    j = json.load(open(os.path.join(GOLD, "ref_gold_1m.json")))
    x = O.glibc_rand_bytes(1 << 20, 255)
    assert "%08x" % O.crc32(x) == j["bwtTest"]["crc_in"] == "e8f0a761"
    b, idx = O.bwt(x)
    assert idx == j["bwtTest"]["bwt_index"] == 296638
    assert "%08x" % O.crc32(b) == j["bwtTest"]["crc_bwt"] == "bd22be99"
    assert "%08x" % O.crc32(O.mtf(b)) == j["bwtTest"]["crc_mtf"] == "1c647b66"
    assert "%08x" % O.crc32(O.suffix_array(x).view(np.uint8)) == j["bwtTest"]["crc_sa"]
    x[-1] = 0
    r = O.compress(x)
    s = j["compressTest_stream_restatement"]
    assert r["bwt_index"] == j["compressTest"]["bwt_index"]
    assert r["size"] == s["size_words"] == 262491
    assert "%08x" % O.crc32(r["words"].view(np.uint8)) == s["crc_words"]
    assert "%08x" % O.crc32(r["offsets"].view(np.uint8)) == s["crc_offsets"]
    assert "%08x" % O.crc32(r["hist"].view(np.uint8)) == s["crc_hist"]
    # gold decoder semantics (test_compress.cpp:240-311) give the input back
    assert np.array_equal(O.decompress(r["bwt_index"], r["hist"], r["offsets"], r["words"], x.size), x)


def test_oracle_vs_live_reference_gold():
    for n, mod in LG.SA_CASES:
        x = O.glibc_rand_bytes(n, mod)
        sa = O.suffix_array(x)
        assert sa.size == n and O.crc32(sa.view(np.uint8)) == int(LIVE["sa_crc_%d_%d" % (n, mod)])
        if O.have_ref_gold():
            assert np.array_equal(sa, O.ref_sa_gold(x))


def test_stream_kats_do_not_drift(kats):
    r = O.compress(kats["huff_in"])
    assert r["bwt_index"] == int(kats["huff_idx"][0])
    assert np.array_equal(r["words"], kats["huff_words"]) and np.array_equal(r["offsets"], kats["huff_offsets"])
    assert np.array_equal(r["hist"], kats["huff_hist"])
    c = O.lzss_candidates(kats["lz_in"])
    assert np.array_equal(c, kats["lz_cand"])
    assert np.array_equal(O.lzss_pack(c, kats["lz_in"].size), kats["lz_packed"])


# ------------------------------------------------------------ properties ----
def _naive_sa(x):
    b = bytes(x)        # symbols are byte+1, the sentinel 0 ends every suffix (sa_kernel.cuh:55-58)
    return np.array(sorted(range(len(b)), key=lambda i: [c + 1 for c in b[i:]] + [0]), dtype=np.uint32)


@pytest.mark.parametrize("case", ["random", "zeros", "period2", "period3tail", "twosym", "text"])
def test_suffix_array_against_naive_sort(case):
    rng = np.random.default_rng(3)
    x = {"random": rng.integers(0, 256, 700, dtype=np.uint8), "zeros": np.zeros(300, dtype=np.uint8),
         "period2": np.tile(np.array([1, 2], dtype=np.uint8), 200),
         "period3tail": np.concatenate([np.tile(np.array([9, 0, 0], dtype=np.uint8), 100), np.zeros(7, dtype=np.uint8)]),
         "twosym": rng.integers(0, 2, 600, dtype=np.uint8), "text": datagen.text_bytes(800)}[case]
    assert np.array_equal(O.suffix_array(x), _naive_sa(x))


@pytest.mark.parametrize("gen,n", [("zipf", 70001), ("text", 131072), ("float", 65536), ("zeros", 5000), ("one", 1)])
def test_bwt_mtf_inverses(gen, n):
    x = {"zipf": datagen.zipf_bytes, "text": datagen.text_bytes, "float": datagen.float_bytes,
         "zeros": lambda k: np.zeros(k, dtype=np.uint8), "one": lambda k: np.array([200], dtype=np.uint8)}[gen](n)
    b, idx = O.bwt(x)
    assert np.array_equal(np.sort(b), np.sort(x))                         # a permutation of the input
    assert np.array_equal(O.ibwt(b, idx), x)
    m = O.mtf(b)
    assert np.array_equal(O.imtf(m), b)


def test_mtf_definition_small():
    assert O.mtf(np.array([0, 0, 1, 1, 0, 255], dtype=np.uint8)).tolist() == [0, 0, 1, 0, 1, 255]
    assert O.mtf(np.array([3, 3, 3, 2, 3], dtype=np.uint8)).tolist() == [3, 0, 0, 3, 1]


def test_huffman_codes_are_a_prefix_code_with_reference_tie_breaks():
    # two symbols + EOF: counts 5, 5, EOF=1 -> first merge takes (EOF, then the lower-index of the 5s)
    hist = np.zeros(256, dtype=np.uint32); hist[10] = 5; hist[20] = 5
    codes, lens, n = O.huff_codes(hist)
    assert n == 3
    # min1 = EOF(count 1, slot 2) -> left, min2 = slot 0 (sym 10) -> right; then composite(6) vs sym 20 (5):
    # min1 = sym20 (count 5) left, min2 = composite right  => sym20 = '0', EOF = '10', sym10 = '11'
    assert (lens[20], codes[20]) == (1, 0) and (lens[256], codes[256]) == (2, 0b10) and (lens[10], codes[10]) == (2, 0b11)
    # Kraft equality for a full binary tree
    rng = np.random.default_rng(5)
    hist = rng.integers(0, 1000, 256).astype(np.uint32)
    codes, lens, n = O.huff_codes(hist)
    present = [s for s in range(257) if (hist[s] if s < 256 else 1) > 0]
    assert abs(sum(2.0 ** -int(lens[s]) for s in present) - 1.0) < 1e-12
    as_str = sorted(format(int(codes[s]), "0%db" % lens[s]) for s in present)
    assert all(not b.startswith(a) for a, b in zip(as_str, as_str[1:]))


@pytest.mark.parametrize("n", [1, 39, 4095, 4096, 4097, 65536, 100001])
def test_compress_round_trip_and_layout(n):
    x = datagen.zipf_bytes(n, seed=n)
    r = O.compress(x)
    nblk = (n + 4095) // 4096
    assert r["offsets"].size == nblk and r["offsets"][0] == 0
    # offset table is the running sum of (1 + block words)  (huffman_datapack_kernel)
    sizes = np.array([int(r["words"][o]) for o in r["offsets"]])
    assert np.array_equal(r["offsets"], np.concatenate([[0], np.cumsum(1 + sizes)[:-1]]))
    assert r["size"] == int((1 + sizes).sum()) == r["words"].size
    assert int(r["hist"].sum()) == n
    assert np.array_equal(O.decompress(r["bwt_index"], r["hist"], r["offsets"], r["words"], n), x)


@pytest.mark.parametrize("gen", ["log", "text", "zeros", "float"])
def test_lzss_round_trip_and_format(gen):
    n = 65536
    x = {"log": datagen.log_bytes, "text": datagen.text_bytes, "float": datagen.float_bytes,
         "zeros": lambda k: np.zeros(k, dtype=np.uint8)}[gen](n)
    c = O.lzss_candidates(x)
    assert c.size == 2 * n
    lens = c[0::2]
    assert lens.min() >= 1 and lens.max() <= 127 and not np.any(lens == 2)       # 1 = literal, else 3..127
    lit = lens == 1
    assert np.array_equal(c[1::2][lit], x[lit])
    p = O.lzss_pack(c, n)
    if p is None:
        assert gen == "float"                                                    # incompressible: store raw
        return
    assert int.from_bytes(bytes(p[-6:-2]), "big") == n and bytes(p[-2:]) == b"\x00\x00"
    npk = n // 4096
    sizes = np.frombuffer(bytes(p[-6 - 2 * npk:-6]), dtype=">u2")
    assert int(sizes.sum()) == p.size - 6 - 2 * npk
    assert np.array_equal(O.lzss_decode(p), x)


def test_lzss_last_chunk_quirks():
    """the last 128-byte chunk of a packet: matches are clamped to the packet end"""
    x = np.tile(np.frombuffer(b"abcdefgh", dtype=np.uint8), 512)
    c = O.lzss_candidates(x)
    lens = c[0::2].astype(int)
    pos = np.arange(4096)
    tail = pos >= 3968
    assert np.all(pos[tail] + np.where(lens[tail] == 1, 1, lens[tail]) <= 4096)
    assert np.array_equal(O.lzss_decode(O.lzss_pack(c, 4096)), x)


# ---------------------------------------------------------------- C ABI -----
def test_library_exports_every_declared_symbol(glc):
    L = glc.lib()
    missing = [s for s in glc.CUDPP_SYMBOLS + glc.CULZSS_SYMBOLS + glc.HD_SYMBOLS + glc.EXCHANGE_SYMBOLS if not hasattr(L, s)]
    assert not missing, missing
    # every function declared in the headers is in the binding's symbol lists
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for hdr, syms in (("cudpp.h", glc.CUDPP_SYMBOLS), ("culzss.h", glc.CULZSS_SYMBOLS),
                      ("glc_hd.h", glc.HD_SYMBOLS), ("glc_exchange.h", glc.EXCHANGE_SYMBOLS)):
        text = open(os.path.join(root, "include", hdr)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        declared = set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\(", text)) - {"defined", "sizeof"}
        declared = {d for d in declared if not d.isupper()}
        assert declared <= set(syms), (hdr, declared - set(syms))


def test_host_side_argument_validation_without_gpu(glc):
    """validation that happens before any device work (cudpp_plan.cpp:29-46,147-190)"""
    L = glc.lib()
    h = C.c_size_t(0)
    assert L.cudppPlan(0, C.byref(h), glc.config(glc.CUDPP_COMPRESS), 1 << 20, 1, 0) == glc.CUDPP_ERROR_INVALID_HANDLE
    fake = 0x1000      # never dereferenced for these paths
    both = glc.CUDPP_OPTION_FORWARD | glc.CUDPP_OPTION_BACKWARD
    assert L.cudppPlan(fake, C.byref(h), glc.config(glc.CUDPP_COMPRESS, options=both), 1 << 20, 1, 0) == glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION
    assert h.value == glc.CUDPP_INVALID_HANDLE
    assert L.cudppPlan(fake, C.byref(h), glc.config(glc.CUDPP_SCAN), 1024, 1, 0) == glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION
    assert L.cudppPlan(fake, C.byref(h), glc.config(glc.CUDPP_BWT), (1 << 20) + 1, 1, 0) == glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION
    assert L.cudppPlan(fake, C.byref(h), glc.config(glc.CUDPP_COMPRESS), 0, 1, 0) == glc.CUDPP_ERROR_ILLEGAL_CONFIGURATION
    assert L.cudppCompress(0, None, None, None, None, None, None, None, 4096) == glc.CUDPP_ERROR_INVALID_HANDLE
    assert L.cudppDestroyPlan(glc.CUDPP_INVALID_HANDLE) == glc.CUDPP_ERROR_INVALID_HANDLE
    assert L.cudppDestroy(0) == glc.CUDPP_ERROR_INVALID_HANDLE
    # CULZSS wrappers reject malformed arguments before touching the device
    n = C.c_int(0)
    assert L.culzss_compress(None, 4096, None, C.byref(n)) == 0
    buf = (C.c_uint8 * 8192)()
    assert L.culzss_compress(buf, 5000, buf, C.byref(n)) == 0               # not whole packets
    assert L.decompression_kernel_wrapper(buf, 4, C.byref(n), 0, 1, 1) == 0  # shorter than a trailer
    assert L.glcLzssPackStride(1 << 20) >= (1 << 20) + 2 * 256 + 6
    assert L.glcLzssWorkBytes(1 << 20, 4) > 4 * (2 << 20)


def test_product_does_not_reference_the_oracle():
    """the oracle is a checker: nothing under the package or include/ may mention it"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bad = []
    for base in ("gpu-lossless-compression_amd", "include"):
        for dp, _, fs in os.walk(os.path.join(root, base)):
            for f in fs:
                if f.endswith((".so", ".pyc")):
                    continue
                t = open(os.path.join(dp, f), errors="ignore").read()
                if "oracle_lib" in t or "glc_oracle" in t or "libglc_oracle" in t or "/root/reference" in t:
                    bad.append(os.path.join(dp, f))
    assert not bad, bad


# --------------------------------------------------------------------------
# Huffman half pinned to the reference (tests/golden/ref_huff_gold.npz, made by make_huff_gold.py from the
# reference's own huffman_build_tree_cpu / FindMinimumCountTest / computeCompressGold lines)
# --------------------------------------------------------------------------
HUFF = np.load(os.path.join(GOLD, "ref_huff_gold.npz"))


@pytest.mark.parametrize("name", [str(s) for s in HUFF["hist_cases"]])
def test_oracle_huffman_vs_reference_tree(name):
    hist = HUFF["h_%s_hist" % name]
    sym = datagen.symbols_from_hist(hist)
    _, lens, _ = O.huff_codes(hist)
    assert np.array_equal(lens, HUFF["h_%s_lens" % name]), "code lengths differ from huffman_build_tree_cpu"
    r = O.huff_encode(sym)
    assert r["size"] == int(HUFF["h_%s_size" % name][0])
    assert O.crc32(r["words"].view(np.uint8)) == int(HUFF["h_%s_crc_words" % name][0])
    assert O.crc32(r["offsets"].view(np.uint8)) == int(HUFF["h_%s_crc_offsets" % name][0])
    assert O.crc32(O.imtf(sym)) == int(HUFF["h_%s_crc_imtf" % name][0])        # inverse MTF of computeCompressGold


@pytest.mark.parametrize("name", [str(s) for s in HUFF["e2e_cases"]])
def test_oracle_compress_vs_reference_gold_chain(name):
    n = 1 << 20
    if name == "ref_compressTest":
        x = datagen.glibc_rand_bytes(n, 255); x[-1] = 0
    else:
        x = {"zipf": datagen.zipf_bytes, "float": datagen.float_bytes, "text": datagen.text_bytes}[name](n)
    assert O.crc32(x) == int(HUFF["e_%s_crc_in" % name][0])
    r = O.compress(x)
    assert r["bwt_index"] == int(HUFF["e_%s_bwt_index" % name][0])
    assert r["size"] == int(HUFF["e_%s_size" % name][0])
    assert O.crc32(r["words"].view(np.uint8)) == int(HUFF["e_%s_crc_words" % name][0])
    assert O.crc32(r["offsets"].view(np.uint8)) == int(HUFF["e_%s_crc_offsets" % name][0])
    assert np.array_equal(r["hist"], HUFF["e_%s_hist" % name])


def test_reference_gold_live_against_oracle():
    """trees, MTF, BWT and the gold decoder of the reference against the oracle: as ref_live_gold.npz keeps them, and live
    where the reference's lines are compiled"""
    live = O.have_ref_compress_gold()
    for i, hist in enumerate(LG.huff_hists()):
        lens = LIVE["huff_lens"][i]
        if live:
            assert np.array_equal(O.ref_codes_from_tree(O.ref_huffman_tree(hist))[1], lens)
        assert np.array_equal(lens.astype(np.uint8), O.huff_codes(hist)[1])
    x, y = LG.compress_gold_inputs()
    b, idx = LIVE["bwt_out"], int(LIVE["bwt_idx"])
    if live:
        rb, ridx = O.ref_bwt_gold(x)
        assert ridx == idx and np.array_equal(rb, b)
        assert np.array_equal(O.ref_mtf_gold(b), LIVE["mtf_out"])
    ob, oidx = O.bwt(x)
    assert idx == oidx and np.array_equal(b, ob)
    assert np.array_equal(LIVE["mtf_out"], O.mtf(b))
    r = O.compress(y)
    want = O.bwt(y)[0]
    # the stream the gold decoder read back when ref_live_gold.npz was made
    assert r["size"] == int(LIVE["stream_size"]) and r["bwt_index"] == int(LIVE["stream_bwt_index"])
    for k in ("words", "offsets", "hist"):
        assert O.crc32(r[k].view(np.uint8)) == int(LIVE["stream_crc_" + k]), k
    if live:
        sym, byt = O.ref_compress_gold_decode(r["hist"], r["offsets"], r["words"], y.size)
        assert np.array_equal(byt, want)                      # gold Huffman decode + inverse MTF reads the oracle's stream
    assert O.crc32(want) == int(LIVE["decode_crc"])


# ------------------------------------------------ CULZSS packer vs the reference's own aftercomp (row a13) ----
LZSS_GOLD = np.load(os.path.join(GOLD, "ref_lzss_gold.npz"))
_LZSS_INPUTS = None


def lzss_gold_candidates(name):
    """the candidate stream of a fixture case, regenerated from its seed (and checked against the fixture's CRC)"""
    global _LZSS_INPUTS
    import zlib
    n = int(LZSS_GOLD[name + "/n"])
    if str(LZSS_GOLD[name + "/kind"]) == "input":
        if _LZSS_INPUTS is None:
            _LZSS_INPUTS = datagen.lzss_gold_inputs()
        x = _LZSS_INPUTS[name]
        cand = O.lzss_candidates(x)
    else:
        x = None
        cand = datagen.lzss_synthetic_candidates()[1][name[4:]]
    assert (zlib.crc32(cand.tobytes()) & 0xFFFFFFFF) == int(LZSS_GOLD[name + "/cand_crc"]), "candidates of %s drifted" % name
    return n, x, cand


@pytest.mark.parametrize("name", [str(s) for s in LZSS_GOLD["names"]])
def test_oracle_lzss_pack_vs_reference_aftercomp(name):
    """orc_lzss_pack == the reference's own aftercompression_wrapper (gpu_compress.cu:462-672, compiled from the
    reference's lines; tests/golden/make_lzss_gold.py): return code, size, CRC, first / last bytes, and the bytes
    themselves where the fixture keeps them; the oracle's decoder reads the reference-packed bytes back."""
    import zlib
    n, x, cand = lzss_gold_candidates(name)
    got = O.lzss_pack(cand, n)
    if int(LZSS_GOLD[name + "/rc"]) == 0:
        assert got is None
        return
    assert got is not None and got.size == int(LZSS_GOLD[name + "/size"])
    assert (zlib.crc32(got.tobytes()) & 0xFFFFFFFF) == int(LZSS_GOLD[name + "/crc"])
    assert np.array_equal(got[:64], LZSS_GOLD[name + "/head"]) and np.array_equal(got[-32:], LZSS_GOLD[name + "/tail"])
    if name + "/packed" in LZSS_GOLD:
        ref_bytes = LZSS_GOLD[name + "/packed"]
        assert np.array_equal(got, ref_bytes)
        if x is not None:
            assert np.array_equal(O.lzss_decode(ref_bytes), x), "oracle decoder on reference-packed bytes"


def test_reference_aftercomp_live_against_fixture_and_oracle():
    """the reference's packer == the committed fixture == the oracle, on fresh candidate streams too (random mixtures the
    fixture does not hold; what the reference made of them is in ref_live_gold.npz); where oracle/_ref was built, the
    reference's packer runs again now"""
    import zlib
    live = O.have_ref_aftercomp()
    for name in ("log_4pkt", "spaces_then_text", "syn_random_mix", "one_packet_random"):
        n, _, cand = lzss_gold_candidates(name)
        for r in [O.lzss_pack(cand, n)] + ([LG.ref_aftercomp(cand, n)] if live else []):
            if int(LZSS_GOLD[name + "/rc"]) == 0:
                assert r is None
            else:
                assert (zlib.crc32(r.tobytes()) & 0xFFFFFFFF) == int(LZSS_GOLD[name + "/crc"])
    for trial, x in enumerate(LG.aftercomp_inputs()):
        cand = O.lzss_candidates(x)
        o = O.lzss_pack(cand, x.size)
        if int(LIVE["ac_%d_rc" % trial]) == 0:
            assert o is None, trial
        else:
            assert o is not None and o.size == int(LIVE["ac_%d_size" % trial]), trial
            assert (zlib.crc32(o.tobytes()) & 0xFFFFFFFF) == int(LIVE["ac_%d_crc" % trial]), trial
        if live:
            r = LG.ref_aftercomp(cand, x.size)
            assert (r is None) == (o is None) and (r is None or np.array_equal(r, o)), trial


def test_survey_kat_on_pg1661():
    """the survey's INDEPENDENT lock-step restatement of EncodeKernel / aftercomp on pg1661.txt
    zero-padded to one 1 MiB buffer gave candidates CRC 799b54ef and 569 823 packed bytes, CRC 15c4edd7.  The only
    pin rows a11 / a14 can have (EncodeKernel and DecodeKernel are CUDA only, no CPU twin, no test in the reference).
    The text is the reference's pg1661.txt, kept as tests/golden/pg1661.txt.bz2."""
    import zlib
    raw = LG.pg1661_text()
    x = np.zeros(1 << 20, dtype=np.uint8)
    x[: raw.size] = raw[: 1 << 20]
    cand = O.lzss_candidates(x)
    assert "%08x" % (zlib.crc32(cand.tobytes()) & 0xFFFFFFFF) == "799b54ef"
    packed = O.lzss_pack(cand, x.size)
    assert packed.size == 569823 and "%08x" % (zlib.crc32(packed.tobytes()) & 0xFFFFFFFF) == "15c4edd7"
    assert np.array_equal(O.lzss_decode(packed), x)
    if O.have_ref_aftercomp():
        import ctypes
        buf = np.zeros(x.size + 8192, dtype=np.uint8)
        m = ctypes.c_int(-1)
        assert O.ref_aftercomp_lib().aftercompression_wrapper(buf.ctypes.data, x.size, cand.ctypes.data, ctypes.byref(m)) == 1
        assert m.value == 569823 and np.array_equal(buf[: m.value], packed)


# ------------------------------------------------ CULZSS match search vs the reference's own FindMatch (row a11) ----
FM_GOLD = np.load(os.path.join(GOLD, "ref_findmatch_gold.npz"))
_FM_INPUTS = None


@pytest.mark.parametrize("name", [str(s) for s in FM_GOLD["names"]])
def test_oracle_lzss_candidates_vs_reference_findmatch(name):
    """orc_lzss_candidates == the candidate stream the reference's own FindMatch (gpu_compress.cu:104-168, compiled
    from the reference's lines by oracle/mk_ref_findmatch.sh) produced inside EncodeKernel's ring choreography
    (tests/golden/make_findmatch_gold.py): CRC-32 for every input, every byte for inputs up to 64 KiB."""
    global _FM_INPUTS
    import zlib
    if _FM_INPUTS is None:
        _FM_INPUTS = datagen.findmatch_gold_inputs()
    x = _FM_INPUTS[name]
    assert x.size == int(FM_GOLD[name + "/n"]) and (zlib.crc32(x.tobytes()) & 0xFFFFFFFF) == int(FM_GOLD[name + "/in_crc"]), "input of %s drifted" % name
    cand = O.lzss_candidates(x)
    assert (zlib.crc32(cand.tobytes()) & 0xFFFFFFFF) == int(FM_GOLD[name + "/cand_crc"]), name
    if name + "/cand" in FM_GOLD:
        assert np.array_equal(cand, FM_GOLD[name + "/cand"]), name
    assert int(np.count_nonzero(cand[0::2] > 1)) == int(FM_GOLD[name + "/matches"])


def test_reference_findmatch_live_on_fresh_packets():
    """the reference's FindMatch on packets that are not in the fixture (its candidates kept in ref_live_gold.npz, and run
    HERE where oracle/_ref was built) against the oracle"""
    import make_findmatch_gold as M
    for i, x in enumerate(LG.findmatch_inputs()):
        want = LIVE["fm_%d" % i]
        if O.have_ref_findmatch():
            assert np.array_equal(M.ref_candidates(x), want)
        assert np.array_equal(want, O.lzss_candidates(x))


# ------------------------------------------------ the config-2 generator ----
def test_philox4x32_10_known_answers():
    """Random123's kat_vectors for philox4x32-10: counter, key -> output"""
    kats = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
            ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
            ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kats:
        got = datagen.philox4x32_10(*[np.array([v], dtype=np.uint64) for v in ctr], *key)
        assert tuple(int(g[0]) for g in got) == want


def test_zipf_philox_stream_is_a_function_of_the_byte_index():
    a = datagen.zipf_philox_bytes(0, 1 << 16)
    b = datagen.zipf_philox_bytes(1 << 12, 1 << 12)
    assert np.array_equal(a[1 << 12: 1 << 13], b)                    # any range, from anywhere
    h = np.bincount(datagen.zipf_philox_bytes(5 << 20, 1 << 20), minlength=256) / float(1 << 20)
    p = 1.0 / np.arange(1, 257); p /= p.sum()
    assert abs(h[0] - p[0]) < 2e-3 and abs(h[1] - p[1]) < 2e-3 and abs(h[255] - p[255]) < 3e-4

