#!/usr/bin/env python3
"""Generates tests/golden/ref_live_gold.npz -- run where oracle/_ref was built from the reference (`make -C oracle`):
    python tests/golden/make_ref_live_gold.py <reference root>

tests/test_cpu_oracle.py runs the reference's own CPU routines against the oracle where oracle/_ref exists.  So that
those checks hold on every machine, this script runs the same routines on the same inputs once and keeps what they
produced:

  sa_crc_<n>_<mod>          computeSaGold on glibc-rand inputs (SA_CASES): CRC-32 of the suffix array's bytes
  huff_lens                 [40, 257] code lengths of huffman_build_tree_cpu on the seeded histograms of huff_hists()
  bwt_out, bwt_idx, mtf_out computeBwtGold / computeMtfGold on 20 000 bytes of text (compress_gold_inputs)
  decode_crc                computeCompressGold's Huffman + inverse-MTF half on the oracle's stream of a 1 MiB Zipf block
  stream_*                  that stream (size, BWT index, CRC-32 of words / offsets / hist), as the gold decoder read it
  ac_<t>_rc, _size, _crc    aftercompression_wrapper on the candidate streams of aftercomp_inputs()
  fm_<i>                    the candidate stream of FindMatch (make_findmatch_gold.ref_candidates) on findmatch_inputs()

and copies the reference's pg1661.txt (the text of SURVEY.md App. C) to tests/golden/pg1661.txt.bz2.
The files hold data only."""
import bz2
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import datagen  # noqa: E402
import oracle_lib as O  # noqa: E402

SA_CASES = ((1 << 20, 255), (500001, 128), (1048577, 255))
PG1661_REF = "cuda-lzss-unknown/pg1661.txt"
PG1661 = os.path.join(HERE, "pg1661.txt.bz2")


def huff_hists():
    rng = np.random.default_rng(3)
    for _ in range(40):
        k = int(rng.integers(1, 257))
        hist = np.zeros(256, dtype=np.uint32)
        hist[rng.choice(256, k, replace=False)] = rng.integers(1, 50, k) if rng.random() < 0.5 else rng.integers(1, 100000, k)
        yield hist


def compress_gold_inputs():
    """(text block for the BWT / MTF gold, Zipf block for the gold decoder)"""
    return datagen.text_bytes(20000, seed=8), datagen.zipf_bytes(1 << 20, seed=77)


def aftercomp_inputs():
    rng = np.random.default_rng(5)
    for trial in range(6):
        yield np.concatenate([datagen.log_bytes(8192, seed=100 + trial), rng.integers(97, 101, 4096, dtype=np.uint8),
                              datagen.text_bytes(4096, seed=trial)])


def findmatch_inputs():
    rng = np.random.default_rng(20260929)
    return (datagen.log_bytes(8192, seed=123), datagen.text_bytes(4096, seed=321),
            rng.integers(0, 3, 4096, dtype=np.uint8), np.repeat(rng.integers(0, 256, 64, dtype=np.uint8), 64))


def pg1661_text():
    return np.frombuffer(bz2.decompress(open(PG1661, "rb").read()), dtype=np.uint8)


def ref_aftercomp(cand, n):
    import ctypes
    buf = np.zeros(n + 8192, dtype=np.uint8)
    m = ctypes.c_int(-1)
    c = cand.copy()
    rc = O.ref_aftercomp_lib().aftercompression_wrapper(buf.ctypes.data, n, c.ctypes.data, ctypes.byref(m))
    return buf[: m.value].copy() if rc == 1 else None


def main():
    import make_findmatch_gold as M
    assert len(sys.argv) == 2, __doc__
    assert O.have_ref_gold() and O.have_ref_compress_gold() and O.have_ref_aftercomp() and O.have_ref_findmatch(), \
        "run `make -C oracle` where the reference is present"
    out = {}
    for n, mod in SA_CASES:
        out["sa_crc_%d_%d" % (n, mod)] = np.uint32(O.crc32(O.ref_sa_gold(O.glibc_rand_bytes(n, mod)).view(np.uint8)))
    out["huff_lens"] = np.stack([O.ref_codes_from_tree(O.ref_huffman_tree(h))[1] for h in huff_hists()])
    x, y = compress_gold_inputs()
    b, idx = O.ref_bwt_gold(x)
    out["bwt_out"], out["bwt_idx"], out["mtf_out"] = b, np.int64(idx), O.ref_mtf_gold(b)
    r = O.compress(y)
    _, byt = O.ref_compress_gold_decode(r["hist"], r["offsets"], r["words"], y.size)
    assert np.array_equal(byt, O.bwt(y)[0]), "the gold decoder does not read the oracle's stream back"
    out["decode_crc"] = np.uint32(O.crc32(byt))
    out["stream_size"], out["stream_bwt_index"] = np.int64(r["size"]), np.int64(r["bwt_index"])
    for k in ("words", "offsets", "hist"):
        out["stream_crc_" + k] = np.uint32(O.crc32(r[k].view(np.uint8)))
    for t, x in enumerate(aftercomp_inputs()):
        p = ref_aftercomp(O.lzss_candidates(x), x.size)
        out["ac_%d_rc" % t] = np.int64(0 if p is None else 1)
        out["ac_%d_size" % t] = np.int64(0 if p is None else p.size)
        out["ac_%d_crc" % t] = np.uint32(0 if p is None else zlib.crc32(p.tobytes()))
    for i, x in enumerate(findmatch_inputs()):
        out["fm_%d" % i] = M.ref_candidates(x)
    np.savez_compressed(os.path.join(HERE, "ref_live_gold.npz"), **out)
    with open(os.path.join(sys.argv[1], PG1661_REF), "rb") as f:
        open(PG1661, "wb").write(bz2.compress(f.read(), 9))
    print("wrote ref_live_gold.npz (%d arrays) and pg1661.txt.bz2" % len(out))


if __name__ == "__main__":
    main()
