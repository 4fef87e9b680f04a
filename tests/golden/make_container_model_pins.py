"""Writes tests/golden/container_model_pins.json: what the Python model of the BWT container (tests/container_model.py) writes
and reads, recorded so that a change to the model cannot change the format unnoticed.  The committed file was recorded from
the four per-version model modules that came before the one model (their writers through the version-4 one, which fell back
to the older ones; their readers one by one, as readers 1 to 4); this generator reproduces it byte for byte.

  writer pins: SHA-256 and length of the container of a grid of inputs, element sizes, codecs and delta modes, and of the
               mixed-kind containers;
  reader pins: for every such container, every refusal case the CPU tests build, the four .bin fixtures and two truncations
               of every valid container of more than one frame, the outcome of the reader of each format version
               (read(..., max_version=k)): the SHA-256 of the decoded bytes and the kinds, or (what, frame, block).
Outcomes are stored once each in "outcomes"; a container's "read" is four indices into that list.
python tests/golden/make_container_model_pins.py"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import container_model as M  # noqa: E402
import datagen  # noqa: E402
import series_datagen  # noqa: E402
import typed_datagen  # noqa: E402

OUT = os.path.join(HERE, "container_model_pins.json")
GRID = ((0, 4096, 2), (5, 4096, 1), (3 * 4096 + 77, 4096, 2), (70000, 65536, 4))
MIXED = [0, 2, 1, 2, 0, 1]
FIXTURES = ("container_v1.bin", "container_v2_f32.bin", "container_v3_mixed.bin", "container_v4_series.bin")


def grid_input(n, elem, delta):
    if n == 0:
        return np.zeros(0, np.uint8)
    if delta:
        return series_datagen.series_bytes({2: "adc16", 4: "ids32", 8: "ts64"}[elem], n + 8)[:n].copy()
    if elem > 1:
        return typed_datagen.typed_bytes({2: "quant16", 4: "smooth32", 8: "smooth64"}[elem], n, seed=3)
    return datagen.text_bytes(n, seed=3)


def grid_name(n, bl, rows, elem, codec, delta):
    return "grid/n%d_bl%d_r%d/e%d_c%d_d%d" % (n, bl, rows, elem, codec, delta)


def pin(c):
    return [hashlib.sha256(c).hexdigest(), len(c)]


def committed():
    with open(OUT) as f:
        return json.load(f)


def written():
    """[(name, container)]: the writer grid and the mixed-kind containers"""
    out = []
    for n, bl, rows in GRID:
        for elem in (0, 1, 2, 4, 8):
            for codec in (0, 1):
                for delta in (False, True) if elem > 1 else (False,):
                    x = grid_input(n, elem, delta)
                    out.append((grid_name(n, bl, rows, elem, codec, delta), M.write(x, bl, rows, elem, codec, delta)))
    x = np.concatenate([datagen.text_bytes(3 * 4096, seed=1), datagen.zipf_bytes(4 * 4096 + 100, seed=2)])
    for elem, delta in ((0, False), (4, False), (4, True)):
        out.append(("mixed/e%d_d%d" % (elem, delta), M.write(x, 4096, 4, elem, 0, delta, kinds=MIXED)))
    return out


def _flip(c, pos):
    b = bytearray(c)
    b[pos] ^= 0x20
    return bytes(b)


def refusals():
    """[(name, container)]: the corruption cases of the CPU container tests, built as those tests build them"""
    out = []
    # test_cpu_container.py
    x = np.concatenate([datagen.text_bytes(3 * 4096, seed=2), np.random.default_rng(1).integers(0, 256, 3, dtype=np.uint8)])
    c = M.write(x, 4096, 2)
    lay = M.layout(c)
    f0, f1, f2 = lay["frames"]
    s1, e1, _ = f0["records"][1]
    at = [5, f0["start"] + 8, f1["tables"][0] + 700, (s1 + e1) // 2, f2["records"][0][0] + 1, lay["trailer"] + 6]
    at += list(range(f0["start"], f0["tables"][1], 97))
    out += [("v1/flip%d" % pos, _flip(c, pos)) for pos in at]
    out += [("v1/cut_last", c[:-1]), ("v1/cut_frame1", c[:f1["start"] + 40])]
    # test_cpu_container_filter.py
    x = typed_datagen.typed_bytes("smooth32", 3 * 4096 + 123, seed=5)
    c, v1 = M.write(x, 4096, 2, 4), M.write(x, 4096, 2)
    lay = M.layout(c)
    s, e, _ = lay["frames"][1]["records"][0]
    out += [("v2/valid", c)] + [("v2/elem%d" % el, M.with_header(c, 2, 0, el)) for el in (0, 1, 3, 16, 2)]
    out += [("v2/v1_elem4", M.with_header(v1, 1, 0, 4)), ("v2/as_v3", M.with_header(c, 3, 0, 4)), ("v2/flip", _flip(c, (s + e) // 2)),
            ("v2/cut_frame1", c[:lay["frames"][1]["start"] + 40])]
    # test_cpu_container_codec.py
    n, rows, elem = 4096, 3, 4
    x = np.concatenate([typed_datagen.typed_bytes("smooth32", 5 * n, seed=4), datagen.zipf_bytes(2 * n + 123, seed=4)])
    c = M.write(x, n, rows, elem, 1)
    out += [("v3/valid", c), ("v3/unfiltered", M.write(x, n, rows, 0, 1))]
    out += [("v3/case%d" % i, cont) for i, (cont, _) in enumerate(M.corrupted_cases(c, x, n, rows, elem)[0])]
    # test_cpu_container_delta.py
    n, rows, elem = 4096, 2, 4
    x = series_datagen.series_bytes("ids32", 5 * n + 123 + 8)[:5 * n + 123].copy()
    for codec in (0, 1):
        c4, c3 = M.write(x, n, rows, elem, codec, True), M.write(x, n, rows, elem, 1)
        out += [("v4/c%d/valid" % codec, c4)]
        out += [("v4/c%d/case%d" % (codec, i), cont) for i, (cont, _) in enumerate(M.refusal_cases(c4, c3, elem)[0])]
    c = M.write(x, n, 4, elem, 0, True, kinds=[0, 2, 1, 2])
    fr = M.layout(c)["frames"][0]
    bad = bytearray(c)
    bad[fr["tables"][0]:fr["tables"][0] + 4] = (3).to_bytes(4, "little")
    out += [("v4/kinds", c), ("v4/kind3", M.retable(bytes(bad), fr["start"]))]
    return out


def outcome(c, k):
    """what the reader of format version k makes of c"""
    try:
        data, kinds = M.read(c, with_kinds=True, max_version=k)
    except M.ContainerError as e:
        return [e.what, e.frame, e.block]
    return {"sha256": hashlib.sha256(data.tobytes()).hexdigest(), "kinds": "".join(str(v) for v in kinds)}


def pins():
    valid = written()
    cases = list(valid)
    for name, c in valid:
        frames = M.layout(c)["frames"]
        if len(frames) > 1:
            cases += [(name + "/cut_last", c[:-1]), (name + "/cut_frame1", c[:frames[1]["start"] + 40])]
    cases += refusals()
    cases += [("fixture/" + f, open(os.path.join(HERE, f), "rb").read()) for f in FIXTURES]
    outcomes, index, read = [], {}, {}
    for name, c in cases:
        assert name not in read, name
        row = []
        for k in (1, 2, 3, 4):
            o = outcome(c, k)
            key = json.dumps(o, sort_keys=True)
            if key not in index:
                index[key] = len(outcomes)
                outcomes.append(o)
            row.append(index[key])
        read[name] = row
    return {"written": {name: pin(c) for name, c in valid}, "outcomes": outcomes, "read": read}


def dumps(p):
    """one outcome, one container per line"""
    def j(v):
        return json.dumps(v, sort_keys=True, separators=(",", ":"))

    def section(d):
        return "{\n" + ",\n".join("%s:%s" % (j(k), j(d[k])) for k in sorted(d)) + "\n}"
    return ('{\n"outcomes":[\n' + ",\n".join(j(o) for o in p["outcomes"]) + '\n],\n"read":' + section(p["read"])
            + ',\n"written":' + section(p["written"]) + "\n}\n")


if __name__ == "__main__":
    with open(OUT, "w") as f:
        f.write(dumps(pins()))
