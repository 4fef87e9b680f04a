"""The container model against its pins (tests/golden/container_model_pins.json, recorded from the four per-version model modules
that tests/container_model.py replaced): every container of the writer grid byte for byte, and what the reader of each format
version makes of every valid, corrupted, truncated and fixture container -- decoded bytes and kinds, or (what, frame, block)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def replay():
    spec = importlib.util.spec_from_file_location("make_container_model_pins",
                                                  os.path.join(ROOT, "tests", "golden", "make_container_model_pins.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    return g, g.pins(), g.committed()


def test_the_grid_is_the_one_the_pins_were_asked_for(replay):
    g, now, want = replay
    grid = [k for k in want["written"] if k.startswith("grid/")]
    assert len(grid) == 4 * (5 * 2 + 3 * 2) and len(want["written"]) == len(grid) + 3
    assert {"fixture/" + f for f in g.FIXTURES} <= set(want["read"])
    assert all(len(r) == 4 for r in want["read"].values())
    multi = [k for k in want["written"] if k + "/cut_last" in want["read"]]
    assert multi and all(k + "/cut_frame1" in want["read"] for k in multi)


def test_writer_makes_the_pinned_containers(replay):
    _, now, want = replay
    assert now["written"].keys() == want["written"].keys()
    assert [k for k in want["written"] if now["written"][k] != want["written"][k]] == []


def test_reader_of_every_version_gives_the_pinned_outcome(replay):
    _, now, want = replay
    assert now["read"].keys() == want["read"].keys()
    for name, row in want["read"].items():
        got = [now["outcomes"][i] for i in now["read"][name]]
        assert got == [want["outcomes"][i] for i in row], name


def test_generator_reproduces_the_committed_file_byte_for_byte(replay):
    g, now, _ = replay
    with open(g.OUT) as f:
        assert g.dumps(now) == f.read()
