"""The repair walk of the chunked recursions (hammlet_amd/csrc/hml_k_chunks.h: hml_chunk_same, hml_chunk_rerun_walk) on the
host, around a toy recursion: tests/fixtures/chunk_walk_main.cpp, a stand-alone program built with g++ -Wall -Werror, and a
second time with the address and undefined-behaviour sanitizers (nothing is loaded into Python for this, and no GPU is used).

The program itself checks, per case and round, that (a) the order in which the heads are walked leaves no trace in entry, exit
and rows - no lane writes what another reads -, (b) every round strictly lowers the number of stale chunks, (c) after a serial
finish the rows are the sequential recursion's byte for byte, and (d) every walk stopped where the rule says it stops; it
exits with 1 at the first miss.  What it prints per case is asserted here, so that none of that holds vacuously."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "fixtures", "chunk_walk_main.cpp")
CSRC = os.path.join(ROOT, "hammlet_amd", "csrc")

# seed, B, L, W, hard resets in percent, rounds
CASES = [
    (1, 400, 4, 1, 5, 8),      # the geometry of the GPU tests: chunks of 4 blocks, a warm-up of 1
    (2, 400, 4, 1, 10, 8),
    (3, 400, 4, 1, 20, 8),
    (4, 401, 4, 1, 2, 8),      # B no multiple of L
    (5, 1000, 4, 2, 5, 3),
    (6, 300, 1, 1, 10, 8),     # L = 1
    (7, 300, 3, 0, 10, 8),     # W = 0
    (8, 7, 8, 1, 10, 8),       # one chunk: nothing can be stale, and it is not counted below
    (9, 257, 16, 4, 3, 8),
    (10, 400, 4, 1, 0, 2),     # no hard reset and two rounds: the serial finish has work left
    (11, 64, 4, 1, 10, 0),     # no round at all
]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    directory = tmp_path_factory.mktemp("chunk_walk")
    out = {}
    for name, extra in (("plain", ["-O2"]), ("sanitized", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = os.path.join(str(directory), name)
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC] + extra + ["-o", exe, SRC], check=True)
        out[name] = exe
    return out


def run(exe, word):
    text = "".join("%d %d %d %d %d %d\n" % c for c in CASES)
    p = subprocess.run([exe, word], input=text, capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    rows = []
    for line in p.stdout.splitlines():
        row = dict(re.findall(r"(\w+)=([\d,]+)", line))
        rows.append({k: [int(x) for x in v.split(",")] if k == "stale" else int(v) for k, v in row.items()})
    assert [r["seed"] for r in rows] == [c[0] for c in CASES]
    return rows


@pytest.mark.parametrize("build", ["plain", "sanitized"])
@pytest.mark.parametrize("word", ["ll", "dbl"])
def test_rounds_and_finish(programs, build, word):
    rows = run(programs[build], word)
    counted = [r for r in rows if r["stale"][0] > 0]
    # every case of more than one chunk has stale chunks behind its first run, and only those are counted
    assert [r["seed"] for r in counted] == [c[0] for c in CASES if c[1] > c[2]]
    assert all(r["chunks"] == 1 and r["stale"] == [0] for r in rows if r not in counted)
    for r, case in zip(rows, CASES):
        assert r["chunks"] == -(-case[1] // case[2])
        assert len(r["stale"]) - 1 <= case[5]
        assert all(b < a for a, b in zip(r["stale"], r["stale"][1:])), r   # (b), once more
        assert r["stale"][-1] == 0 or len(r["stale"]) - 1 == case[5]          # the rounds ended for a reason
    # each of the walk's ways on was taken: it returned at a chunk that matched and still does, stepped over a stale chunk that
    # is right as stored now, returned before the matching predecessor of another lane's head, ran the successor again
    for way in ("still", "stored", "other", "again"):
        assert sum(r[way] for r in counted) > 0, way
    assert any(r["longest"] >= 3 for r in counted)
    assert any(len(r["stale"]) > 1 and r["stale"][1] > 0 for r in counted)    # stale chunks behind a first round
    assert any(r["stale"][-1] > 0 for r in counted)                           # ... and for the serial finish
    # doubles: an entry of -0.0 where the predecessor left 0.0 is equal as a value and stale as a word
    traps = sum(r["zero_traps"] for r in counted)
    assert traps > 0 if word == "dbl" else traps == 0
