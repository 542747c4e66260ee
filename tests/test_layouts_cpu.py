"""The device buffers that hold several arrays have one layout function each (hammlet_amd/csrc/hml_layouts.h: no HIP, a host
compiler builds it), which the allocation and the launch sites both call.  A layout that disagrees with the size it reports
writes out of bounds on the GPU; here a stand-alone program (tests/fixtures/layouts_main.cpp) prints sizes and view offsets,
and this file holds them to the formulas of the commit before the layouts existed, written out below: the total bytes, every
view aligned to its element type (the three list arrays to 16 bytes), the views ascending, disjoint and inside the total, and
the size on a null base equal to the size on a real one."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = [2, 16, 17, 64]
CAPS = [64, 100001, 10 ** 8]

MAX_CHUNKS = 16384          # of the state-a-lane forms (HML_COMPAT_MAX_CHUNKS)
WL_MAX_CHUNKS = 131072      # of the chunk-a-lane form
WL_TOT_WORDS = 4 + 2 * (WL_MAX_CHUNKS // 64)   # three counters (in four words), a bit per chunk for the filter and for the backward draws
CAP_K = 64                  # states the model's arrays hold
PART_TILE = 4096            # blocks per tile of the partition by state
WL_PITCH, WL_GTAB = 64, 2048
FUSED_WAVES = 8


def ceil_div(a, b):
    return (a + b - 1) // b


def wide_max_chunks_of(K, wmc):
    if wmc:
        return min(wmc, WL_MAX_CHUNKS)
    return WL_MAX_CHUNKS if K <= 36 else WL_MAX_CHUNKS // 2


def cchunk_case(mode, K, cap, lshift=-1, wmc=0):
    """(input row, total bytes, views (name, bytes, alignment) in address order, extras) by the earlier formulas"""
    if mode == "compat":
        n = MAX_CHUNKS
        tot = 64                                   # the 64 bytes of slack that `tot` pointed into
        total = n * (2 * K * 4 + 4 * 4) + 64
    else:
        Lmin = 1 << lshift if lshift >= 0 else 4
        n = max(MAX_CHUNKS, min(WL_MAX_CHUNKS, ceil_div(cap, Lmin) + 64))
        tot = WL_TOT_WORDS * 8
        total = n * (2 * K * 4 + 4 * 4) + tot
    Lmax = max(4, 1 << lshift if lshift >= 0 else 4)
    while ceil_div(cap, Lmax) > wide_max_chunks_of(K, wmc):
        Lmax *= 2
    plane = (cap + 1 + 64 * Lmax) * K
    views = [("entry", n * K * 4, 4), ("exitv", n * K * 4, 4), ("nfb", n * 4, 4), ("in_state", n * 4, 4), ("out_state", n * 4, 4), ("bad", n * 4, 4), ("tot", tot, 8)]
    return "cchunk %s %d %d %d %d" % (mode, K, cap, lshift, wmc), total, views, "chunks %d tot_bytes %d plane %d" % (n, tot, plane)


def clists_case(K, cap):
    entries = (cap + 4 * CAP_K + 3) & ~3
    tiles = ceil_div(cap, PART_TILE)
    total = 3 * entries * 4 + CAP_K * CAP_K * 8 + tiles * K * 4 + 2 * (CAP_K + 1) * 4 + 64
    views = [("sx", entries * 4, 16), ("sq", entries * 4, 16), ("n", entries * 4, 16), ("offdiag", CAP_K * CAP_K * 8, 8), ("tile_count", tiles * K * 4, 4),
             ("state_off", 2 * (CAP_K + 1) * 4, 4)]
    return "clists %d %d" % (K, cap), total, views, None


def wa_case():
    views = [("A", WL_PITCH * WL_PITCH * 4, 16), ("gtab", CAP_K * WL_GTAB * 4, 4)]
    return "wa", (WL_PITCH * WL_PITCH + CAP_K * WL_GTAB) * 4, views, None


def wave_total_case(tiles):
    views = [("wave_total", (tiles + 1) * FUSED_WAVES * 4, 4), ("tile_before", (tiles + 1) * 4, 4), ("tile_prev", (tiles + 1) * 4, 4)]
    return "wave_total %d" % tiles, (tiles + 1) * (FUSED_WAVES + 2) * 4, views, None


CASES = []
for K in KS:
    for cap in CAPS:
        CASES.append(cchunk_case("compat", K, cap))
        # the chunk-a-lane path: the default geometry (at 100001 blocks an odd number of chunks, 25065), forced chunk lengths of 1 and 32,
        # and a bound on the chunks of a sweep (longer chunks: a larger plane, the same per-chunk arrays)
        CASES += [cchunk_case("wide", K, cap), cchunk_case("wide", K, cap, lshift=0), cchunk_case("wide", K, cap, lshift=5), cchunk_case("wide", K, cap, wmc=100)]
        CASES.append(clists_case(K, cap))
CASES.append(wa_case())
CASES += [wave_total_case(t) for t in (1, 2, 763, 32768)]   # (tiles of 2^17 positions: 763 at 10^8, 32768 at 2^32)


def build(tmp_path, *flags):
    exe = str(tmp_path / ("layouts" + "".join(flags).replace("=", "_").replace(",", "_")))
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", os.path.join(REPO, "hammlet_amd", "csrc"), "-o", exe,
                    os.path.join(REPO, "tests", "fixtures", "layouts_main.cpp")], check=True)
    return exe


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "sanitized"])
def test_layouts_match_the_earlier_formulas(tmp_path, flags):
    exe = build(tmp_path, *flags)
    r = subprocess.run([exe], input="".join(c[0] + "\n" for c in CASES), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = r.stdout.splitlines()
    assert len(got) == len(CASES)
    for (row, total, views, extras), line in zip(CASES, got):
        numbers, _, rest = line.partition(" | ")
        bytes_null, bytes_real, *offsets = [int(v) for v in numbers.split()]
        assert bytes_null == total and bytes_real == total, row
        assert len(offsets) == len(views), row
        end = 0
        for (name, size, align), off in zip(views, offsets):
            assert off % align == 0, (row, name)
            assert off >= end, (row, name)          # ascending and disjoint: it starts where the one before it ended, or later
            end = off + size
        assert end <= total, row
        if extras is not None:
            assert rest == extras, row


def test_the_cases_cover_what_they_claim():
    rows = [c[0] for c in CASES]
    assert "cchunk wide 17 100001 -1 0" in rows and cchunk_case("wide", 17, 100001)[3].startswith("chunks 25065 ")
    assert len(rows) == len(set(rows))
