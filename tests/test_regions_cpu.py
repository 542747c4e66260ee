"""Joint posteriors over regions (include/hml.h: hml_set_regions, hml_get_regions, hml_regions_read, hml_regions_add,
hml_regions_merge) - what can be checked without a GPU: the library's surface, the numpy restatement of
tests/regions_util.py by hand, that the cases of tests/test_gpu_regions.py have something to find on the CPU checker alone,
the saturation rule of the helpers, and the driver's reading of a regions file (it fails before any GPU call)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import bands_cases as bc
from tests import regions_util as ru

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "hammlet_amd", "hammlet")
CALLS = ("hml_set_regions", "hml_get_regions", "hml_regions_read", "hml_regions_add", "hml_regions_merge")


def test_library_exports_the_region_calls():
    from hammlet_amd import build, capi
    import hammlet_amd
    build.build_library()
    lib = ctypes.CDLL(build.LIB_PATH)
    for name in CALLS:
        assert hasattr(lib, name), name
        assert name in capi.SIGNATURES
    lib.hml_abi_version.restype = ctypes.c_uint32
    assert lib.hml_abi_version() == 5 and capi.ABI_VERSION == 5      # additions only
    for name in ("set_regions", "get_regions", "regions", "regions_add", "regions_merge"):
        assert hasattr(capi.Chain, name)
    assert callable(capi.regions_summary) and hammlet_amd.regions_summary is capi.regions_summary


def test_helper_regions_by_hand():
    """ten positions, blocks [0, 2) [2, 5) [5, 6) [6, 10) in states 0 0 1 2, means 1.0, -2.0, 0.5, one edge at 1.0 (the level 1.0
    lies ON the edge: band 1; -2.0 and 0.5: band 0).  One breakpoint at 5 (state 0 -> 1) and one at 6 (1 -> 2); the band changes
    at 5 only."""
    sweep = (np.array([0, 2, 5, 6, 10]), np.array([0, 0, 1, 2]), np.array([1.0, -2.0, 0.5], np.float32))
    start = np.array([0, 0, 1, 4, 5, 5, 5, 6, 9, 2])
    end = np.array([10, 5, 3, 6, 6, 7, 10, 10, 10, 5])
    nb, m, same, band = ru.sweep_values(sweep, start, end, edges=(1.0,))
    #                                  [0,10) [0,5) [1,3) [4,6) [5,6) [5,7) [5,10) [6,10) [9,10) [2,5)
    assert list(nb) == [2, 0, 0, 1, 0, 1, 1, 0, 0, 0]       # (a breakpoint AT the region's start is not inside it)
    assert list(same[0]) == [False, True, True, False, True, True, True, True, True, True]
    assert list(band[0][same[0]]) == [1, 1, 0, 0, 0, 0, 0, 1]
    want = [(5 * 1.0 - 2.0 + 4 * 0.5) / 10, 1.0, 1.0, (1.0 - 2.0) / 2, -2.0, (-2.0 + 0.5) / 2, (-2.0 + 4 * 0.5) / 5, 0.5, 0.5, 1.0]
    assert np.array_equal(m[0].astype(np.float64), np.array(want))
    acc = ru.accumulate([sweep, sweep], start, end, edges=(1.0,))
    assert acc["N"] == 2 and list(acc["whole"]) == [0, 2, 2, 0, 2, 0, 0, 2, 2, 2] and list(acc["breaks_sq"]) == [8, 0, 0, 2, 0, 2, 2, 0, 0, 0]
    assert acc["inband"].shape == (10, 2) and list(acc["inband"][:, 1]) == [0, 2, 2, 0, 0, 0, 0, 0, 0, 2] and list(acc["inband"][:, 0]) == [0, 0, 0, 0, 2, 2, 2, 2, 2, 0]
    # D = 2 over P = 2 parameters: state s uses parameter s % 2 in dimension 0 and s // 2 in dimension 1
    sweep2 = (np.array([0, 4, 8]), np.array([1, 2]), np.array([3.0, -1.0], np.float32))
    nb, m, same, band = ru.sweep_values(sweep2, [0, 2], [8, 4], edges=(0.0,), D=2, P=2)
    assert list(nb) == [1, 0] and np.array_equal(m.astype(np.float64), [[1.0, -1.0], [1.0, 3.0]])
    assert np.array_equal(same, [[False, True], [False, True]]) and list(band[:, 1]) == [0, 1]
    assert ru.accumulate([sweep2], [0, 2], [8, 4], edges=(), D=2, P=2)["inband"].shape == (2, 0)
    # the bound: from T, B, N, max |mean| and the length alone
    b_sum, b_sq = ru.bounds([sweep], [0, 5], [10, 6])
    u = 2.0 ** -53
    assert np.allclose(b_sum, [2 * 8 * u * 10 * 2.0 / 10 + u * 2.0, 2 * 8 * u * 10 * 2.0 / 1 + u * 2.0], rtol=1e-12)
    e = 2 * 8 * u * 10 * 2.0 / 10
    assert np.allclose(b_sq[0], 2 * 2.0 * e + e * e + 2 * u * 4.0, rtol=1e-12)


def test_k3_has_something_to_find():
    """case k3 (T = 10^5, F 30 1, edges -0.5 and 0.5) on the checker alone, 400 random regions each of 10, 100, 1000 and 10 000
    positions: regions that are whole in some recorded sweeps and cut in others; regions wholly in one band in some sweeps
    only; regions that lie in one band more often than they are whole (runs of different states in one band); and a positive
    spread of the mean level in every region - none of which the per-position marginals hold"""
    c = bc.CASES["k3"]
    sweeps = bc.sweeps_of("k3")
    T, N = c["T"], len(sweeps)
    assert N == 30 and c["edges"] == (-0.5, 0.5)
    rng = np.random.RandomState(1)
    more_in_band = 0
    for length in (10, 100, 1000, 10000):
        a = rng.randint(0, T - length + 1, size=400)
        acc = ru.accumulate(sweeps, a, a + length, c["edges"])
        whole, inband = acc["whole"].astype(np.int64), acc["inband"].astype(np.int64).sum(axis=1)
        assert np.sum((whole > 0) & (whole < N)) >= 2, length
        assert np.sum((inband > 0) & (inband < N)) >= 2, length
        assert np.all(inband >= whole) and np.all(inband <= N)
        if length >= 100:
            assert np.sum(inband > whole) >= 5, length
        more_in_band += int(np.sum(inband > whole))
        mean = acc["level_sum"][0] / N
        assert np.all(acc["level_sq"][0] / N - mean * mean > 0), length
        # an off-by-one in an overlap or a wrong block at an end moves a region's mean by |level difference| / length, far above the bound
        assert acc["bound_sum"].max() < 1e-7 and acc["bound_sum"].max() * 1e3 < 1.0 / length
        s = acc["breaks_sum"].astype(np.int64)
        assert np.all(acc["breaks_sq"].astype(np.int64) >= s) and np.all((s == 0) == (whole == N))
    assert more_in_band >= 50


@pytest.mark.parametrize("T", sorted(ru.EDGE_B))
def test_chunk_edge_traces_reach_their_block_counts(T):
    """the traces of test_regions_at_chunk_edges on the checker: every sweep has the number of blocks the test is about, runs
    of equal states among them, and breakpoints to count"""
    c = ru.edge_case(T)
    o = bc.checker(c)
    try:
        sweeps = bc.checker_sweeps(o, c["scheme"])
    finally:
        o.close()
    assert len(sweeps) == 6 and all(len(s[1]) == ru.EDGE_B[T] for s in sweeps)
    changes = [int(np.sum(s[1][1:] != s[1][:-1])) for s in sweeps]
    assert min(changes) >= 1
    if 63 <= T <= 257:
        assert 20 <= min(changes) and max(changes) < T - 1          # runs of equal states, and many of them
    start, end = ru.edge_regions(T)
    assert np.all(start < end) and np.all(end <= T) and len(start) >= 3
    acc = ru.accumulate(sweeps, start, end, c["edges"])
    assert np.any(acc["whole"] == 6) and np.any(acc["whole"] == 0)
    assert np.any((acc["whole"] > 0) & (acc["whole"] < 6)) or T <= 2


def test_saturation_rule_of_the_helpers():
    from hammlet_amd import capi
    top = ru.U64_MAX
    a = np.array([0, 5, top - 3, top - 3, top, top], np.uint64)
    b = np.array([7, top - 5, 3, 4, 0, top], np.uint64)
    assert [int(v) for v in ru.sat_add(a, b)] == [7, top, top, top, top, top]
    sums = dict(N=4, whole=np.array([1, 0], np.uint64), breaks_sum=np.array([6, 2 ** 33], np.uint64), breaks_sq=np.array([14, top], np.uint64),
                level_sum=np.array([[2.0, 4.0]]), level_sq=np.array([[1.5, 4.0]]), inband=np.array([[4, 0, 0], [1, 2, 0]], np.uint64))
    s = capi.regions_summary(sums)
    assert list(s["p_whole"]) == [0.25, 0.0] and list(s["breaks_mean"]) == [1.5, 2.0 ** 31]
    assert s["breaks_sd"][0] == np.sqrt(14 / 4 - 1.5 * 1.5) and np.isnan(s["breaks_sd"][1])       # saturated: no spread
    assert np.array_equal(s["level_mean"], [[0.5, 1.0]]) and np.array_equal(s["level_sd"], [[np.sqrt(1.5 / 4 - 0.25), 0.0]])
    assert np.array_equal(s["p_inband"], [[1.0, 0.0, 0.0], [0.25, 0.5, 0.0]])
    none = capi.regions_summary(dict(sums, N=0))
    assert all(np.all(np.isnan(none[k])) for k in ("p_whole", "breaks_mean", "breaks_sd", "level_mean", "level_sd", "p_inband"))


@pytest.fixture(scope="module")
def cli():
    from hammlet_amd import build
    build.build_cli()
    return CLI


@pytest.mark.parametrize("text,message", ru.MALFORMED)
def test_driver_refuses_a_malformed_regions_file(cli, tmp_path, text, message):
    """every malformed file is an error in the driver's style, raised before the GPU is touched and before any output file
    exists; a good line in front of the bad one changes nothing"""
    raw = str(tmp_path / "in.f32")
    np.zeros(2000, np.float32).tofile(raw)
    fn = ru.write_malformed(str(tmp_path), text)
    r = subprocess.run([cli, "-raw", raw, "-o", str(tmp_path / "g-"), ".csv", "-a", "-w", "-s", "3", "-R", "1", "-i", "F", "2", "1",
                        "-regions", fn, "-O", "RG"], capture_output=True, text=True)
    assert r.returncode == 1 and message in r.stderr, r.stderr
    assert r.stderr.startswith("\n[ERROR] ") and r.stderr.endswith("!\nTerminating HaMMLET. The rest is silence.\n")
    assert [f for f in os.listdir(str(tmp_path)) if f.startswith("g-")] == []


def test_driver_needs_the_regions_for_their_output(cli, tmp_path):
    raw = str(tmp_path / "in.f32")
    np.zeros(2000, np.float32).tofile(raw)
    r = subprocess.run([cli, "-raw", raw, "-o", str(tmp_path / "g-"), ".csv", "-a", "-s", "3", "-i", "F", "2", "1", "-O", "regions"],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "give them with -regions FILE" in r.stderr
    assert "-regions FILE" in subprocess.run([cli, "-h"], capture_output=True, text=True).stdout


def test_regions_text_helpers_round_trip():
    text = ru.regions_file_text([0, 7], [5, 9], ["BRCA2 exon 3", ""])
    assert text == "# start end label\n\n0 5 BRCA2 exon 3\n7 9\n"
    out = ru.parse_output("0\t5\t15\t3\t1.5\t0.5\t0.25\t0.125\t1\t2\t3\tBRCA2 exon 3\n7\t9\t15\t15\t0\t0\t-1\t0\t0\t15\t0\t\n", D=1, ncol=3)
    assert list(out["start"]) == [0, 7] and list(out["whole"]) == [3, 15] and out["label"] == ["BRCA2 exon 3", ""]
    assert np.array_equal(out["inband"], [[1, 2, 3], [0, 15, 0]]) and np.array_equal(out["level_mean"], [[0.25, -1.0]])


def test_set_regions_refuses_positions_that_would_wrap():
    """Chain.set_regions checks the range before it casts to uint32: nothing wraps silently into another region"""
    from hammlet_amd import capi
    ok = capi._region_positions([0, 5, 2 ** 32 - 1], "start")
    assert ok.dtype == np.uint32 and list(ok) == [0, 5, 2 ** 32 - 1]
    assert list(capi._region_positions(np.array([3.0, 4.0]), "end")) == [3, 4] and capi._region_positions((), "end").shape == (0,)
    for bad in ([-1, 5], [0, 2 ** 32], np.array([1.5]), np.array([np.nan]), [[1, 2]], np.array([-3], np.int64)):
        with pytest.raises(ValueError):
            capi._region_positions(bad, "start")
