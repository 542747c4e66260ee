"""include/hammlet/Records.hpp on the host: MarginalSegmentSets::addSweep (the `segments` side file) with a sweep of no runs
or a trace of no positions - next to where inputs of a handful of positions walk - compiled with bounds-checked vectors."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include "hammlet/hammlet.hpp"
int main() {
    hammlet::MarginalSegmentSets s;
    const std::vector<uint32_t> none;
    const std::vector<int16_t> nostate;
    if (s.addSweep(none, nostate, 0) != 0 || s.nrSegments() != 1) return 1;
    if (s.addSweep(none, nostate, 100) != 0 || s.nrSegments() != 1) return 2;     // no runs: runStart[R - 1] must not be read
    if (s.addSweep({0}, {1}, 0) != 0 || s.nrSegments() != 1) return 3;            // no positions: the one segment stays
    // two runs over ten positions: segments {0}, {1}; before the last run is added the queue holds {0} (one count and a
    // terminator) and the still empty second segment (a terminator)
    if (s.addSweep({0, 5}, {0, 1}, 10) != 3 || s.nrSegments() != 2) return 4;
    if (s.addSweep(none, nostate, 10) != 0 || s.nrSegments() != 2) return 5;      // ... and an empty sweep leaves them alone
    // one position, one run: the tiniest recorded sweep
    hammlet::MarginalSegmentSets t;
    if (t.addSweep({0}, {3}, 1) != 1 || t.nrSegments() != 1) return 6;
    std::puts("ok");
    return 0;
}
"""


def test_add_sweep_without_runs_or_positions(tmp_path):
    src = tmp_path / "records_edge.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "records_edge")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-D_GLIBCXX_ASSERTIONS", "-I", os.path.join(REPO, "include"), "-o", exe, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.returncode, r.stderr)
