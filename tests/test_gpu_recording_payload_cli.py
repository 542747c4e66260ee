"""`hammlet -chains N -merge-gpus` (extension): the levels, breakpoints, consensus, bands, bandcalls and rhat files of chains whose
recordings are merged through sparse payloads (hml_recording_merge_across, shadow contexts for R-hat).  On one GPU the flag takes
the payload path for every merge and every shadow, and the six files must be those of the run without it, byte for byte."""
import subprocess

import pytest

from tests import cli_util
from tests.cli_util import CLI
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu
T, K, SEED = 100000, 3, 4
FILES = ["levels", "breakpoints", "consensus", "bands", "bandcalls", "rhat"]


def run_cli(tmp, x, flags, outputs, prefix):
    """the chains of these runs share the first GPU"""
    return cli_util.run_cli(tmp, x, flags, outputs, one_gpu=True, prefix=prefix)


def test_cli_merge_gpus_writes_the_same_files_on_one_gpu(tmp_path):
    x = ol.trace(T, K, 1)
    flags = "-s %d -R %d -chains 3 -i F 40 2 -bands -0.5 0.5" % (K, SEED)
    outputs = ["L", "BP", "CS", "LB", "LC", "R"]
    plain = run_cli(str(tmp_path), x, flags, outputs, "p-")
    assert plain.returncode == 0, plain.stderr
    merged = run_cli(str(tmp_path), x, flags + " -merge-gpus", outputs, "m-")
    assert merged.returncode == 0, merged.stderr
    for name in FILES:
        a = open(str(tmp_path / ("p-%s.csv" % name)), "rb").read()
        b = open(str(tmp_path / ("m-%s.csv" % name)), "rb").read()
        assert len(a) > 0 and a == b, name
    assert len(open(str(tmp_path / "m-levels.csv")).read().splitlines()) > 1
    assert len(open(str(tmp_path / "m-rhat.csv")).read().splitlines()) > 1


def test_cli_help_names_the_flag():
    r = subprocess.run([CLI, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and "-merge-gpus" in r.stdout
