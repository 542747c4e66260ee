"""The backward pass packs a map [K] -> [K] into one 64-bit word (hammlet_amd/csrc/hml_maps.h: no HIP, a host compiler builds
it): a byte per entry up to 8 states - composition is then a byte permute on the device -, 4 bits per entry beyond.  A
stand-alone program (tests/fixtures/mapfmt_main.cpp) holds, for 1 to 8 states, the byte format's compose / get / set /
broadcast / identity to the 4-bit format and to maps kept as plain arrays - all K^K x K^K pairs up to 3 states, 10^5 seeded
random pairs beyond, associativity on random triples, and after every operation the invariant that the permute relies on
(every byte of a map, unused entries included, is below 8) - and for 9 to 16 states the 4-bit format to hml_map_compose.
The host's byte loop stands in for the device's permute; that the two agree is what tests/test_gpu_backward_maps.py shows."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path, *flags):
    exe = str(tmp_path / ("mapfmt" + "".join(flags).replace("=", "_").replace(",", "_")))
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", *flags, "-I", os.path.join(REPO, "hammlet_amd", "csrc"),
                    "-o", exe, os.path.join(REPO, "tests", "fixtures", "mapfmt_main.cpp")], check=True)
    return exe


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "sanitized"])
def test_map_formats_agree_with_plain_arrays(tmp_path, flags):
    r = subprocess.run([build(tmp_path, *flags)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr + r.stdout
    lines = r.stdout.splitlines()
    assert len(lines) == 16
    for K, line in zip(range(1, 17), lines):
        w = line.split()
        assert w[0] == "K" and int(w[1]) == K and w[-1] == "ok", line
        assert w[2] == ("bytes" if K <= 8 else "nibbles"), line
        pairs, triples = int(w[4]), int(w[6])
        assert pairs == ((K ** K) ** 2 if K <= 3 else 100000), line
        assert triples == 20000, line
