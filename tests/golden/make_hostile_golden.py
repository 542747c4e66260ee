#!/usr/bin/env python3
"""Golden files for inputs that are not a unit-scale Gaussian trace (tests/hostile_inputs.py): the UNMODIFIED reference binary
(oracle/_ref/hammlet, built by oracle/Makefile from the reference's src/main.cpp) on every input of that module - scaled by
2^+-10, 2^+-40 and 10^+-3, shifted by 10 / 100 / 1000, read depths of 1 to 5000 with 3 to 20 states, integer data full of ties,
spikes of +-10^3, 2 to 65 positions - plus two read-depth runs of 10^6 positions (dynamic and static block structure), and the
reference's message and exit status for the inputs it refuses.

Only runs where the reference sources exist (the build container).  Committed under tests/golden/hostile/ are two files:
manifest.json - per case the flags, the sha256 of the float32 input the tests regenerate, the reference's exit status, stdout and
stderr, and for every output (`marginals`, `parameters`, `compression`; `blocks` and `sequences` below 10^5 positions) its size,
line count and sha256 - and outputs.tar.xz, the outputs themselves (data, not source) as <case>/<output>.csv, except those that
still take more than 64 KiB when compressed alone: these are held by their sha256 only, which pins every byte just the same.

    python tests/golden/make_hostile_golden.py [case ...]
"""
import ctypes as C
import hashlib
import io
import json
import lzma
import os
import subprocess
import sys
import tarfile
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from tests import hostile_inputs as hi  # noqa: E402
from tests import oracle_lib as ol  # noqa: E402

REF = os.path.join(REPO, "oracle", "_ref", "hammlet")
LIMIT = 64 << 10


def write_archive(members):
    """a tar.xz that depends on nothing but its members' names and bytes"""
    raw = io.BytesIO()
    with tarfile.open(fileobj=raw, mode="w", format=tarfile.USTAR_FORMAT) as tar:
        for name in sorted(members):
            info = tarfile.TarInfo(name)
            info.size = len(members[name])
            tar.addfile(info, io.BytesIO(members[name]))
    with open(hi.ARCHIVE, "wb") as f:
        f.write(lzma.compress(raw.getvalue(), preset=9 | lzma.PRESET_EXTREME))


def main():
    if not os.path.exists(REF):
        raise SystemExit("reference binary missing: run `make -C oracle ref` in the build container")
    lib = ol.load()
    lib.orc_write_text.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p, C.c_int]
    os.makedirs(hi.GOLDEN, exist_ok=True)
    mpath = os.path.join(hi.GOLDEN, "manifest.json")
    manifest = hi.manifest() if os.path.exists(mpath) else {}
    members = hi.archive() if os.path.exists(hi.ARCHIVE) else {}
    for name in sys.argv[1:] or list(hi.INPUTS) + list(hi.MILLION):
        x, flags, outs = hi.case_input(name)
        entry = {"T": int(x.size), "flags": flags, "input_sha256": hi.sha256(x)}
        with tempfile.TemporaryDirectory() as tmp:
            inp = os.path.join(tmp, "in.txt")
            assert lib.orc_write_text(x.ctypes.data, x.size, inp.encode(), 8) == 0
            cmd = [REF, "-f", inp, "-o", os.path.join(tmp, "ref-"), ".csv", "-w", "-a"] + flags.split() + ["-O"] + outs
            r = subprocess.run(cmd, capture_output=True, text=True)
            entry["status"], entry["stdout"], entry["stderr"] = r.returncode, r.stdout, r.stderr
            assert (r.returncode != 0) == (name in hi.REFUSED), (name, r.stderr)
            entry["outputs"] = [] if r.returncode else outs
            entry["files"] = {}
            for o in entry["outputs"]:
                with open(os.path.join(tmp, "ref-%s.csv" % o), "rb") as f:
                    data = f.read()
                member = "%s/%s.csv" % (name, o)
                members.pop(member, None)
                stored = len(lzma.compress(data, preset=9 | lzma.PRESET_EXTREME)) <= LIMIT
                if stored:
                    members[member] = data
                entry["files"][o] = {"stored": stored, "bytes": len(data), "sha256": hashlib.sha256(data).hexdigest(), "lines": data.count(b"\n")}
        manifest[name] = entry
        print(name, "ok", {o: e["bytes"] for o, e in entry["files"].items()} or entry["stderr"], flush=True)
    with open(mpath, "w") as f:   # one case a line
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(manifest[k], sort_keys=True)) for k in sorted(manifest)) + "\n}\n")
    write_archive(members)


if __name__ == "__main__":
    main()
