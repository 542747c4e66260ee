#!/usr/bin/env python3
"""What a kernel does before it requests its first byte of data: python tools/head_waits.py FILE.s PATTERN [PATTERN ...]

FILE.s is gfx950 assembly of a sweep object: hammlet_amd/csrc/hml_sweep.hip compiled with the flags of
hammlet_amd/build.py plus `-DHML_TU_K=<k> --cuda-device-only -S`.  PATTERN is a regular expression over the (mangled)
kernel names, e.g. 'hml_k_forwardILi5' or 'hml_k_(forward|backward_maps)I'.  No GPU is needed.

Per kernel the tool walks the text from the entry to the first DATA load and prints every load, wait and barrier on
the way, then their counts.  A wait that has at least one load outstanding is a memory round trip: a kernel whose head
shows four of them pays four cold latencies, one after the other, before its own work starts.

  data load     a vector-memory load (global_/flat_/buffer_load) that is neither the 16-bit read of the workgroup size
                from the dispatch packet (global_load_ushort: listed as a load of the head, it needs a wait of its own)
                nor inside a side block.
  side block    instructions that a forward branch jumps over, at most --side-block of them (default 24), with a store
                to memory among them: a probe or a one-lane bookkeeping stamp, not the path the wavefronts take.  Its
                events are printed in brackets and not counted.  (A short guarded block WITHOUT a store is a guarded
                data load and counts.)  --side-block 0 treats every block alike.
  --until RE    the head ends at the first counted vector load whose text matches RE instead (the block kernel:
                'global_load_dword .* nt', its first summary word - the exponential table is a vector load too).

The walk is linear in the text: it does not know which side of a long branch the wavefronts take, so a kernel whose
rare path comes first in the text (the repair step of the backward chain) is read by eye from the listing.

The register figures (.vgpr_count, .sgpr_count, .sgpr_spill_count, .vgpr_spill_count) come from the code object's
metadata at the end of the file.
"""
import argparse
import re
import sys

LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
BRANCH = re.compile(r"^\s+s_cbranch_\w+\s+(\.LBB\w+)")
SLOAD = re.compile(r"^\s+(s_load_\w+|s_buffer_load_\w+)\s")
VLOAD = re.compile(r"^\s+((global|flat|buffer)_load_\w+)\s")
WAIT = re.compile(r"^\s+s_waitcnt\s+(.*)$")
BARRIER = re.compile(r"^\s+s_barrier\b")
TIME = re.compile(r"^\s+(s_memrealtime|s_memtime)\s")
LDS = re.compile(r"^\s+(ds_\w+)\s")
INSTR = re.compile(r"^\s+[a-z]\w+")
STORE = re.compile(r"^\s+(global|flat|buffer)_(store|atomic)\w*\s")
META = ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count")


def kernels(lines):
    """{name: (first line, one past the last line)} of the functions in the text"""
    out, name, start = {}, None, 0
    for i, l in enumerate(lines):
        m = LABEL.match(l)
        if m and not m.group(1).startswith("."):
            name, start = m.group(1), i + 1
        elif name and l.startswith(".Lfunc_end"):
            out[name] = (start, i)
            name = None
    return out


def metadata(lines):
    """{kernel name: {field: value}} from the amdhsa.kernels list"""
    out, cur = {}, {}
    for l in lines:
        s = l.strip()
        if s.startswith("- ."):   # a new entry of a list
            if "name" in cur and any(k in cur for k in META):
                out[cur["name"]] = cur
            if l.startswith("  - ."):
                cur = {}
            s = s[2:]
        m = re.match(r"\.(\w+):\s+(\S+)", s)
        if m and (m.group(1) in META or (m.group(1) == "name" and l.startswith("    .name:"))):
            cur[m.group(1)] = m.group(2)
    if "name" in cur and any(k in cur for k in META):
        out[cur["name"]] = cur
    return out


def head(lines, lo, hi, side_block, until):
    """events [(line number, text, counted)] from the entry to the first data load, and whether one was found"""
    labels = {}
    for i in range(lo, hi):
        m = LABEL.match(lines[i])
        if m:
            labels[m.group(1)] = i
    ev, side_until, found = [], -1, False
    for i in range(lo, hi):
        l = lines[i]
        inside = i < side_until
        m = BRANCH.match(l)
        if m and not inside and side_block > 0:
            t = labels.get(m.group(1), -1)
            body = range(i + 1, t)
            if t > i and sum(1 for j in body if INSTR.match(lines[j])) <= side_block and any(STORE.match(lines[j]) for j in body):
                side_until = t
            continue
        text = l.split(";")[0].strip()
        if SLOAD.match(l) or WAIT.match(l) or BARRIER.match(l) or TIME.match(l):
            ev.append((i + 1, text, not inside))
        elif VLOAD.match(l):
            ev.append((i + 1, text, not inside))
            if not inside and (until.search(text) if until else not VLOAD.match(l).group(1).endswith("_ushort")):
                found = True
                break
    return ev, found


def report(name, lines, span, meta, side_block, until):
    ev, found = head(lines, span[0], span[1], side_block, until)
    print("== %s" % name)
    pending = 0
    n = {"scalar loads": 0, "vector loads": 0, "waits": 0, "round trips": 0, "barriers": 0, "clock reads": 0}
    for ln, text, counted in ev:
        print(("   %7d  %s" if counted else "   %7d  [%s]") % (ln, text))
        if not counted:
            continue
        if text.startswith(("s_load", "s_buffer_load")):
            n["scalar loads"] += 1
            pending += 1
        elif text.startswith("s_waitcnt"):
            n["waits"] += 1
            if pending:
                n["round trips"] += 1
            pending = 0
        elif text.startswith("s_barrier"):
            n["barriers"] += 1
        elif text.startswith(("s_memrealtime", "s_memtime")):
            n["clock reads"] += 1
            pending += 1
        else:
            n["vector loads"] += 1
            pending += 1
    if found:
        n["vector loads"] -= 1   # the data load itself ends the head
    print("   head: " + ", ".join("%d %s" % (v, k) for k, v in n.items()) + ("" if found else "  (no data load found)"))
    m = meta.get(name, {})
    print("   registers: " + ", ".join(".%s %s" % (k, m.get(k, "?")) for k in META))
    return n


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("patterns", nargs="+")
    ap.add_argument("--side-block", type=int, default=24)
    ap.add_argument("--until", default=None)
    a = ap.parse_args()
    with open(a.asm) as f:
        lines = f.read().splitlines()
    ks, meta = kernels(lines), metadata(lines)
    hit = 0
    for pat in a.patterns:
        rx = re.compile(pat)
        for name in sorted(k for k in ks if rx.search(k)):
            report(name, lines, ks[name], meta, a.side_block, re.compile(a.until) if a.until else None)
            hit += 1
    if not hit:
        sys.exit("no kernel matches")


if __name__ == "__main__":
    main()
