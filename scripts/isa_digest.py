#!/usr/bin/env python3
"""Per-kernel digest of hipcc's device assembly, and a before / after comparison of two sets of such files.

    python scripts/isa_digest.py digest FILE.s [FILE.s ...]
    python scripts/isa_digest.py compare BEFORE_DIR AFTER_DIR [-o TABLE.txt]

The .s files come from the compile of ``wedetect_amd.build.check_isa`` (``-S --cuda-device-only``, the release flags
without ``-fPIC``).  For every kernel symbol the digest holds the seven numbers of its metadata record and of the
function's trailer — .vgpr_count, .sgpr_count, .agpr_count, .group_segment_fixed_size, .private_segment_fixed_size,
.kernarg_segment_size, codeLenInByte — and two hashes of its instruction lines: in order, and sorted with label names
and branch targets replaced by one token.  ``compare`` pairs the files of the two directories by name and gives each
kernel a verdict:

    identical   the in-order hashes are equal
    reordered   only the sorted hashes are equal: the same instructions, neighbours swapped or blocks moved
    DIFFERENT   neither (or one of the seven numbers moved)

and exits non-zero if a kernel is DIFFERENT or the two sets of kernel symbols are not equal.  Lines that carry the
per-compile ``__hip_cuid_`` symbol lie outside the kernels and are dropped; everything else hipcc writes is deterministic.
This script hashes and compares; it looks for no instruction in particular.
"""
from __future__ import annotations

import argparse
import hashlib
import os
import re
import sys

META = ("vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
        "kernarg_segment_size")
NUMBERS = META + ("codeLenInByte",)
_LABEL = re.compile(r"\.L[A-Za-z_]*\d+(?:_\d+)?")


def _sha(lines) -> str:
    h = hashlib.sha256()
    for ln in lines:
        h.update(ln.encode())
        h.update(b"\n")
    return h.hexdigest()[:16]


def digest(path: str) -> dict:
    """{kernel symbol: {the seven numbers, 'n_instr', 'ordered', 'sorted'}} of one .s file."""
    lines = [ln.rstrip("\n") for ln in open(path) if "__hip_cuid_" not in ln]
    kernels = [ln.split()[1] for ln in lines if ln.startswith("\t.amdhsa_kernel ")]
    out = {k: {} for k in kernels}
    # function bodies: from "SYMBOL:" to its ".Lfunc_end"; "; codeLenInByte" follows in the trailer comments
    cur, last, body = None, None, []
    for ln in lines:
        if cur is None:
            head = ln.split(":")[0]
            if ln[:1] not in ("\t", " ", ";", ".") and head in out and ln[len(head):len(head) + 1] == ":":
                cur, body = head, []
            elif ln.startswith("; codeLenInByte = ") and last is not None:
                out[last]["codeLenInByte"] = int(ln.split("=")[1])    # the trailer of the kernel that just ended
                last = None
            continue
        if ln.startswith(".Lfunc_end"):
            out[cur].update(n_instr=len(body), ordered=_sha(body), sorted=_sha(sorted(_LABEL.sub("L", b) for b in body)))
            cur, last = None, cur
            continue
        if not ln.startswith("\t"):
            continue                                                  # labels, block comments
        ins = ln.split(";")[0].strip()
        if ins and not ins.startswith("."):                           # drop assembler directives
            body.append(" ".join(ins.split()))
    # metadata records: "  - .agpr_count:" opens one, its own keys sit at four spaces
    if "amdhsa.kernels:" in lines:
        rec = None
        recs = []
        for ln in lines[lines.index("amdhsa.kernels:") + 1:]:
            m = re.match(r"^  - \.(\w+):\s*(.*)$", ln)
            if m:
                rec = {m.group(1): m.group(2)}
                recs.append(rec)
                continue
            m = re.match(r"^    \.(\w+):\s*(.*)$", ln)
            if m and rec is not None:
                rec[m.group(1)] = m.group(2)
            elif not ln.startswith(" "):
                break
        for rec in recs:
            if rec.get("name") in out:
                for key in META:
                    out[rec["name"]][key] = int(rec[key])
    for k, d in out.items():
        missing = [n for n in NUMBERS + ("ordered", "sorted") if n not in d]
        if missing:
            raise RuntimeError(f"{path}: kernel {k}: no {missing} found")
    return out


def _fmt(d: dict) -> str:
    return " ".join(str(d[n]) for n in NUMBERS) + f" {d['ordered']} {d['sorted']}"


def verdict(a: dict, b: dict) -> str:
    if any(a[n] != b[n] for n in NUMBERS):
        return "DIFFERENT"
    if a["ordered"] == b["ordered"]:
        return "identical"
    return "reordered" if a["sorted"] == b["sorted"] else "DIFFERENT"


def compare(before_dir: str, after_dir: str, out) -> int:
    bad = 0
    names = sorted(f for f in os.listdir(after_dir) if f.endswith(".s"))
    print("# per kernel: " + " ".join("." + n if n != "codeLenInByte" else n for n in NUMBERS) +
          " sha256/16(instructions in order) sha256/16(instructions sorted, labels normalised)", file=out)
    for f in names:
        if not os.path.exists(os.path.join(before_dir, f)):
            print(f"\n== {f}: no file before", file=out)
            bad += 1
            continue
        a, b = digest(os.path.join(before_dir, f)), digest(os.path.join(after_dir, f))
        counts = {"identical": 0, "reordered": 0, "DIFFERENT": 0}
        rows = []
        for k in sorted(set(a) | set(b)):
            if k not in a or k not in b:
                rows.append(f"{k}\n    only {'after' if k in b else 'before'}: MISSING")
                bad += 1
                continue
            v = verdict(a[k], b[k])
            counts[v] += 1
            bad += v == "DIFFERENT"
            if v == "identical":
                rows.append(f"{k}\n    both    {_fmt(a[k])}  identical")
            else:
                rows.append(f"{k}\n    before  {_fmt(a[k])}\n    after   {_fmt(b[k])}  {v}")
        print(f"\n== {f}: {len(b)} kernels, " + ", ".join(f"{n} {v}" for v, n in counts.items()), file=out)
        for r in rows:
            print(r, file=out)
    return bad


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    d = sub.add_parser("digest")
    d.add_argument("files", nargs="+")
    c = sub.add_parser("compare")
    c.add_argument("before")
    c.add_argument("after")
    c.add_argument("-o", "--output")
    args = ap.parse_args()
    if args.cmd == "digest":
        for f in args.files:
            print(f"== {os.path.basename(f)}")
            for k, dd in sorted(digest(f).items()):
                print(f"{k}\n    {_fmt(dd)}")
        return 0
    out = open(args.output, "w") if args.output else sys.stdout
    bad = compare(args.before, args.after, out)
    if args.output:
        out.close()
        print(f"{args.output}: {bad} kernels DIFFERENT or missing")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
