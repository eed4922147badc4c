#!/usr/bin/env python3
"""Compare the kernels of two device-only assembly listings (hipcc ... --cuda-device-only -S) by name.

    tools/isa_diff.py before.s after.s [more_after.s ...]

Per kernel found on both sides: SAME or DIFF of the instruction stream (comments stripped, the compiler's local label
numbers normalised) and of the register / LDS / scratch metadata (a DIFF is followed by a `->` line with the `after` side's
line count and metadata).  A text comparison and nothing more.  Exit status 1 on
any DIFF or on a kernel of `before.s` that no `after` file defines."""
import re
import sys

LABEL = re.compile(r"\.(LBB|Ltmp|Lfunc_begin|Lfunc_end|LJTI)\d+(_?)")
META = (".sgpr_count", ".vgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def kernels(path):
    """{kernel symbol: (instruction lines, metadata lines)}"""
    text = open(path).read()
    entries = text.split("amdhsa.kernels:")[1].split("amdhsa.target")[0].split("\n  - ")[1:]
    out = {}
    for entry in entries:
        name = re.search(r"^\s*\.name:\s+(\S+)", entry, flags=re.M).group(1)
        body = re.search(r"^%s:[^\n]*\n(.*?)^\s*\.section\s+\.rodata" % re.escape(name), text, flags=re.M | re.S).group(1)
        lines = []
        for ln in body.split("\n"):
            ln = LABEL.sub(r".\1#\2", ln.split(";")[0]).strip()
            if ln:
                lines.append(ln)
        meta = sorted(m.strip() for m in entry.split("\n") if m.strip().startswith(META))
        out[name] = (lines, meta)
    return out


def main():
    before, after = kernels(sys.argv[1]), {}
    for p in sys.argv[2:]:
        after.update(kernels(p))
    bad = 0
    for name, (code, meta) in sorted(before.items()):
        if name not in after:
            verdict = "MISSING"
        else:
            verdict = "SAME" if (code, meta) == after[name] else "DIFF"
        bad += verdict != "SAME"
        print("%-8s %6d lines  %s  %s" % (verdict, len(code), " ".join(meta), name))
        if verdict == "DIFF":
            print("%-8s %6d lines  %s" % ("  ->", len(after[name][0]), " ".join(after[name][1])))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
