#!/usr/bin/env python3
"""Compare two device assembly files (hipcc --cuda-device-only -S) function by function, comments and label numbers stripped.
   tools/asm_functions_diff.py parent.s this.s   -> how many functions are identical, and the names of those that differ or
   exist on one side only."""
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path, errors="replace"):
        line = line.split(";", 1)[0].rstrip()
        if not line.strip():
            continue
        m = re.match(r"^(\w+):\s*$", line)
        if m and not line.startswith(".L"):
            name, body = m.group(1), []
            out[name] = body
            continue
        if name is None:
            continue
        if line.strip().startswith(".size") or line.strip() == ".end_amdhsa_kernel":
            name = None
            continue
        line = re.sub(r"\.L(BB|tmp|func_end|func_begin|JTI)?\d+(_\d+)?", ".L", line)
        if re.match(r"^\s*\.(loc|file|cfi_|p2align|section|type|globl|protected|weak)", line):
            continue
        body.append(line.strip())
    return out


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    same = [n for n in a if n in b and a[n] == b[n]]
    differ = [n for n in a if n in b and a[n] != b[n]]
    print("%d functions in %s, %d in %s: %d identical" % (len(a), sys.argv[1], len(b), sys.argv[2], len(same)))
    for n in differ:
        print("  differs:", n)
    for n in a:
        if n not in b:
            print("  only in the first:", n)
    for n in b:
        if n not in a:
            print("  only in the second:", n)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
