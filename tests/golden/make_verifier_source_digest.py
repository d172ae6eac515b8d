#!/usr/bin/env python3
"""Writes tests/golden/verifier_source.json: the sha256 of the verifier components' circom text as the reference's
modify_circom_file (rust/src/aggregator.rs:215-314) renders it for three meta vectors.  Run where the reference tree
is available (pass its root as the argument; the text itself is not committed, only its digest):

    python tests/golden/make_verifier_source_digest.py <reference-root>

Its two template strings (`let verifiers = "..."`, `let source = "..."`) are read out of aggregator.rs and rendered with
a three-line substitute for tera ({{ name }} -> value), each source appended as `format!("{}\\n{}", v, s)` (:289).
tests/test_circom_input.py holds gkr_amd.aggregate.verifier_source against the digest.
"""
import hashlib
import json
import os
import re
import sys

METAS = [[4, 7, 5, 0, 3, 8, 12, 7, 5, 6, 7, 7], [3, 2, 0, 1, 2, 3, 4, 2, 0, 2, 2], [6, 6, 5, 0, 3, 7, 40, 6, 5, 6, 6, 6, 6, 6]]


def render_reference(aggregator_rs, metas):
    rust = open(aggregator_rs).read()
    verifiers_tpl = re.search(r'let verifiers = "(.*?)";', rust, re.S).group(1)
    source_tpl = re.search(r'let source = "(.*?)";', rust, re.S).group(1)
    render = lambda tpl, ctx: re.sub(r"\{\{\s*(\w+)\s*\}\}", lambda m: ctx[m.group(1)], tpl)
    text = render(verifiers_tpl, {"total": str(len(metas))})
    for i, m in enumerate(metas):
        ctx = {"num": str(i), "meta": "[" + ", ".join(map(str, m)) + "]"}
        ctx.update({"meta_%d" % j: str(v) for j, v in enumerate(m)})
        text = "%s\n%s" % (text, render(source_tpl, ctx))
    return text


if __name__ == "__main__":
    text = render_reference(os.path.join(sys.argv[1], "rust", "src", "aggregator.rs"), METAS)
    out = {"what": "sha256 of the reference's modify_circom_file verifier text (aggregator.rs:215-289) for `metas`, UTF-8",
           "metas": METAS, "sha256": hashlib.sha256(text.encode()).hexdigest(), "bytes": len(text.encode())}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "verifier_source.json")
    with open(path, "w") as f:
        json.dump(out, f)
        f.write("\n")
    print(path, out["sha256"])
