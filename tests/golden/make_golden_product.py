#!/usr/bin/env python3
"""Generate tests/golden/product_sumcheck.json by running the REFERENCE'S OWN Python prover on products of extensions.

Run in the build container only (needs the reference checkout make_golden.py names; nothing under tests/ reads it at test
time -- the JSON file is the fixture):

    python tests/golden/make_golden_product.py

What is executed: the reference's python/{poly,sumcheck}.py, imported unmodified through make_golden.py (its ``ethsnarks``
stand-in, its ``table_func``): ``g = get_ext(T_0) * get_ext(T_1) [* get_ext(T_2)]`` and ``prove_sumcheck(g, n, 1)``.
Each round vector's leading constant slot is asserted zero and dropped, as make_golden.py does for its own fixtures.
"""

import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg      # noqa: E402  (installs the stand-in, imports the reference modules; main() is not run)

SHAPES = [(2, 2), (3, 2), (4, 2), (5, 2), (2, 3), (3, 3), (4, 3)]      # (n, degree)


def main():
    rng = random.Random(0xC0FFEE + 600)
    cases = []
    for n, d in SHAPES:
        tables = [[rng.randrange(mg.P) for _ in range(1 << n)] for _ in range(d)]
        g = mg.ref_poly.get_ext(mg.table_func(tables[0], n), n)
        for t in tables[1:]:
            g = g * mg.ref_poly.get_ext(mg.table_func(t, n), n)
        proof, r = mg.ref_sumcheck.prove_sumcheck(g, n, 1)
        for vec in proof:
            assert int(vec[0]) == 0
        claim = 0
        for i in range(1 << n):
            term = 1
            for t in tables:
                term = term * t[i] % mg.P
            claim = (claim + term) % mg.P
        assert mg.ref_sumcheck.verify_sumcheck(mg.FQ(claim), proof, r, n)
        cases.append({"n": n, "degree": d, "tables": [[mg.S(x) for x in t] for t in tables],
                      "proof": [[mg.S(x) for x in vec[1:]] for vec in proof], "r": [mg.S(x) for x in r], "claim": mg.S(claim)})
        print("case n=%d degree=%d ok" % (n, d))
    with open(os.path.join(HERE, "product_sumcheck.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_product.py", "modulus": mg.S(mg.P), "cases": cases}, f, indent=1)
    print("wrote", len(cases), "product cases")


if __name__ == "__main__":
    main()
