#!/usr/bin/env python3
"""Generate tests/golden/sop_sumcheck.json by running the REFERENCE'S OWN Python prover on sums of products of extensions.

Run in the build container only (needs the reference checkout make_golden.py names; nothing under tests/ reads it at test
time -- the JSON file is the fixture):

    python tests/golden/make_golden_sop.py

What is executed: the reference's python/{poly,sumcheck}.py, imported unmodified through make_golden.py (its ``ethsnarks``
stand-in, its ``table_func``): ``g = get_ext(A) * get_ext(B) + (-1) get_ext(C)`` and ``g = get_ext(eq) * get_ext(A) * get_ext(B)
+ (-1) get_ext(eq) * get_ext(C)``, then ``prove_sumcheck(g, n, 1)``.  Random tables only: the Python prover keeps structural
leading zeros that the Rust one drops, and random tables stay where both agree.  Each round vector's leading constant slot is
asserted zero and dropped, as make_golden.py does for its own fixtures.
"""

import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg      # noqa: E402  (installs the stand-in, imports the reference modules; main() is not run)

# (name, n, number of tables, terms as [coefficient, table indices]; table 0 of the "eq" cases is eq(z, .))
CASES = [("AB-C", 2), ("AB-C", 3), ("AB-C", 4), ("eq(AB-C)", 2), ("eq(AB-C)", 3)]
TERMS = {"AB-C": (3, [[1, [0, 1]], [-1, [2]]]), "eq(AB-C)": (4, [[1, [0, 1, 2]], [-1, [0, 3]]])}


def scaled(poly, c):
    c = mg.FQ(c)
    return mg.ref_poly.polynomial([mg.ref_poly.monomial(m.coeff * c, m.terms) for m in poly.terms], poly.constant * c)


def eq_table(z, n):
    out = []
    for i in range(1 << n):
        v = 1
        for j in range(n):
            v = v * (z[j] if (i >> (n - 1 - j)) & 1 else 1 - z[j]) % mg.P
        out.append(v)
    return out


def main():
    rng = random.Random(0xC0FFEE + 1500)
    cases = []
    for name, n in CASES:
        n_tables, terms = TERMS[name]
        tables = [[rng.randrange(mg.P) for _ in range(1 << n)] for _ in range(n_tables)]
        z = None
        if name.startswith("eq"):
            z = [rng.randrange(mg.P) for _ in range(n)]
            tables[0] = eq_table(z, n)
        ext = [mg.ref_poly.get_ext(mg.table_func(t, n), n) for t in tables]
        g = None
        for c, idx in terms:
            prod = ext[idx[0]]
            for i in idx[1:]:
                prod = prod * ext[i]
            prod = scaled(prod, c)
            g = prod if g is None else g + prod
        proof, r = mg.ref_sumcheck.prove_sumcheck(g, n, 1)
        for vec in proof:
            assert int(vec[0]) == 0
        claim = 0
        for i in range(1 << n):
            for c, idx in terms:
                v = c
                for m in idx:
                    v = v * tables[m][i] % mg.P
                claim = (claim + v) % mg.P
        assert mg.ref_sumcheck.verify_sumcheck(mg.FQ(claim), proof, r, n)
        cases.append({"name": name, "n": n, "terms": [[mg.S(c % mg.P), idx] for c, idx in terms], "z": [mg.S(x) for x in z] if z else None,
                      "tables": [[mg.S(x) for x in t] for t in tables],
                      "proof": [[mg.S(x) for x in vec[1:]] for vec in proof], "r": [mg.S(x) for x in r], "claim": mg.S(claim)})
        print("case %s n=%d ok" % (name, n))
    with open(os.path.join(HERE, "sop_sumcheck.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_sop.py", "modulus": mg.S(mg.P), "cases": cases}, f, indent=1)
    print("wrote", len(cases), "sum-of-products cases")


if __name__ == "__main__":
    main()
