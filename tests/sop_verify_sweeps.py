"""Generators shared by the sum-of-products sumcheck verifier's sweeps (test_sop_verify_host.py on the CPU,
test_gpu_sop_verify.py on the device), after product_verify_sweeps.py, whose helpers they reuse: every single-element change of a
transcript of gkr_sumcheck_sop* and of its tables, and the closed-form model of the verdict
gkr_sumcheck_sop_verify_batch_device gives it.

A transcript is (C, L, R): n rows of D + 1 right-aligned slots (D the largest term degree), n lengths, n challenges, with its M
tables of 2^n entries, the terms [(coeff, (table indices ..)), ..] and, optionally, the claimed sum.  The slot, r, len and claim
cases and their verdicts are the product sweep's (product_verify_sweeps.cases: the checks before the last one do not look at the
tables).  The table case has ONE rule:

  * entry i of table m + 1 moves e_m = T_m~(r) to e_m + eq(r, i) and nothing else; the verdict is (EVALUATION, n) iff
    sop_eval of the changed values differs from sop_eval(evals), computed exactly, and ACCEPTED otherwise.

A table that stands twice in a term (a square), terms that cancel (AB - AB: no change of any table shows) and a table whose
cofactor vanishes (AB - AC with B = C: A's cofactor is e_B - e_C = 0) all follow from it.
"""

from typing import List, Optional, Tuple

from gkr_amd.field import MODULUS as P, from_limbs
from mle_verify_sweeps import ACCEPTED, CHALLENGE, EVALUATION, NON_CANONICAL, OK, ROUND_SUM, SHAPE, eq_weight
from product_verify_sweeps import (Case, arrays_of, assert_sweep_is_sharp, assert_sweep_reaches_short_rows, build_batch,  # noqa: F401
                                   cases as product_cases, point_sees, rounds_of)
from sop_model import sop_degree, sop_eval
from verify_sweeps import value


def cases(C, L, R, evals: List[int], terms, with_claim: bool, table_positions=None) -> List[Case]:
    """Every tampering of the list above for one transcript whose M tables have the values `evals` at the challenges, and one
    honest copy in front and at the end.  table_positions: the entries changed in every table (all)."""
    n, D = L.shape[0], C.shape[1] - 1
    assert D == sop_degree(terms) and all(0 <= m < len(evals) for _, idx in terms for m in idx)
    out = product_cases(C, L, R, [1] * D, with_claim, table_positions=())[:-1]   # (no table cases: they follow)
    assert not any(c.what == "table" for c in out)
    r = from_limbs(R)
    honest = sop_eval(evals, terms)
    for m in range(len(evals)):
        for i in (range(1 << n) if table_positions is None else table_positions):
            changed = list(evals)
            changed[m] = (evals[m] + eq_weight(r, i)) % P
            out.append(Case("table", (m, i), "plus1", (False, n, EVALUATION) if sop_eval(changed, terms) != honest else ACCEPTED))
    out.append(Case("honest", (), None, ACCEPTED))
    return out


def reference_verdict(tables: List[List[int]], terms, C, L, R, claim: Optional[int], multi_hash) -> Tuple[bool, int, int]:
    """The four checks of include/gkr_amd.h one after the other on Python integers (multi_hash: gkr_amd.multi_hash); the last
    one folds every table with the challenges and calls sop_model.sop_eval."""
    n, W = L.shape[0], C.shape[1]
    assert W == sop_degree(terms) + 1
    for j in range(n):                                                   # 1. shape
        if not 1 <= int(L[j]) <= W:
            return False, j, SHAPE
    if claim is not None and claim >= P:                                 # 2. canonical: the claim, then row by row
        return False, 0, NON_CANONICAL
    rows = []
    for j in range(n):
        g = [value(C[j, t]) for t in range(W - int(L[j]), W)]
        if any(x >= P for x in g) or value(R[j]) >= P:
            return False, j, NON_CANONICAL
        rows.append(g)
    rs = [value(x) for x in R]
    running = claim
    for j, g in enumerate(rows):                                         # 3. the rounds
        if running is not None and (g[-1] + sum(g)) % P != running:      # g(0) + g(1) = 2 c_0 + c_1 + ..
            return False, j, ROUND_SUM
        if multi_hash(g, 0) != rs[j]:
            return False, j, CHALLENGE
        running = 0
        for c in g:
            running = (running * rs[j] + c) % P
    evals = []                                                           # 4. the tables
    for table in tables:
        t = [x % P for x in table]
        for r in rs:
            half = len(t) // 2
            t = [(t[i] + r * (t[i + half] - t[i])) % P for i in range(half)]
        evals.append(t[0])
    return (True, 0, OK) if running == sop_eval(evals, terms) else (False, n, EVALUATION)


def table_verdicts(sweep: List[Case], m: int):
    """The set of verdicts of the sweep's changes of table m."""
    return {c.verdict for c in sweep if c.what == "table" and c.index[0] == m}
