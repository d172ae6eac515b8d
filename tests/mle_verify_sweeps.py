"""Generators shared by the plain-sumcheck verifier's sweeps (test_mle_verify_host.py on the CPU, test_gpu_mle_verify.py on the
device), after verify_sweeps.py: every single-element change of a transcript of prove_sumcheck and of its table, and the
closed-form model of the verdict gkr_sumcheck_mle_verify_batch_device gives it.

A transcript is (C, L, R): n rows of two right-aligned slots, n lengths in {1, 2}, n challenges (uint64 limbs), with the
table's 2^n entries and, optionally, the claimed sum.  The model follows the order of the checks in include/gkr_amd.h:

  * shape first: a length of 0 or 3 is (SHAPE, its row) whatever else the transcript holds;
  * the modulus r in a used slot or a challenge is (NON_CANONICAL, its row); an unused slot is never read: any value is accepted;
  * x + 1 in a used slot of row j changes g_j(0) + g_j(1) by 1 or 2: (ROUND_SUM, j) -- except in row 0 when no claim is given,
    where nothing is compared with that sum and the first relation to notice is the challenge: (CHALLENGE, 0);
  * r_j + 1 is (CHALLENGE, j): round j's sum was checked before, against values that did not change;
  * a length 2 -> 1 drops a non-zero leading coefficient (the prover's length rule): as a used coefficient of that row;
    1 -> 2 adopts the unused slot, which the prover left zero: the same polynomial, another hash: (CHALLENGE, j);
  * the claim + 1 is (ROUND_SUM, 0);
  * a table entry + 1 moves T(r) by eq(r, i), non-zero for challenges that are hash outputs: (EVALUATION, n).
"""

from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from gkr_amd.field import MODULUS as P, from_limbs, to_limbs
from verify_sweeps import R_LIMBS, limbs, value

OK, SHAPE, NON_CANONICAL, ROUND_SUM, CHALLENGE, EVALUATION = 0, 1, 2, 4, 5, 10
ACCEPTED = (True, 0, 0)


class Case(NamedTuple):
    what: str                        # "slot", "r", "len", "claim", "table", "honest"
    index: Tuple[int, ...]
    new: object                      # limbs for field elements, an int for a length, None for honest
    verdict: Tuple[bool, int, int]   # (accept, failed_round, failed_check)


def arrays_of(proof: List[List[int]], r: List[int]):
    """(C, L, R) of a transcript given as the reference gives it: round vectors highest degree first, challenges."""
    n = len(proof)
    C = np.zeros((n, 2, 4), dtype=np.uint64)
    L = np.zeros(n, dtype=np.uint32)
    for j, g in enumerate(proof):
        L[j] = len(g)
        C[j, 2 - len(g):] = to_limbs(g)
    return C, L, to_limbs(r)


def eq_weight(point: List[int], index: int) -> int:
    v = 1
    for i, x in enumerate(point):
        v = v * (x if (index >> (len(point) - 1 - i)) & 1 else 1 - x) % P
    return v


def cases(C, L, R, with_claim: bool, table_positions=None) -> List[Case]:
    """Every tampering of the issue's list for one transcript, and one honest copy in front and at the end."""
    n = L.shape[0]
    first_sum = lambda j: (False, j, ROUND_SUM) if (with_claim or j > 0) else (False, 0, CHALLENGE)
    out = [Case("honest", (), None, ACCEPTED)]
    for j in range(n):
        for t in range(2):
            used = t >= 2 - int(L[j])
            x = value(C[j, t])
            if used:
                out.append(Case("slot", (j, t), limbs((x + 1) % P), first_sum(j)))
                out.append(Case("slot", (j, t), R_LIMBS, (False, j, NON_CANONICAL)))
            else:
                assert x == 0, "the prover leaves an unused slot zero"
                out.append(Case("slot", (j, t), limbs(1), ACCEPTED))
                out.append(Case("slot", (j, t), R_LIMBS, ACCEPTED))
                out.append(Case("slot", (j, t), limbs((1 << 256) - 1), ACCEPTED))
    for j in range(n):
        out.append(Case("r", (j,), limbs((value(R[j]) + 1) % P), (False, j, CHALLENGE)))
        out.append(Case("r", (j,), R_LIMBS, (False, j, NON_CANONICAL)))
    for j in range(n):
        for v in range(4):
            old = int(L[j])
            if v in (0, 3):
                verdict = (False, j, SHAPE)
            elif v == old:
                verdict = ACCEPTED
            elif old == 2:
                assert value(C[j, 0]) != 0, "a vector of length 2 has a non-zero leading coefficient"
                verdict = first_sum(j)
            else:
                verdict = (False, j, CHALLENGE)
            out.append(Case("len", (j,), v, verdict))
    if with_claim:
        out.append(Case("claim", (), "plus1", (False, 0, ROUND_SUM)))
    for i in (range(1 << n) if table_positions is None else table_positions):
        out.append(Case("table", (i,), "plus1", (False, n, EVALUATION)))
    out.append(Case("honest", (), None, ACCEPTED))
    return out


def build_batch(table_limbs, C, L, R, claim_limbs: Optional[np.ndarray], sweep: List[Case]):
    """The batch of len(sweep) transcripts and tables, copy e with change e applied.  -> (tables (B, 2^n, 4), C, L, R, claims or None)."""
    B = len(sweep)
    T = np.ascontiguousarray(np.repeat(table_limbs[None], B, axis=0))
    Cb, Lb, Rb = (np.ascontiguousarray(np.repeat(a[None], B, axis=0)) for a in (C, L, R))
    cl = np.ascontiguousarray(np.repeat(claim_limbs[None], B, axis=0)) if claim_limbs is not None else None
    for e, c in enumerate(sweep):
        if c.what == "slot":
            Cb[(e,) + c.index] = c.new
        elif c.what == "r":
            Rb[(e,) + c.index] = c.new
        elif c.what == "len":
            Lb[(e,) + c.index] = c.new
        elif c.what == "claim":
            cl[e] = limbs((value(cl[e]) + 1) % P)
        elif c.what == "table":
            T[(e,) + c.index] = limbs((value(T[(e,) + c.index]) + 1) % P)
    return T, Cb, Lb, Rb, cl


def reference_verdict(table: List[int], C, L, R, claim: Optional[int], multi_hash) -> Tuple[bool, int, int]:
    """The checks of include/gkr_amd.h one after the other on Python integers (multi_hash: gkr_amd.multi_hash)."""
    n = L.shape[0]
    for j in range(n):
        if not 1 <= int(L[j]) <= 2:
            return False, j, SHAPE
    if claim is not None and claim >= P:
        return False, 0, NON_CANONICAL
    rows = []
    for j in range(n):
        g = [value(C[j, t]) for t in range(2 - int(L[j]), 2)]
        if any(x >= P for x in g) or value(R[j]) >= P:
            return False, j, NON_CANONICAL
        rows.append(g)
    rs = [value(x) for x in R]
    running = claim
    for j, g in enumerate(rows):
        g1 = sum(g) % P
        if running is not None and (g[-1] + g1) % P != running:
            return False, j, ROUND_SUM
        if multi_hash(g, 0) != rs[j]:
            return False, j, CHALLENGE
        running = 0
        for c in g:
            running = (running * rs[j] + c) % P
    t = [x % P for x in table]
    for r in rs:
        half = len(t) // 2
        t = [(t[i] + r * (t[i + half] - t[i])) % P for i in range(half)]
    return (True, 0, OK) if running == t[0] else (False, n, EVALUATION)


# tables that do not depend on every variable (test_mle_length_rule_edge_cases'): their transcripts have rows of length 1 --
# all four rows of the constant table, the last of the table of pairs, the first of the two-halves table
LENGTH_RULE_TABLES = [[5] * 16, [i >> 1 for i in range(32)], [3, 4, 7, 1, 3, 4, 7, 1]]


def assert_sweep_reaches_short_rows(sweep: List[Case], L) -> None:
    """The sweep of a transcript with rows of length 1 holds their two kinds of case: the unused slot changed (three values per
    short row, all accepted) and the length 1 -> 2 (CHALLENGE at the row)."""
    short = [j for j in range(L.shape[0]) if int(L[j]) == 1]
    assert short
    unused = [c for c in sweep if c.what == "slot" and c.index[1] == 0 and c.index[0] in short]
    assert len(unused) == 3 * len(short) and all(c.verdict == ACCEPTED for c in unused)
    grown = [c for c in sweep if c.what == "len" and c.new == 2 and c.index[0] in short]
    assert [c.verdict for c in grown] == [(False, j, CHALLENGE) for j in short]


def rounds_of(C, L):
    return [from_limbs(C[j])[2 - int(L[j]):] for j in range(L.shape[0])]
