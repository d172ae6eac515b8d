"""Generators shared by the product-sumcheck verifier's sweeps (test_product_verify_host.py on the CPU,
test_gpu_product_verify.py on the device), after mle_verify_sweeps.py: every single-element change of a transcript of
gkr_sumcheck_product* and of its tables, and the closed-form model of the verdict gkr_sumcheck_product_verify_batch_device
gives it.

A transcript of degree D is (C, L, R): n rows of D + 1 right-aligned slots (highest degree first), n lengths in 1 .. D + 1, n
challenges (uint64 limbs), with its D tables of 2^n entries and, optionally, the claimed sum.  The model follows the order of
the checks in include/gkr_amd.h:

  * shape first: a length of 0 or D + 2 is (SHAPE, its row) whatever else the transcript holds;
  * the modulus r in a used slot or a challenge is (NON_CANONICAL, its row); an unused slot is never read: any value is accepted;
  * x + 1 in a used slot of row j changes g_j(0) + g_j(1) = 2 c_0 + c_1 + .. + c_D by 1 or 2: (ROUND_SUM, j) -- except in row 0
    when no claim is given, where nothing is compared with that sum and the first relation to notice is the challenge:
    (CHALLENGE, 0);
  * r_j + 1 is (CHALLENGE, j): round j's sum was checked before, against values that did not change;
  * a longer length adopts slots the prover left zero: the same polynomial, another hash: (CHALLENGE, j);
  * a shorter length drops the leading coefficients; with s their sum, g_j(0) + g_j(1) moves by -s: s != 0 is a change of a
    used slot of that row, s == 0 leaves the sum and changes the hash: (CHALLENGE, j).  s is computed from the transcript;
  * the claim + 1 is (ROUND_SUM, 0);
  * entry i of factor f + 1 moves prod_g T_g(r) by eq(r, i) prod_{g != f} T_g(r): (EVALUATION, n) iff that product of the
    OTHER factors' values is non-zero (eq(r, i) != 0 for challenges that are hash outputs; the tests assert it), accepted
    otherwise -- the library's zero-factor transcripts: a change of a non-zero factor is invisible behind the zero one.
"""

from typing import List, NamedTuple, Optional, Tuple

import numpy as np

from gkr_amd.field import MODULUS as P, from_limbs, to_limbs
from mle_verify_sweeps import ACCEPTED, CHALLENGE, EVALUATION, NON_CANONICAL, OK, ROUND_SUM, SHAPE, eq_weight
from verify_sweeps import R_LIMBS, limbs, value


class Case(NamedTuple):
    what: str                        # "slot", "r", "len", "claim", "table", "honest"
    index: Tuple[int, ...]           # (row, slot), (row,), (), (factor, entry)
    new: object                      # limbs for field elements, an int for a length, None for honest
    verdict: Tuple[bool, int, int]   # (accept, failed_round, failed_check)
    dropped: Optional[int] = None    # a shortened row: the sum s of the coefficients it drops


def arrays_of(proof: List[List[int]], r: List[int], degree: int):
    """(C, L, R) of a transcript given as the reference gives it: round vectors highest degree first, challenges."""
    n, W = len(proof), degree + 1
    C = np.zeros((n, W, 4), dtype=np.uint64)
    L = np.zeros(n, dtype=np.uint32)
    for j, g in enumerate(proof):
        assert 1 <= len(g) <= W
        L[j] = len(g)
        C[j, W - len(g):] = to_limbs(g)
    return C, L, to_limbs(r)


def rounds_of(C, L):
    W = C.shape[1]
    return [from_limbs(C[j])[W - int(L[j]):] for j in range(L.shape[0])]


def cases(C, L, R, evals: List[int], with_claim: bool, table_positions=None) -> List[Case]:
    """Every tampering of the list above for one transcript of degree C.shape[1] - 1 whose factors have the values `evals` at
    the challenges, and one honest copy in front and at the end.  table_positions: the entries changed in every factor (all)."""
    n, W = L.shape[0], C.shape[1]
    degree = W - 1
    assert len(evals) == degree
    first_sum = lambda j: (False, j, ROUND_SUM) if (with_claim or j > 0) else (False, 0, CHALLENGE)
    out = [Case("honest", (), None, ACCEPTED)]
    for j in range(n):
        for t in range(W):
            used = t >= W - int(L[j])
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
        old = int(L[j])
        for v in range(W + 2):
            if v < 1 or v > W:
                out.append(Case("len", (j,), v, (False, j, SHAPE)))
            elif v == old:
                out.append(Case("len", (j,), v, ACCEPTED))
            elif v > old:
                out.append(Case("len", (j,), v, (False, j, CHALLENGE)))
            else:
                s = sum(value(C[j, t]) for t in range(W - old, W - v)) % P
                out.append(Case("len", (j,), v, first_sum(j) if s else (False, j, CHALLENGE), dropped=s))
    if with_claim:
        out.append(Case("claim", (), "plus1", (False, 0, ROUND_SUM)))
    for f in range(degree):
        others = 1
        for g in range(degree):
            if g != f:
                others = others * evals[g] % P
        for i in (range(1 << n) if table_positions is None else table_positions):
            out.append(Case("table", (f, i), "plus1", (False, n, EVALUATION) if others else ACCEPTED))
    out.append(Case("honest", (), None, ACCEPTED))
    return out


def build_batch(tables_limbs, C, L, R, claim_limbs: Optional[np.ndarray], sweep: List[Case]):
    """The batch of len(sweep) transcripts and table groups, copy e with change e applied.
    tables_limbs: (degree, 2^n, 4).  -> (tables (B, degree, 2^n, 4), C, L, R, claims or None)."""
    B = len(sweep)
    T = np.ascontiguousarray(np.repeat(tables_limbs[None], B, axis=0))
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


def reference_verdict(tables: List[List[int]], C, L, R, claim: Optional[int], multi_hash) -> Tuple[bool, int, int]:
    """The four checks of include/gkr_amd.h one after the other on Python integers (multi_hash: gkr_amd.multi_hash)."""
    n, W = L.shape[0], C.shape[1]
    assert len(tables) == W - 1
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
    prod = 1                                                             # 4. the tables
    for table in tables:
        t = [x % P for x in table]
        for r in rs:
            half = len(t) // 2
            t = [(t[i] + r * (t[i + half] - t[i])) % P for i in range(half)]
        prod = prod * t[0] % P
    return (True, 0, OK) if running == prod else (False, n, EVALUATION)


def assert_sweep_is_sharp(sweep: List[Case], evals: List[int]) -> None:
    """A condition on the test's inputs, not a measurement: a transcript without a zero factor has non-zero values at its
    challenges, so every table change is seen (EVALUATION), and no shortened row drops coefficients that sum to zero (the
    verdict is then the used-slot one, not the weaker CHALLENGE).  Seeds are chosen for which this holds."""
    assert all(e != 0 for e in evals), "a factor vanishes at the challenges"
    tables = [c for c in sweep if c.what == "table"]
    assert tables and all(c.verdict[2] == EVALUATION for c in tables)
    assert all(c.dropped != 0 for c in sweep if c.what == "len" and c.dropped is not None)


def assert_sweep_reaches_short_rows(sweep: List[Case], L, degree: int) -> None:
    """The sweep of a transcript with rows shorter than degree + 1 holds their kinds of case: every unused slot changed (three
    values each, all accepted) and every longer length (CHALLENGE at the row)."""
    W = degree + 1
    short = [j for j in range(L.shape[0]) if int(L[j]) < W]
    assert short
    unused = [c for c in sweep if c.what == "slot" and c.index[0] in short and c.index[1] < W - int(L[c.index[0]])]
    assert len(unused) == 3 * sum(W - int(L[j]) for j in short) and all(c.verdict == ACCEPTED for c in unused)
    grown = [c for c in sweep if c.what == "len" and c.index[0] in short and int(L[c.index[0]]) < c.new <= W]
    assert len(grown) == sum(W - int(L[j]) for j in short)
    assert all(c.verdict == (False, c.index[0], CHALLENGE) for c in grown)


def point_sees(R, positions) -> bool:
    """eq(r, i) != 0 at every position: a change of entry i moves the table's value at r."""
    r = from_limbs(R)
    return all(eq_weight(r, i) != 0 for i in positions)
