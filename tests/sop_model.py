"""Dense integer model of the sumcheck over a sum of products of multilinear tables (include/gkr_amd.h, gkr_sumcheck_sop*), and
the term-list side it is held against.

  g(x) = sum_k c_k prod_j T_t(k,j)(x),   terms = [(c_k, (t(k,0), ..)), ..],   D = the largest term degree

The transcript is the reference's prove_sumcheck(g, n) (rust/src/gkr/sumcheck.rs:158-214; oracle/termlist.py restates it) on
g = add_poly over k of c_k mult_poly(get_multi_ext(T_t(k,0)), ..).  On the tables themselves:

  round j:  the sum over k of c_k times term k's round polynomial of the current tables (product_model.round_coefficients),
            right-aligned in D + 1 slots;
  EVERY round (the last included): leading zero coefficients dropped, one kept at least;
  r_j = multi_hash(round vector, 0);  every table folds ONCE:  T_m[i] += r_j (T_m[i+h] - T_m[i]);
  evals[m] = the one entry table m has left.

g identically zero (the empty term list; the reference panics): every round vector [0] -- what the value rule gives by itself.
"""

import numpy as np

from oracle.field import P
from oracle.mimc7 import multi_hash
from product_model import product_term_list, round_coefficients

# the structures the tests share: (name, number of tables, terms)
STRUCTURES = [
    ("AB-C", 3, [(1, (0, 1)), (P - 1, (2,))]),
    ("ABC-AD", 4, [(1, (0, 1, 2)), (P - 1, (0, 3))]),
    ("5AB+7BC+11A", 3, [(5, (0, 1)), (7, (1, 2)), (11, (0,))]),
    ("AA+3B", 2, [(1, (0, 0)), (3, (1,))]),
    ("AB-AB", 2, [(1, (0, 1)), (P - 1, (0, 1))]),
    ("AB-AC", 3, [(1, (0, 1)), (P - 1, (0, 2))]),
]


def sop_degree(terms):
    return max(len(idx) for _, idx in terms)


def sop_round_coefficients(tables, terms):
    """c_D .. c_0 (highest degree first, all D + 1 of them) of the current tables' round polynomial."""
    D = sop_degree(terms)
    acc = [0] * (D + 1)
    for c, idx in terms:
        tc = round_coefficients([tables[i] for i in idx])
        for k, v in enumerate(tc):
            acc[D - len(idx) + k] = (acc[D - len(idx) + k] + c * v) % P
    return acc


def sop_sumcheck(tables, terms, n):
    """-> (proof, r, evals): proof[j] the round vector (used slots, highest degree first), r the challenges, evals[m] the single
    entry table m has left after the last fold (= its multilinear extension at r)."""
    cur = [[x % P for x in t] for t in tables]
    assert all(len(t) == 1 << n for t in cur)
    proof, r = [], []
    for _ in range(n):
        c = sop_round_coefficients(cur, terms)
        while len(c) > 1 and c[0] == 0:
            c = c[1:]
        proof.append(c)
        r.append(multi_hash(c, 0))
        h = len(cur[0]) // 2
        cur = [[(t[i] + r[-1] * (t[i + h] - t[i])) % P for i in range(h)] for t in cur]
    return proof, r, [t[0] for t in cur]


def sop_claim(tables, terms):
    """sum_x g(x), summed entry by entry (independent of the round polynomials)."""
    total = 0
    for i in range(len(tables[0])):
        for c, idx in terms:
            v = c
            for m in idx:
                v = v * tables[m][i] % P
            total += v
    return total % P


def sop_eval(evals, terms):
    """g at a point, from the tables' values there."""
    total = 0
    for c, idx in terms:
        v = c
        for m in idx:
            v = v * evals[m] % P
        total += v
    return total % P


def constant_tables_transcript(values, terms, n):
    """sop_sumcheck of CONSTANT tables (table m is values[m] everywhere) without the tables: round j's vector is
    [2^(n-1-j) g(values)] and evals = values."""
    g = sop_eval(values, terms)
    proof = [[(1 << (n - 1 - j)) * g % P] for j in range(n)]
    return proof, [multi_hash(v, 0) for v in proof], [v % P for v in values]


# ---- the term-list side (tests only)


def sop_term_list(tables, terms, n):
    """add_poly over k of c_k * mult_poly(the extensions of term k's tables); [] when g is identically zero."""
    from oracle.termlist import add_poly
    g = []
    for c, idx in terms:
        scaled = [[t[0] * c % P] + list(t[1:]) for t in product_term_list([tables[i] for i in idx], n)]
        g = add_poly(g, [t for t in scaled if t[0]])
    return g


# ---- the same model on numpy object arrays (Python integers, vectorised): the multi-block shapes of the GPU tests


def limbs_to_object(a):
    """(.., 4) uint64 limbs -> an object array of Python integers of the leading shape."""
    buf = np.ascontiguousarray(a, dtype="<u8").tobytes()
    out = np.empty(len(buf) // 32, dtype=object)
    out[:] = [int.from_bytes(buf[i:i + 32], "little") for i in range(0, len(buf), 32)]
    return out.reshape(a.shape[:-1])


def sop_claim_np(tables, terms):
    """sop_claim on an (M, 2^n) object array."""
    total = 0
    for c, idx in terms:
        v = tables[idx[0]]
        for m in idx[1:]:
            v = v * tables[m]                                     # (unreduced: one reduction at the end)
        total += c * int(v.sum())
    return total % P


def sop_sumcheck_np(tables, terms, n):
    """sop_sumcheck on an (M, 2^n) object array: the same coefficients (the per-index polynomials multiplied out slot by slot,
    then summed), the same length rule, the same folds."""
    cur = tables % P
    D = sop_degree(terms)
    proof, r = [], []
    for _ in range(n):
        h = cur.shape[1] // 2
        lo, diff = cur[:, :h], cur[:, h:] - cur[:, :h]
        acc = [0] * (D + 1)                                       # highest degree first
        for c, idx in terms:
            poly = [1]                                            # lowest degree first, arrays over the index
            for m in idx:
                nxt = [0] * (len(poly) + 1)
                for k, p in enumerate(poly):
                    nxt[k] = nxt[k] + p * lo[m]
                    nxt[k + 1] = nxt[k + 1] + p * diff[m]
                poly = [x % P for x in nxt]
            for k, p in enumerate(poly):
                acc[D - k] = (acc[D - k] + c * int(p.sum())) % P
        while len(acc) > 1 and acc[0] == 0:
            acc = acc[1:]
        proof.append(acc)
        r.append(multi_hash(acc, 0))
        cur = (lo + r[-1] * diff) % P
    return proof, r, [int(x) for x in cur[:, 0]]
