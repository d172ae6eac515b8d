"""Dense integer model of the sumcheck over a product of multilinear tables (include/gkr_amd.h, gkr_sumcheck_product*), and
the term-list side it is held against.

The transcript is the reference's prove_sumcheck(g, n) (rust/src/gkr/sumcheck.rs:158-214; oracle/termlist.py restates it) on
g = mult_poly(get_multi_ext(T_0), .., get_multi_ext(T_{d-1})) (poly.rs:349-386).  On the tables themselves:

  round j (0-based), h = half the current tables:  sum_{i<h} prod_f (T_f[i] + t (T_f[i+h] - T_f[i]))  =  c_d t^d + .. + c_0
  rounds j < n-1:  leading zero coefficients dropped, one kept at least (add_poly merges by exponent and drops zero sums)
  round n-1:       1 + (factors with T_f[2m] != T_f[2m+1] for some m) coefficients (no merge: the length is structural)
  r_j = multi_hash(round vector, 0);  every factor folds:  T_f[i] += r_j (T_f[i+h] - T_f[i])
  a factor that is the zero table (g the empty term list; the reference panics): every round vector [0] -- the library's choice
"""

from oracle.field import P
from oracle.mimc7 import multi_hash


def round_coefficients(tables):
    """c_d .. c_0 (highest degree first, all d + 1 of them) of the current tables' round polynomial."""
    d, h = len(tables), len(tables[0]) // 2
    acc = [0] * (d + 1)                     # lowest degree first
    for i in range(h):
        poly = [1]
        for t in tables:
            lo = t[i]
            diff = t[i + h] - lo
            nxt = [0] * (len(poly) + 1)
            for k, c in enumerate(poly):
                nxt[k] += c * lo
                nxt[k + 1] += c * diff
            poly = nxt
        for k in range(d + 1):
            acc[k] += poly[k]
    return [a % P for a in reversed(acc)]


def depends_on_last(table):
    return any(table[2 * m] != table[2 * m + 1] for m in range(len(table) // 2))


def product_sumcheck(tables, n):
    """-> (proof, r, evals): proof[j] the round vector (used slots, highest degree first), r the challenges, evals[f] the
    single entry factor f has left after the last fold (= its multilinear extension at r)."""
    cur = [[x % P for x in t] for t in tables]
    d = len(cur)
    assert d >= 1 and all(len(t) == 1 << n for t in cur)
    zero = any(not any(t) for t in cur)
    last_len = 1 if zero else 1 + sum(depends_on_last(t) for t in cur)
    proof, r = [], []
    for j in range(n):
        c = round_coefficients(cur)
        if j < n - 1:
            while len(c) > 1 and c[0] == 0:
                c = c[1:]
        else:
            assert not any(c[:d + 1 - last_len])
            c = c[d + 1 - last_len:]
        proof.append(c)
        r.append(multi_hash(c, 0))
        h = len(cur[0]) // 2
        cur = [[(t[i] + r[-1] * (t[i + h] - t[i])) % P for i in range(h)] for t in cur]
    return proof, r, [t[0] for t in cur]


def constant_tables_transcript(values, n):
    """product_sumcheck of CONSTANT tables (factor f is values[f] everywhere) without the tables: no factor depends on a
    variable, a fold leaves a constant table as it is, so round j's vector is [2^(n-1-j) prod values] and evals = values."""
    prod = 1
    for v in values:
        prod = prod * v % P
    proof = [[(1 << (n - 1 - j)) * prod % P] for j in range(n)]
    return proof, [multi_hash(g, 0) for g in proof], [v % P for v in values]


# ---- the term-list side (tests only): mult_poly, poly.rs:349-386 with mult_mono 336-347, restated on oracle term lists


def mult_poly(f1, f2):
    """Every term of f1 times every term of f2 (coefficients multiplied, exponents added), equal monomials merged, zero
    coefficients dropped.  (The reference iterates a HashMap: term order is unspecified, here first-seen.)"""
    acc = {}
    for t1 in f1:
        for t2 in f2:
            key = tuple(a + b for a, b in zip(t1[1:], t2[1:]))
            acc[key] = (acc.get(key, 0) + t1[0] * t2[0]) % P
    return [[c] + list(k) for k, c in acc.items() if c != 0]


def product_term_list(tables, n):
    from oracle.termlist import get_multi_ext
    g = get_multi_ext(tables[0], n)
    for t in tables[1:]:
        g = mult_poly(g, get_multi_ext(t, n))
    return g


# ---- factor kinds the tests mix (a table of 2^n values each)

SPECIALS = [0, 1, P - 1, P - 2, (1 << 253) - 1, int.from_bytes(b"\x80" * 31 + b"\x20", "little"),
            int.from_bytes(b"\x7f" * 31 + b"\x2f", "little"), int.from_bytes(b"\xff" * 31 + b"\x2f", "little"),
            int.from_bytes(b"\x00\xff" * 15 + b"\x00\x30", "little"), 0x80, 0xff, 1 << 128]   # tests/test_gpu_mle_eval.py's byte patterns
KINDS = ["random", "all_max", "specials", "bits", "constant", "indep_last", "indep_first", "indep_middle"]


def factor(kind, n, rng):
    size = 1 << n
    if kind == "random":
        return [rng.randrange(P) for _ in range(size)]
    if kind == "all_max":
        return [P - 1] * size
    if kind == "specials":
        return [SPECIALS[rng.randrange(len(SPECIALS))] for _ in range(size)]
    if kind == "bits":
        return [rng.randrange(2) for _ in range(size)]
    if kind == "constant":
        return [rng.randrange(1, P)] * size
    if kind == "zero":
        return [0] * size
    var = {"indep_last": n - 1, "indep_first": 0, "indep_middle": n // 2}[kind]      # 0-based variable the table ignores
    bit = 1 << (n - 1 - var)
    base = [rng.randrange(P) for _ in range(size)]
    return [base[i & ~bit] for i in range(size)]
