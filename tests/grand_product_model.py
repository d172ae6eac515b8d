"""Integer model of the grand product argument (include/gkr_amd.h, gkr_grand_product*), written from the protocol on
zerocheck_model and oracle.mimc7 and independently of gkr_amd/verifier.py.

  tree     L_n = V;  L_k[i] = L_{k+1}[i] L_{k+1}[i + 2^k] mod r  (k = n-1 .. 0, i < 2^k);  P = L_0[0]
  head     L_2 and P;  zeta_1 = multi_hash(L_2, 0), zeta_2 = multi_hash([zeta_1], 0), z^(2) = (zeta_1, zeta_2), c_2 = L_2~(z^(2))
  layer k  = 2 .. n-1: the zero-check of eq(z^(k), .) L_{k+1}[0 .. 2^k) L_{k+1}[2^k ..) -- its claimed sum is c_k -- gives k round
           vectors, r^(k), (a_k, b_k) and eq(z^(k), r^(k));  tau_k = multi_hash([a_k, b_k], 0), c_{k+1} = a_k + tau_k (b_k - a_k),
           z^(k+1) = (tau_k, r^(k)_1 .. r^(k)_k)
  end      c_n = V~(z^(n))

Variable 1 is the most significant index bit everywhere.  The verifier here (model_verdict) states the order of the checks of
the header once more, on the model's own arithmetic."""

import numpy as np

from oracle.field import P
from oracle.mimc7 import multi_hash
from zerocheck_model import zerocheck_sumcheck, zerocheck_sumcheck_np

TERMS = [(1, (0, 1))]                                              # one term, L_{k+1}[0 ..) * L_{k+1}[2^k ..), coefficient 1
SHAPE, NON_CANONICAL, ROUND_SUM, CHALLENGE, FINAL_CLAIM, EVALUATION, PRODUCT = 1, 2, 4, 5, 6, 10, 13


def rounds(n):
    return n * (n - 1) // 2 - 1


def layer_row(k):
    return k * (k - 1) // 2 - 1


def product_tree(table, n):
    """[L_0, L_1, .., L_n] of a table of 2^n integers."""
    assert len(table) == 1 << n
    levels = [[x % P for x in table]]
    for k in range(n - 1, -1, -1):
        up = levels[0]
        levels.insert(0, [up[i] * up[i + (1 << k)] % P for i in range(1 << k)])
    return levels


def product_tree_np(table, n):
    """The same on a numpy object array of Python integers."""
    levels = [table % P]
    for k in range(n - 1, -1, -1):
        up = levels[0]
        levels.insert(0, up[:1 << k] * up[1 << k:] % P)
    return levels


def mle(table, point):
    t = [x % P for x in table]
    for r in point:
        h = len(t) // 2
        t = [(t[i] + r * (t[i + h] - t[i])) % P for i in range(h)]
    return t[0]


def mle_np(table, point):
    t = table % P
    for r in point:
        h = len(t) // 2
        t = (t[:h] + r * (t[h:] - t[:h])) % P
    return int(t[0])


def eq_point(z, r):
    v = 1
    for zj, rj in zip(z, r):
        v = v * (zj * rj + (1 - zj) * (1 - rj)) % P
    return v


def grand_product(table, n, use_np=False):
    """-> dict: product, head, layers [(proof, r, (a_k, b_k))] for k = 2 .. n-1, and what the chain passes through: points
    [z^(2) .. z^(n)], claims [c_2 .. c_n], eqs [eq(z^(k), r^(k))], levels."""
    assert n >= 3
    levels = product_tree_np(table, n) if use_np else product_tree(table, n)
    head = [int(x) for x in levels[2]]
    z = [multi_hash(head, 0)]
    z.append(multi_hash([z[0]], 0))
    out = {"product": int(levels[0][0]), "head": head, "layers": [], "points": [list(z)], "claims": [mle(head, z)], "eqs": [], "levels": levels}
    for k in range(2, n):
        up, h = levels[k + 1], 1 << k
        if use_np:
            proof, r, evals, eq_r = zerocheck_sumcheck_np(np.stack([up[:h], up[h:]]), TERMS, z, k)
        else:
            proof, r, evals, eq_r = zerocheck_sumcheck([up[:h], up[h:]], TERMS, z, k)
        a, b = evals
        tau = multi_hash([a, b], 0)
        z = [tau] + list(r)
        out["layers"].append((proof, list(r), (a, b)))
        out["eqs"].append(eq_r)
        out["points"].append(list(z))
        out["claims"].append((a + tau * (b - a)) % P)
    out["point"], out["claim"] = out["points"][-1], out["claims"][-1]
    return out


def model_verdict(head, layers, table=None, product=None):
    """(check, layer, round) of the first failure in the header's order, (0, 0, 0) for an accepted proof.  Elements are taken as
    they are."""
    n = len(layers) + 2
    for k, (proof, _, _) in enumerate(layers, start=2):
        for j, g in enumerate(proof):
            if not 1 <= len(g) <= 4:
                return SHAPE, k, j
    if any(not 0 <= h < P for h in head) or (product is not None and not 0 <= product < P):
        return NON_CANONICAL, 0, 0
    for k, (proof, r, ab) in enumerate(layers, start=2):
        for j in range(k):
            if any(not 0 <= c < P for c in proof[j]) or not 0 <= r[j] < P:
                return NON_CANONICAL, k, j
        if any(not 0 <= e < P for e in ab):
            return NON_CANONICAL, k, k
    if product is not None and product != head[0] * head[1] * head[2] * head[3] % P:
        return PRODUCT, 0, 0
    z = [multi_hash(head, 0)]
    z.append(multi_hash([z[0]], 0))
    claim = mle(head, z)
    for k, (proof, r, (a, b)) in enumerate(layers, start=2):
        for j, g in enumerate(proof):
            at0, at1 = g[-1], sum(g) % P
            if (at0 + at1) % P != claim:
                return ROUND_SUM, k, j
            if multi_hash(g, 0) != r[j]:
                return CHALLENGE, k, j
            claim = 0
            for c in g:
                claim = (claim * r[j] + c) % P
        if claim != eq_point(z, r) * a * b % P:
            return FINAL_CLAIM, k, k
        tau = multi_hash([a, b], 0)
        claim, z = (a + tau * (b - a)) % P, [tau] + list(r)
    if table is not None and claim != mle(table, z):
        return EVALUATION, n, n
    return 0, 0, 0


# ---- the tables the tests run: random, all ones, one zero entry, the whole upper half zero, every entry r - 1

KINDS = ["random", "ones", "one_zero", "upper_zero", "all_max"]


def make_table(kind, n, rng):
    size = 1 << n
    t = [rng.randrange(1, P) for _ in range(size)]
    if kind == "ones":
        t = [1] * size
    elif kind == "one_zero":
        t[rng.randrange(size)] = 0
    elif kind == "upper_zero":
        t[size // 2:] = [0] * (size // 2)
    elif kind == "all_max":
        t = [P - 1] * size
    else:
        assert kind == "random", kind
    return t


# ---- the proof as the ABI's arrays (Python integers; tests turn them into limbs)


def proof_arrays(g, n):
    """-> (head [4], coeffs [R][4] right-aligned, lens [R], r [R], evals [n - 2][2]) of grand_product's result."""
    C, L, R, E = [], [], [], []
    for proof, r, ab in g["layers"]:
        for vec, rj in zip(proof, r):
            C.append([0] * (4 - len(vec)) + list(vec))
            L.append(len(vec))
            R.append(rj)
        E.append(list(ab))
    assert len(C) == rounds(n)
    return list(g["head"]), C, L, R, E
