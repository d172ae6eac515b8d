"""Integer model of the fractional sum (LogUp) argument (include/gkr_amd.h, gkr_fraction_sum*), written from the protocol on
zerocheck_model and oracle.mimc7 and independently of gkr_amd/verifier.py.

  tree     (p_n, q_n) = (N, D);  p_k[i] = p_{k+1}[i] q_{k+1}[i + 2^k] + p_{k+1}[i + 2^k] q_{k+1}[i],  q_k[i] = q_{k+1}[i] q_{k+1}[i + 2^k]
           (k = n-1 .. 0, i < 2^k);  (P, Q) = (p_0[0], q_0[0]);  sum_i N[i] / D[i] = P / Q;  nothing is inverted
  head     p_2[0..3], q_2[0..3];  zeta_1 = multi_hash(those 8, 0), zeta_2 = multi_hash([zeta_1], 0), z^(2) = (zeta_1, zeta_2),
           lambda_2 = multi_hash([zeta_2], 0), cp_2 = p_2~(z^(2)), cq_2 = q_2~(z^(2))
  layer k  = 2 .. n-1: the zero-check at z^(k) of T0 T3 + T1 T2 + lambda_k T2 T3 over T0, T1 = the halves of p_{k+1}, T2, T3 = the
           halves of q_{k+1} -- its claimed sum is cp_k + lambda_k cq_k -- gives k round vectors, r^(k), (a0, a1, b0, b1) and
           eq(z^(k), r^(k));  tau_k = multi_hash([a0, a1, b0, b1], 0), cp_{k+1} = a0 + tau_k (a1 - a0), cq_{k+1} = b0 + tau_k (b1 - b0),
           z^(k+1) = (tau_k, r^(k)_1 .. r^(k)_k), lambda_{k+1} = multi_hash([tau_k], 0)
  end      cp_n = N~(z^(n)), cq_n = D~(z^(n))

Variable 1 is the most significant index bit everywhere.  The verifier here (model_verdict) states the order of the checks of
the header once more, on the model's own arithmetic."""

import numpy as np

from oracle.field import P
from oracle.mimc7 import multi_hash
from zerocheck_model import zerocheck_sumcheck, zerocheck_sumcheck_np

SHAPE, NON_CANONICAL, ROUND_SUM, CHALLENGE, FINAL_CLAIM, EVALUATION, ZERO_DENOMINATOR, FRACTION_SUM = 1, 2, 4, 5, 6, 10, 14, 15


def layer_terms(lam):
    """T0 T3 + T1 T2 + lambda T2 T3."""
    return [(1, (0, 3)), (1, (1, 2)), (lam, (2, 3))]


def rounds(n):
    return n * (n - 1) // 2 - 1


def layer_row(k):
    return k * (k - 1) // 2 - 1


def fraction_tree(num, den, n):
    """[(p_0, q_0), .., (p_n, q_n)] of two tables of 2^n integers."""
    assert len(num) == 1 << n == len(den)
    levels = [([x % P for x in num], [x % P for x in den])]
    for k in range(n - 1, -1, -1):
        p, q = levels[0]
        h = 1 << k
        levels.insert(0, ([(p[i] * q[i + h] + p[i + h] * q[i]) % P for i in range(h)], [q[i] * q[i + h] % P for i in range(h)]))
    return levels


def fraction_tree_np(num, den, n):
    """The same on numpy object arrays of Python integers."""
    levels = [(num % P, den % P)]
    for k in range(n - 1, -1, -1):
        p, q = levels[0]
        h = 1 << k
        levels.insert(0, ((p[:h] * q[h:] + p[h:] * q[:h]) % P, q[:h] * q[h:] % P))
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


def head_root(head):
    """(P, Q) of p_2[0..3], q_2[0..3] by the tree rule."""
    levels = fraction_tree(head[:4], head[4:], 2)
    return levels[0][0][0], levels[0][1][0]


def head_chain(head):
    """-> (z^(2), lambda_2, cp_2, cq_2)."""
    z = [multi_hash(list(head), 0)]
    z.append(multi_hash([z[0]], 0))
    return z, multi_hash([z[1]], 0), mle(head[:4], z), mle(head[4:], z)


def next_chain(vals, r):
    """(a0, a1, b0, b1), r^(k) -> (z^(k+1), lambda_{k+1}, cp_{k+1}, cq_{k+1})."""
    a0, a1, b0, b1 = vals
    tau = multi_hash([a0, a1, b0, b1], 0)
    return [tau] + list(r), multi_hash([tau], 0), (a0 + tau * (a1 - a0)) % P, (b0 + tau * (b1 - b0)) % P


def fraction_sum(num, den, n, use_np=False):
    """-> dict: sums (P, Q), head, layers [(proof, r, (a0, a1, b0, b1))] for k = 2 .. n-1, and what the chain passes through: points
    [z^(2) .. z^(n)], lambdas [lambda_2 .. lambda_n], claims [(cp_2, cq_2) .. (cp_n, cq_n)], eqs [eq(z^(k), r^(k))], levels."""
    assert n >= 3
    levels = fraction_tree_np(num, den, n) if use_np else fraction_tree(num, den, n)
    head = [int(x) for x in levels[2][0]] + [int(x) for x in levels[2][1]]
    z, lam, cp, cq = head_chain(head)
    out = {"sums": (int(levels[0][0][0]), int(levels[0][1][0])), "head": head, "layers": [], "points": [list(z)], "lambdas": [lam],
           "claims": [(cp, cq)], "eqs": [], "levels": levels}
    for k in range(2, n):
        (p, q), h = levels[k + 1], 1 << k
        if use_np:
            proof, r, evals, eq_r = zerocheck_sumcheck_np(np.stack([p[:h], p[h:], q[:h], q[h:]]), layer_terms(lam), z, k)
        else:
            proof, r, evals, eq_r = zerocheck_sumcheck([p[:h], p[h:], q[:h], q[h:]], layer_terms(lam), z, k)
        z, lam, cp, cq = next_chain(evals, r)
        out["layers"].append((proof, list(r), tuple(evals)))
        out["eqs"].append(eq_r)
        out["points"].append(list(z))
        out["lambdas"].append(lam)
        out["claims"].append((cp, cq))
    out["point"], out["claim"] = out["points"][-1], out["claims"][-1]
    return out


def model_verdict(head, layers, num=None, den=None, sums=None):
    """(check, layer, round) of the first failure in the header's order, (0, 0, 0) for an accepted proof.  Elements are taken as
    they are."""
    n = len(layers) + 2
    for k, (proof, _, _) in enumerate(layers, start=2):
        for j, g in enumerate(proof):
            if not 1 <= len(g) <= 4:
                return SHAPE, k, j
    if any(not 0 <= h < P for h in head) or (sums is not None and any(not 0 <= s < P for s in sums)):
        return NON_CANONICAL, 0, 0
    for k, (proof, r, vals) in enumerate(layers, start=2):
        for j in range(k):
            if any(not 0 <= c < P for c in proof[j]) or not 0 <= r[j] < P:
                return NON_CANONICAL, k, j
        if any(not 0 <= e < P for e in vals):
            return NON_CANONICAL, k, k
    root = head_root(head)
    if root[1] == 0:
        return ZERO_DENOMINATOR, 0, 0
    if sums is not None and (sums[0], sums[1]) != root:
        return FRACTION_SUM, 0, 0
    z, lam, cp, cq = head_chain(head)
    for k, (proof, r, vals) in enumerate(layers, start=2):
        claim = (cp + lam * cq) % P
        for j, g in enumerate(proof):
            at0, at1 = g[-1], sum(g) % P
            if (at0 + at1) % P != claim:
                return ROUND_SUM, k, j
            if multi_hash(g, 0) != r[j]:
                return CHALLENGE, k, j
            claim = 0
            for c in g:
                claim = (claim * r[j] + c) % P
        a0, a1, b0, b1 = vals
        if claim != eq_point(z, r) * (a0 * b1 + a1 * b0 + lam * b0 * b1) % P:
            return FINAL_CLAIM, k, k
        z, lam, cp, cq = next_chain(vals, r)
    if num is not None and (cp != mle(num, z) or cq != mle(den, z)):
        return EVALUATION, n, n
    return 0, 0, 0


# ---- the pairs the tests run

KINDS = ["random", "lookup", "zero_numerators", "one_zero_denominator", "all_max"]


def make_tables(kind, n, rng):
    """-> (N, D).  random: every entry of both non-zero.  lookup: a real LogUp instance -- a table t of 2^(n-1) distinct values,
    2^(n-1) witness values w drawn from it, m their multiplicities: N = 1, D = alpha - w_i on the first half, N = -m_j,
    D = alpha - t_j on the second: the sum is zero, no denominator is."""
    size = 1 << n
    num = [rng.randrange(1, P) for _ in range(size)]
    den = [rng.randrange(1, P) for _ in range(size)]
    if kind == "lookup":
        half = size // 2
        t = []
        while len(t) < half:
            v = rng.randrange(P)
            if v not in t:
                t.append(v)
        picks = [rng.randrange(half) for _ in range(half)]
        alpha = rng.randrange(P)
        while alpha in t:
            alpha = rng.randrange(P)
        num = [1] * half + [(-picks.count(j)) % P for j in range(half)]
        den = [(alpha - t[i]) % P for i in picks] + [(alpha - v) % P for v in t]
    elif kind == "zero_numerators":
        num = [0] * size
    elif kind == "one_zero_denominator":
        den[rng.randrange(size)] = 0
    elif kind == "all_max":
        num, den = [P - 1] * size, [P - 1] * size
    else:
        assert kind == "random", kind
    return num, den


# ---- the proof as the ABI's arrays (Python integers; tests turn them into limbs)


def proof_arrays(g, n):
    """-> (head [8], coeffs [R][4] right-aligned, lens [R], r [R], evals [n - 2][4]) of fraction_sum's result."""
    C, L, R, E = [], [], [], []
    for proof, r, vals in g["layers"]:
        for vec, rj in zip(proof, r):
            C.append([0] * (4 - len(vec)) + list(vec))
            L.append(len(vec))
            R.append(rj)
        E.append(list(vals))
    assert len(C) == rounds(n)
    return list(g["head"]), C, L, R, E
