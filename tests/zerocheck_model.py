"""Integer model of the zero-check sumcheck (include/gkr_amd.h, gkr_sumcheck_zerocheck*), in the IMPLICIT form the kernels use:
no table eq(z, .) of 2^n entries exists here either.

  sum_x eq(z, x) g(x),   g(x) = sum_k c_k prod_f T_t(k,f)(x),   terms = [(c_k, (t(k,0), ..)), ..] of 1 or 2 indices,
  d = the largest term degree, D = d + 1.

  round j = 1 .. n, on the current tables of 2^(n-j+1) entries (lo_f = T_f[i], hi_f = T_f[i + 2^(n-j)]):
      w_j(i) = eq((z_{j+1} .. z_n), i)                              the suffix weights, 2^(n-j) of them
      h_j(X) = sum_i w_j(i) sum_k c_k prod_f (lo_f + X (hi_f - lo_f))
      s_j    = prod_{l < j} (z_l r_l + (1 - z_l)(1 - r_l))
      g_j(X) = s_j ((1 - z_j) + (2 z_j - 1) X) h_j(X)
  the round vector: g_j's D + 1 coefficients, highest degree first, leading zeros dropped, one kept at least;
  r_j = multi_hash(round vector, 0); every table folds once; evals[m] = the entry table m has left; eq_r = s_{n+1}.

tests/test_zerocheck_host.py holds this against sop_model.sop_sumcheck on [eq_table(z)] + tables with lift_terms(terms)."""

import numpy as np

from oracle.field import P
from oracle.mimc7 import multi_hash


def eq_table(z):
    """eq(z, i) for i < 2^n, variable 1 (z[0]) = the most significant index bit."""
    t = [1]
    for zj in z:
        t = [v * f % P for v in t for f in ((1 - zj) % P, zj % P)]
    return t


def lift_terms(terms):
    """The terms over [eq] + tables: table 0 in front of every term, every index shifted by one."""
    return [(c, (0,) + tuple(i + 1 for i in idx)) for c, idx in terms]


def zc_degree(terms):
    return max(len(idx) for _, idx in terms) + 1


def _inner_coefficients(cur, terms, w):
    """h_j's coefficients, lowest degree first (d + 1 of them), the index's contribution weighted by w[i]."""
    d = zc_degree(terms) - 1
    h = len(cur[0]) // 2
    acc = [0] * (d + 1)
    for c, idx in terms:
        for i in range(h):
            poly = [c * w[i] % P]
            for m in idx:
                lo, diff = cur[m][i], cur[m][i + h] - cur[m][i]
                nxt = [0] * (len(poly) + 1)
                for k, p in enumerate(poly):
                    nxt[k] += p * lo
                    nxt[k + 1] += p * diff
                poly = [x % P for x in nxt]
            for k, p in enumerate(poly):
                acc[k] = (acc[k] + p) % P
    return acc


def _finish_round(hc, s, zj, D):
    """h_j (lowest degree first) -> the round vector of g_j = s ((1 - z_j) + (2 z_j - 1) X) h_j."""
    a, b = s * (1 - zj) % P, s * (2 * zj - 1) % P
    g = [0] * (D + 1)
    for k, v in enumerate(hc):
        g[k] = (g[k] + a * v) % P
        g[k + 1] = (g[k + 1] + b * v) % P
    g = g[::-1]                                                   # highest degree first
    while len(g) > 1 and g[0] == 0:
        g = g[1:]
    return g, a, b


def zerocheck_sumcheck(tables, terms, z, n):
    """-> (proof, r, evals, eq_r)."""
    cur = [[x % P for x in t] for t in tables]
    assert all(len(t) == 1 << n for t in cur) and len(z) == n and all(1 <= len(idx) <= 2 for _, idx in terms)
    z = [x % P for x in z]
    D = zc_degree(terms)
    proof, r, s = [], [], 1
    for j in range(n):
        g, a, b = _finish_round(_inner_coefficients(cur, terms, eq_table(z[j + 1:])), s, z[j], D)
        proof.append(g)
        r.append(multi_hash(g, 0))
        s = (a + b * r[-1]) % P                                   # s_j eq(z_j, r_j)
        h = len(cur[0]) // 2
        cur = [[(t[i] + r[-1] * (t[i + h] - t[i])) % P for i in range(h)] for t in cur]
    return proof, r, [t[0] for t in cur], s


def zerocheck_claim(tables, terms, z):
    """sum_i eq(z, i) g[i], summed entry by entry."""
    e = eq_table(z)
    total = 0
    for i in range(len(e)):
        for c, idx in terms:
            v = c * e[i]
            for m in idx:
                v = v * tables[m][i] % P
            total += v
    return total % P


def zerocheck_eval(evals, terms, eq_r):
    total = 0
    for c, idx in terms:
        v = c
        for m in idx:
            v = v * evals[m] % P
        total += v
    return total * eq_r % P


# ---- the same model on numpy object arrays (Python integers, vectorised): the larger shapes of the GPU tests


def eq_table_np(z):
    t = np.array([1], dtype=object)
    for zj in z:
        t = np.stack([t * ((1 - zj) % P) % P, t * (zj % P) % P], axis=1).reshape(-1)
    return t


def zerocheck_sumcheck_np(tables, terms, z, n):
    """zerocheck_sumcheck on an (M, 2^n) object array."""
    cur = tables % P
    z = [int(x) % P for x in z]
    D = zc_degree(terms)
    proof, r, s = [], [], 1
    for j in range(n):
        h = cur.shape[1] // 2
        lo, diff = cur[:, :h], cur[:, h:] - cur[:, :h]
        w = eq_table_np(z[j + 1:])
        hc = [0] * D
        for c, idx in terms:
            poly = [w]
            for m in idx:
                nxt = [0] * (len(poly) + 1)
                for k, p in enumerate(poly):
                    nxt[k] = nxt[k] + p * lo[m]
                    nxt[k + 1] = nxt[k + 1] + p * diff[m]
                poly = [x % P for x in nxt]
            for k, p in enumerate(poly):
                hc[k] = (hc[k] + c * int(p.sum())) % P
        g, a, b = _finish_round(hc, s, z[j], D)
        proof.append(g)
        r.append(multi_hash(g, 0))
        s = (a + b * r[-1]) % P
        cur = (lo + r[-1] * diff) % P
    return proof, r, [int(x) for x in cur[:, 0]], s


def zerocheck_claim_np(tables, terms, z):
    e = eq_table_np(z)
    total = 0
    for c, idx in terms:
        v = e
        for m in idx:
            v = v * tables[m] % P
        total += c * int(v.sum())
    return total % P
