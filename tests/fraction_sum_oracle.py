"""What tests/test_oracle_fraction_sum_c.py, tests/test_oracle_lookup_c.py and the two *_sizes.py GPU files share: the C oracle's
fractional sum proof (cdense.fraction_sum_raw, ogkr_fraction_sum) as the dict tests/fraction_sum_model.fraction_sum returns -- so
that fraction_sum_sweeps.tamperings works out its closed-form verdicts from a proof no Python integer model could make at that
size -- and pairs built as limb arrays without a Python integer per entry.

The chain of points, lambdas and claims is formed HERE once more, from the oracle's head, challenges and values, with oracle.mimc7
(the Python hash, not the C one) and the closed form of eq; the oracle's own point and claims must agree."""

import numpy as np

from fraction_sum_model import KINDS, eq_point, head_chain, layer_row, next_chain, rounds
from oracle import cdense
from oracle.field import P

PAIR_KINDS = KINDS + ["padded", "upper_zero"]
MAX_LIMBS = cdense.to_limbs([P - 1])[0]


def zero_index(n):
    """Where the "one_zero_denominator" pair has its zero in D: in the LAST block of 256 of the upper half (and not at that block's
    edge)."""
    return (1 << n) - 256 + 77 if n >= 9 else (1 << n) - 2


def lookup_instance(n_w, n_t, seed):
    """(W, T, M, alpha) limbs of a lookup that holds: T cdense.fill_table's values (distinct in practice; asserted by the callers
    that need it), W drawn uniformly from it, M the oracle's own count, alpha one more value of the stream."""
    T = cdense.fill_table((1 << n_t) + 1, seed)
    alpha, T = T[-1].copy(), np.ascontiguousarray(T[:-1])
    W = np.ascontiguousarray(T[np.random.default_rng(seed + 1).integers(0, 1 << n_t, size=1 << n_w)])
    M, missing, first = cdense.lookup_multiplicities_raw(W, T)
    assert (missing, first) == (0, 0xFFFFFFFF)
    return W, T, M, alpha


def limb_pair(kind, n, seed):
    """(2, 2^n, 4) limbs, N then D, of a pair of one of PAIR_KINDS: cdense.fill_table's values (below 2^253, none zero in practice)
    with the structured kinds written over them by numpy; "lookup" (n_w = n_t = n - 1) and "padded" (n_w = n - 5, n_t = n - 1:
    fifteen sixteenths of the witness half is (0, 1)) by the oracle's own lookup functions; "upper_zero" has the upper halves of N
    and of D zero: every level below the pair is zero and every round vector is [0] -- the zero-bearing pair whose vectors are
    short in every layer (the other kinds' vectors are full, all_max apart)."""
    size = 1 << n
    if kind in ("lookup", "padded"):
        W, T, M, alpha = lookup_instance(n - 1 if kind == "lookup" else n - 5, n - 1, seed)
        pair = cdense.lookup_pair_raw(W, T, M, alpha)
        assert pair.shape == (2, size, 4)
        return pair
    pair = cdense.fill_table(2 * size, seed).reshape(2, size, 4)
    if kind == "zero_numerators":
        pair[0] = 0
    elif kind == "one_zero_denominator":
        pair[1, zero_index(n)] = 0
    elif kind == "all_max":
        pair[:] = MAX_LIMBS
    elif kind == "upper_zero":
        pair[:, size // 2:] = 0
    else:
        assert kind == "random", kind
    return pair


def as_model(raw, n):
    """cdense.fraction_sum_raw's (S, H, C, L, R, E, Z, K) -> the dict of fraction_sum_model.fraction_sum (no "levels")."""
    S, H, C, L, R, E, Z, K = raw[:8]
    assert C.shape == (rounds(n), 4, 4) and L.shape == (rounds(n),) and E.shape == (n - 2, 4, 4) and Z.shape == (n, 4) and K.shape == (2, 4)
    head, rs, ev = cdense.from_limbs(H), cdense.from_limbs(R), cdense.from_limbs(E)
    z, lam, cp, cq = head_chain(head)
    g = {"sums": tuple(cdense.from_limbs(S)), "head": head, "layers": [], "points": [list(z)], "lambdas": [lam], "claims": [(cp, cq)], "eqs": []}
    for k in range(2, n):
        row = layer_row(k)
        proof = []
        for j in range(k):
            slots, ln = cdense.from_limbs(C[row + j]), int(L[row + j])
            assert 1 <= ln <= 4 and not any(slots[:4 - ln]), ("unused slots hold zero", k, j)
            proof.append(slots[4 - ln:])
        r, vals = rs[row:row + k], tuple(ev[4 * (k - 2):4 * (k - 2) + 4])
        g["layers"].append((proof, r, vals))
        g["eqs"].append(eq_point(z, r))
        z, lam, cp, cq = next_chain(vals, r)
        g["points"].append(list(z))
        g["lambdas"].append(lam)
        g["claims"].append((cp, cq))
    g["point"], g["claim"] = g["points"][-1], g["claims"][-1]
    assert g["point"] == cdense.from_limbs(Z) and list(g["claim"]) == cdense.from_limbs(K), "the oracle's own point and claims"
    return g


def pick(sweep, *names):
    """The cases of fraction_sum_sweeps.tamperings' list with these names, in the order asked for (a missing name is an error: a
    slot the proof does not use cannot be changed)."""
    by_name = {name: (name, what, want) for name, what, want in sweep}
    return [by_name[name] for name in names]
