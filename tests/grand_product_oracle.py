"""What tests/test_oracle_grand_product_c.py and tests/test_gpu_grand_product_sizes.py share: the C oracle's grand product proof
(cdense.grand_product_raw, ogkr_grand_product) as the dict tests/grand_product_model.grand_product returns -- so that
grand_product_sweeps.tamperings works out its closed-form verdicts from a proof no Python integer model could make at that size
-- and tables built as limb arrays without a Python integer per entry.

The chain of points and claims is formed HERE once more, from the oracle's head, challenges and values, with oracle.mimc7 (the
Python hash, not the C one) and the closed form of eq; the oracle's own point and claim must agree."""

import numpy as np

from grand_product_model import eq_point, layer_row, rounds
from oracle import cdense
from oracle.field import P
from oracle.mimc7 import multi_hash
from product_model import SPECIALS

TABLE_KINDS = ["random", "all_max", "ones", "specials", "one_zero", "upper_zero"]
SPECIAL_LIMBS = cdense.to_limbs([s for s in SPECIALS])
MAX_LIMBS = cdense.to_limbs([P - 1])[0]
ONE_LIMBS = np.array([1, 0, 0, 0], dtype=np.uint64)


def zero_index(n):
    """Where the "one_zero" table has its zero: in the LAST block of 256 of the upper half (and not at that block's edge)."""
    return (1 << n) - 256 + 77 if n >= 9 else (1 << n) - 2


def limb_table(kind, n, seed):
    """(2^n, 4) limbs of a table of one of TABLE_KINDS: cdense.fill_table's values (below 2^253, none zero in practice) with the
    structured kinds written over them by numpy."""
    size = 1 << n
    t = cdense.fill_table(size, seed)
    if kind == "all_max":
        t[:] = MAX_LIMBS
    elif kind == "ones":
        t[:] = ONE_LIMBS
    elif kind == "specials":
        t[:] = SPECIAL_LIMBS[np.random.default_rng(seed + 1).integers(0, len(SPECIAL_LIMBS), size=size)]
    elif kind == "one_zero":
        t[zero_index(n)] = 0
    elif kind == "upper_zero":
        t[size // 2:] = 0
    else:
        assert kind == "random", kind
    return t


def as_model(raw, n):
    """cdense.grand_product_raw's (P, H, C, L, R, E, Z, K) -> the dict of grand_product_model.grand_product (no "levels")."""
    Pl, H, C, L, R, E, Z, K = raw[:8]
    assert C.shape == (rounds(n), 4, 4) and L.shape == (rounds(n),) and E.shape == (n - 2, 2, 4) and Z.shape == (n, 4)
    head, rs, ev = cdense.from_limbs(H), cdense.from_limbs(R), cdense.from_limbs(E)
    z = [multi_hash(head, 0)]
    z.append(multi_hash([z[0]], 0))
    t = list(head)
    for x in z:                                                    # c_2 = L_2~(z^(2))
        h = len(t) // 2
        t = [(t[i] + x * (t[i + h] - t[i])) % P for i in range(h)]
    g = {"product": cdense.from_limbs(Pl)[0], "head": head, "layers": [], "points": [list(z)], "claims": [t[0]], "eqs": []}
    for k in range(2, n):
        row = layer_row(k)
        proof = []
        for j in range(k):
            slots, ln = cdense.from_limbs(C[row + j]), int(L[row + j])
            assert 1 <= ln <= 4 and not any(slots[:4 - ln]), ("unused slots hold zero", k, j)
            proof.append(slots[4 - ln:])
        r, (a, b) = rs[row:row + k], ev[2 * (k - 2):2 * (k - 2) + 2]
        g["layers"].append((proof, r, (a, b)))
        g["eqs"].append(eq_point(z, r))
        tau = multi_hash([a, b], 0)
        z = [tau] + r
        g["points"].append(list(z))
        g["claims"].append((a + tau * (b - a)) % P)
    g["point"], g["claim"] = g["points"][-1], g["claims"][-1]
    assert g["point"] == cdense.from_limbs(Z) and [g["claim"]] == cdense.from_limbs(K), "the oracle's own point and claim"
    return g


def pick(sweep, *names):
    """The cases of grand_product_sweeps.tamperings' list with these names, in the order asked for (a missing name is an error:
    a slot the proof does not use cannot be changed)."""
    by_name = {name: (name, what, want) for name, what, want in sweep}
    return [by_name[name] for name in names]
