"""Single-element changes of a grand product proof and the verdict each must get, shared by tests/test_grand_product_host.py (the
integer verifiers) and tests/test_gpu_grand_product.py (the device verifier, honest and tampered proofs in one batch).

A change is (name, what); apply(..) makes the changed proof.  The expected verdict (check, layer, round) is worked out here in
CLOSED FORM from the rules of the header, position by position -- no verifier is run to get it:
  a head entry + 1           with a claimed product: the head's product moves by the product of the other three -- PRODUCT at (0, 0)
                             when that is non-zero.  Otherwise (no claim, or another head entry is zero) zeta_1, z^(2) and c_2 move,
                             layer 2's first round vector still sums to the old c_2: ROUND_SUM at (2, 0);
  a used slot + 1            the round's own sum moves by 1 (2 for the constant term): ROUND_SUM at (k, j);
  a challenge + 1            the round's sum still holds, its hash does not: CHALLENGE at (k, j);
  a length + 1               beyond four SHAPE; else a leading zero joins the used slots -- same sum, same value at r_j, another
                             hash: CHALLENGE at (k, j);
  a length - 1               0: SHAPE; else the leading coefficient (non-zero: the prover drops leading zeros) leaves the sum:
                             ROUND_SUM at (k, j);
  a_k or b_k + 1             eq(z^(k), r^(k)) a_k b_k moves by eq times the other value: FINAL_CLAIM at (k, k) when that is non-zero.
                             Where the other value is zero (a zero half) the layer's last relation still holds, but tau_k and c_{k+1}
                             move: ROUND_SUM at (k + 1, 0), or behind the last layer EVALUATION at (n, n) -- accepted where no table is
                             given;
  the claimed product + 1    PRODUCT at (0, 0);
  a table entry + 1          V~(z^(n)) moves by eq(z^(n), i): EVALUATION at (n, n) -- INVISIBLE where that weight is zero, which takes
                             a boolean coordinate of z^(n) (hashes: never in these tests; the rule is stated and computed all the same)."""

from grand_product_model import CHALLENGE, EVALUATION, FINAL_CLAIM, PRODUCT, ROUND_SUM, SHAPE, layer_row
from oracle.field import P


def _eq_weight(z, i):
    v = 1
    for j, zj in enumerate(z):
        v = v * (zj if (i >> (len(z) - 1 - j)) & 1 else 1 - zj) % P
    return v


def tamperings(g, n, with_product, with_table):
    """-> [(name, what, (check, layer, round))] for the proof g = grand_product_model.grand_product(table, n)."""
    out = []
    head = g["head"]
    for t in range(4):
        others = 1
        for u in range(4):
            if u != t:
                others = others * head[u] % P
        out.append(("head %d" % t, ("head", t), (PRODUCT, 0, 0) if with_product and others else (ROUND_SUM, 2, 0)))
    for k, (proof, r, ab) in enumerate(g["layers"], start=2):
        for j, vec in enumerate(proof):
            for s in range(len(vec)):
                out.append(("layer %d round %d slot %d" % (k, j, s), ("slot", k, j, 4 - len(vec) + s), (ROUND_SUM, k, j)))
            out.append(("layer %d challenge %d" % (k, j), ("r", k, j), (CHALLENGE, k, j)))
            out.append(("layer %d length %d + 1" % (k, j), ("len", k, j, 1), (SHAPE if len(vec) == 4 else CHALLENGE, k, j)))
            out.append(("layer %d length %d - 1" % (k, j), ("len", k, j, -1), (SHAPE if len(vec) == 1 else ROUND_SUM, k, j)))
        for w in range(2):
            if g["eqs"][k - 2] * ab[1 - w] % P:
                want = (FINAL_CLAIM, k, k)
            elif k < n - 1:
                want = (ROUND_SUM, k + 1, 0)
            else:
                want = (EVALUATION, n, n) if with_table else (0, 0, 0)
            out.append(("layer %d value %d" % (k, w), ("eval", k, w), want))
    if with_product:
        out.append(("claimed product", ("product",), (PRODUCT, 0, 0)))
    if with_table:
        for i in range(1 << n):
            out.append(("table entry %d" % i, ("table", i), (EVALUATION, n, n) if _eq_weight(g["point"], i) else (0, 0, 0)))
    return out


def apply(what, arrays, table, product):
    """One change on copies: arrays = (head, C, L, R, E) of grand_product_model.proof_arrays -> (arrays, table, product)."""
    head, C, L, R, E = list(arrays[0]), [list(c) for c in arrays[1]], list(arrays[2]), list(arrays[3]), [list(e) for e in arrays[4]]
    table = list(table) if table is not None else None
    kind = what[0]
    if kind == "head":
        head[what[1]] = (head[what[1]] + 1) % P
    elif kind == "slot":
        row = layer_row(what[1]) + what[2]
        C[row][what[3]] = (C[row][what[3]] + 1) % P
    elif kind == "r":
        row = layer_row(what[1]) + what[2]
        R[row] = (R[row] + 1) % P
    elif kind == "len":
        L[layer_row(what[1]) + what[2]] += what[3]
    elif kind == "eval":
        E[what[1] - 2][what[2]] = (E[what[1] - 2][what[2]] + 1) % P
    elif kind == "product":
        product = (product + 1) % P
    else:
        assert kind == "table", kind
        table[what[1]] = (table[what[1]] + 1) % P
    return (head, C, L, R, E), table, product


def layers_of(arrays, n):
    """(head, C, L, R, E) -> the (rounds, challenges, (a, b)) per layer the integer verifiers take; a row whose length is outside
    1 .. 4 becomes a vector of that many zeros (SHAPE: its slots are not read)."""
    head, C, L, R, E = arrays
    layers = []
    for k in range(2, n):
        row = layer_row(k)
        proof = [C[row + j][4 - L[row + j]:] if 1 <= L[row + j] <= 4 else [0] * L[row + j] for j in range(k)]
        layers.append((proof, R[row:row + k], tuple(E[k - 2])))
    return layers
