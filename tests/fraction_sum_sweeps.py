"""Single-element changes of a fractional sum proof and the verdict each must get, shared by tests/test_fraction_sum_host.py (the
integer verifiers) and tests/test_gpu_fraction_sum.py (the device verifier, honest and tampered proofs in one batch).

A change is (name, what); apply(..) makes the changed proof.  what = (kind, index.., mode): mode "+1" adds one modulo r, ">=r" puts
r itself in a proof element's place and entry + r in a table entry's, 0 and 5 are the new lengths.  The expected verdict
(check, layer, round) is worked out here in CLOSED FORM from the rules of the header, position by position -- no verifier is run
to get it:
  a head entry + 1           p_2[t]: P moves by the product of the other three q_2 entries; q_2[t]: Q moves by that product and stays
                             non-zero while q_2[t] != r - 1.  With claimed sums the pair differs from the root: FRACTION_SUM at (0, 0).
                             Without, zeta_1, z^(2) and both claims move, layer 2's first round vector still sums to the old claim:
                             ROUND_SUM at (2, 0);
  a claimed sum + 1          FRACTION_SUM at (0, 0);
  a used slot + 1            the round's own sum moves by 1 (2 for the constant term): ROUND_SUM at (k, j);
  an unused slot             never read, whatever it holds: accepted;
  a challenge + 1            the round's sum still holds, its hash does not: CHALLENGE at (k, j);
  a length -> 0 or 5         SHAPE at (k, j);
  a length + 1 or - 1        (length_steps) + 1: beyond four SHAPE, else a leading zero joins the used slots -- same sum, same value
                             at r_j, another hash: CHALLENGE at (k, j).  - 1: 0 is SHAPE, else the leading coefficient (non-zero: the
                             prover drops leading zeros) leaves the sum: ROUND_SUM at (k, j);
  a0, a1, b0 or b1 + 1       eq(z^(k), r^(k)) (a0 b1 + a1 b0 + lambda_k b0 b1) moves by eq times the value's cofactor -- b1, b0,
                             a1 + lambda_k b1, a0 + lambda_k b0: FINAL_CLAIM at (k, k);
  an entry of N or D + 1     N~(z^(n)) or D~(z^(n)) moves by eq(z^(n), i): EVALUATION at (n, n);
  an element >= r            NON_CANONICAL at (0, 0) for a head entry or a claimed sum, at (k, j) for a used slot or a challenge, at
                             (k, k) for a value; a table entry is read modulo r: entry + r is accepted.
Every "moves by" above has a cofactor; check_inputs asserts on the sweep's own inputs that none of them is zero, so no rule has
an exception."""

from fraction_sum_model import (CHALLENGE, EVALUATION, FINAL_CLAIM, FRACTION_SUM, NON_CANONICAL, ROUND_SUM, SHAPE, head_root, layer_row)
from oracle.field import P

ACCEPTED = (0, 0, 0)


def _eq_weight(z, i):
    v = 1
    for j, zj in enumerate(z):
        v = v * (zj if (i >> (len(z) - 1 - j)) & 1 else 1 - zj) % P
    return v


def table_entries(n):
    """The entry of N and the entry of D the sweep changes."""
    return 1, (1 << n) - 2


def check_inputs(g, n, num, den):
    """The sweep's inputs have no zero cofactor: every entry of N and D non-zero, Q != 0, no q_2 entry 0 or r - 1, and per layer
    eq(z^(k), r^(k)) and the four values' cofactors non-zero; the changed table entries have non-zero weights at z^(n)."""
    assert all(x % P for x in num) and all(x % P for x in den)
    check_cofactors(g, n)
    assert all(_eq_weight(g["point"], i) for i in table_entries(n))


def check_cofactors(g, n):
    """The part of check_inputs that needs the proof alone (a pair with zero numerators, as a lookup's, can pass it)."""
    assert head_root(g["head"])[1] != 0 and all(q not in (0, P - 1) for q in g["head"][4:])
    for k, (_, _, (a0, a1, b0, b1)) in enumerate(g["layers"], start=2):
        lam = g["lambdas"][k - 2]
        assert g["eqs"][k - 2] and b1 and b0 and (a1 + lam * b1) % P and (a0 + lam * b0) % P, k


def tamperings(g, n, with_sums, with_tables, length_steps=False):
    """-> [(name, what, (check, layer, round))] for the proof g = fraction_sum_model.fraction_sum(N, D, n); length_steps adds a
    length + 1 and a length - 1 per round."""
    out = []
    for t in range(8):
        out.append(("head %d + 1" % t, ("head", t, "+1"), (FRACTION_SUM, 0, 0) if with_sums else (ROUND_SUM, 2, 0)))
        out.append(("head %d >= r" % t, ("head", t, ">=r"), (NON_CANONICAL, 0, 0)))
    if with_sums:
        for t in range(2):
            out.append(("claimed sum %d + 1" % t, ("sum", t, "+1"), (FRACTION_SUM, 0, 0)))
            out.append(("claimed sum %d >= r" % t, ("sum", t, ">=r"), (NON_CANONICAL, 0, 0)))
    for k, (proof, r, vals) in enumerate(g["layers"], start=2):
        for j, vec in enumerate(proof):
            for s in range(len(vec)):
                at = "layer %d round %d slot %d" % (k, j, 4 - len(vec) + s)
                out.append((at + " + 1", ("slot", k, j, 4 - len(vec) + s, "+1"), (ROUND_SUM, k, j)))
                out.append((at + " >= r", ("slot", k, j, 4 - len(vec) + s, ">=r"), (NON_CANONICAL, k, j)))
            if len(vec) < 4:
                out.append(("layer %d round %d unused slot + 1" % (k, j), ("slot", k, j, 0, "+1"), ACCEPTED))
                out.append(("layer %d round %d unused slot >= r" % (k, j), ("slot", k, j, 0, ">=r"), ACCEPTED))
            out.append(("layer %d challenge %d + 1" % (k, j), ("r", k, j, "+1"), (CHALLENGE, k, j)))
            out.append(("layer %d challenge %d >= r" % (k, j), ("r", k, j, ">=r"), (NON_CANONICAL, k, j)))
            out.append(("layer %d length %d -> 0" % (k, j), ("len", k, j, 0), (SHAPE, k, j)))
            out.append(("layer %d length %d -> 5" % (k, j), ("len", k, j, 5), (SHAPE, k, j)))
            if length_steps:
                out.append(("layer %d length %d + 1" % (k, j), ("len", k, j, len(vec) + 1), (SHAPE if len(vec) == 4 else CHALLENGE, k, j)))
                out.append(("layer %d length %d - 1" % (k, j), ("len", k, j, len(vec) - 1), (SHAPE if len(vec) == 1 else ROUND_SUM, k, j)))
        for w in range(4):
            out.append(("layer %d value %d + 1" % (k, w), ("eval", k, w, "+1"), (FINAL_CLAIM, k, k)))
            out.append(("layer %d value %d >= r" % (k, w), ("eval", k, w, ">=r"), (NON_CANONICAL, k, k)))
    if with_tables:
        for which, i in zip(("num", "den"), table_entries(n)):
            out.append(("%s entry %d + 1" % (which, i), (which, i, "+1"), (EVALUATION, n, n)))
            out.append(("%s entry %d + r" % (which, i), (which, i, ">=r"), ACCEPTED))
    return out


def _changed(x, mode):
    return (x + 1) % P if mode == "+1" else P


def apply(what, arrays, num, den, sums):
    """One change on copies: arrays = (head, C, L, R, E) of fraction_sum_model.proof_arrays -> (arrays, num, den, sums)."""
    head, C, L, R, E = list(arrays[0]), [list(c) for c in arrays[1]], list(arrays[2]), list(arrays[3]), [list(e) for e in arrays[4]]
    num, den = (list(num), list(den)) if num is not None else (None, None)
    sums = list(sums) if sums is not None else None
    kind = what[0]
    if kind == "head":
        head[what[1]] = _changed(head[what[1]], what[2])
    elif kind == "sum":
        sums[what[1]] = _changed(sums[what[1]], what[2])
    elif kind == "slot":
        row = layer_row(what[1]) + what[2]
        C[row][what[3]] = _changed(C[row][what[3]], what[4])
    elif kind == "r":
        row = layer_row(what[1]) + what[2]
        R[row] = _changed(R[row], what[3])
    elif kind == "len":
        L[layer_row(what[1]) + what[2]] = what[3]
    elif kind == "eval":
        E[what[1] - 2][what[2]] = _changed(E[what[1] - 2][what[2]], what[3])
    else:
        table = {"num": num, "den": den}[kind]
        table[what[1]] = (table[what[1]] + 1) % P if what[2] == "+1" else table[what[1]] + P
    return (head, C, L, R, E), num, den, sums


def layers_of(arrays, n):
    """(head, C, L, R, E) -> the (rounds, challenges, (a0, a1, b0, b1)) per layer the integer verifiers take; a row whose length is
    outside 1 .. 4 becomes a vector of that many zeros (SHAPE: its slots are not read)."""
    head, C, L, R, E = arrays
    layers = []
    for k in range(2, n):
        row = layer_row(k)
        proof = [C[row + j][4 - L[row + j]:] if 1 <= L[row + j] <= 4 else [0] * L[row + j] for j in range(k)]
        layers.append((proof, R[row:row + k], tuple(E[k - 2])))
    return layers
