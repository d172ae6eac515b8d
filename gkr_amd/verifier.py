"""GKR verifier for the proofs this library produces (host side, plain integers).

Mirrors the reference's Python verifier -- python/gkr.py:202-231 and
python/sumcheck.py:55-70 (the circom one, gkr-verifier-circuits/circom/circom/verifier.circom:39-71,
checks the same relations inside a circuit) -- on the Rust prover's Proof (rust/src/gkr.rs:7-19),
which carries no `f` field: the last sumcheck claim is compared with
add(z, b*, c*) (q(0) + q(1)) + mult(z, b*, c*) q(0) q(1) directly.

Verification is O(gates * k) per layer of cheap arithmetic; it is not on the accelerated path.  It gives an
end-to-end check of a proof that needs neither the CPU checker under tests/ nor the reference.
"""

from typing import List

from . import _native as N
from .field import MODULUS as P
from .prover import GKRCircuit, Proof, multi_hash


def eval_univariate(coeffs: List[int], x: int) -> int:
    """Horner, highest degree first (rust/src/gkr/poly.rs:260-267)."""
    acc = 0
    for c in coeffs:
        acc = (acc * x + c) % P
    return acc


def eval_expansion(terms: List[List[int]], point: List[int]) -> int:
    """sum_t coeff_t * prod_i point_i^{e_ti} (python/poly.py:293-305)."""
    total = 0
    for t in terms:
        v = t[0] % P
        for e, x in zip(t[1:], point):
            if e:
                v = v * pow(x, e, P) % P
        total = (total + v) % P
    return total


def _eq_bits(point: List[int], index: int) -> int:
    """prod_i (bit_i(index) ? point_i : 1 - point_i), variable 1 = most significant bit."""
    k = len(point)
    v = 1
    for i, x in enumerate(point):
        v = v * (x if (index >> (k - 1 - i)) & 1 else 1 - x) % P
    return v


def wiring_at(layer, z: List[int], b: List[int], c: List[int]):
    """(add_i, mult_i) of a layer evaluated at (z, b, c): sum over its gates of
    eq(z, g) eq(b, left_g) eq(c, right_g)  (chi_w_for_binary terms, rust/src/gkr/poly.rs:28-41)."""
    k = len(b)
    eq_b = [_eq_bits(b, i) for i in range(1 << k)]
    eq_c = [_eq_bits(c, i) for i in range(1 << k)]
    add = mult = 0
    for g, (ty, l, r) in enumerate(zip(layer.gate_type, layer.left, layer.right)):
        w = _eq_bits(z, g) * eq_b[int(l)] % P * eq_c[int(r)] % P
        if int(ty):
            mult = (mult + w) % P
        else:
            add = (add + w) % P
    return add, mult


def verify_sumcheck(claim: int, rounds: List[List[int]], challenges: List[int]):
    """python/sumcheck.py:55-70.  Returns (ok, final claim g_v(r_v))."""
    expected = claim % P
    for g, r in zip(rounds, challenges):
        if (eval_univariate(g, 0) + eval_univariate(g, 1)) % P != expected:
            return False, expected
        if multi_hash(g, 0) != r % P:
            return False, expected
        expected = eval_univariate(g, r)
    return True, expected


def mle_eval(table: List[int], point: List[int]) -> int:
    """The multilinear extension of a table of 2^n values at a point, variable 1 = most significant index bit: n folds
    T'[i] = T[i] + r (T[i + half] - T[i]) (partial_eval_i, rust/src/gkr/poly.rs:160-179)."""
    t = [x % P for x in table]
    if len(t) != 1 << len(point):
        raise ValueError("a table of 2^n values and a point of n coordinates expected")
    for r in point:
        half = len(t) // 2
        t = [(t[i] + r * (t[i + half] - t[i])) % P for i in range(half)]
    return t[0]


def verify_sumcheck_table(table: List[int], rounds: List[List[int]], challenges: List[int], claim=None) -> bool:
    """What Context.verify_sumcheck decides on the device, on plain integers: python/sumcheck.py:55-70 on the claim (the first
    round vector's own sum when none is given) and the relation that ties the transcript to its table, g_n(r_n) = T(r_1 .. r_n)."""
    if claim is None:
        claim = eval_univariate(rounds[0], 0) + eval_univariate(rounds[0], 1)
    ok, last = verify_sumcheck(claim, rounds, challenges)
    return ok and last == mle_eval(table, [r % P for r in challenges])


def verify_sumcheck_product(rounds: List[List[int]], challenges: List[int], evals: List[int], degree: int, claim=None, hashes=None) -> bool:
    """The verifier of a product sumcheck's transcript (Context.prove_sumcheck_product) on plain integers: every round vector
    has 1 .. degree + 1 coefficients, python/sumcheck.py:55-70 holds on the claim (the first round vector's own sum when none
    is given), and g_n(r_n) == prod evals.  That evals[f] is factor f's multilinear extension at the challenges is NOT checked
    here: Context.verify_sumcheck_product (host tables) and Context.verify_sumcheck_product_batch_device (resident tables) check
    the transcript against the tables themselves, on the device, and return the values they computed.
    hashes: multi_hash(rounds[j], 0) for every j, computed by the caller (many transcripts: all their round vectors in one
    Context.multi_hash_batch call); None: hashed here, one vector at a time."""
    if len(rounds) < 1 or len(rounds) != len(challenges) or len(evals) != degree:
        return False
    if any(not 1 <= len(g) <= degree + 1 for g in rounds) or (hashes is not None and len(hashes) != len(rounds)):
        return False
    expected = (eval_univariate(rounds[0], 0) + eval_univariate(rounds[0], 1) if claim is None else claim) % P
    for j, (g, r) in enumerate(zip(rounds, challenges)):
        if (eval_univariate(g, 0) + eval_univariate(g, 1)) % P != expected:
            return False
        if (multi_hash(g, 0) if hashes is None else hashes[j] % P) != r % P:
            return False
        expected = eval_univariate(g, r)
    prod = 1
    for e in evals:
        prod = prod * e % P
    return expected == prod


def verify_sumcheck_sop(rounds: List[List[int]], challenges: List[int], evals: List[int], terms, claim=None) -> bool:
    """The verifier of a sum-of-products sumcheck's transcript (Context.prove_sumcheck_sop) on plain integers.  terms:
    [(coeff, (table indices ..)), ..] as the prover took them; evals[m] the value of table m at the challenges.  Every round
    vector has 1 .. D + 1 coefficients (D the largest term degree), python/sumcheck.py:55-70 holds on the claim (the first
    round vector's own sum when none is given), and g_n(r_n) == sum_k c_k prod_j evals[t(k,j)].  That evals[m] is table m's
    multilinear extension at the challenges is NOT checked here: Context.verify_sumcheck_sop (host tables) and
    Context.verify_sumcheck_sop_batch_device (resident tables) check the transcript against the tables themselves, on the device,
    and return the values they computed."""
    if len(terms) < 1 or any(not 1 <= len(idx) <= 3 or any(not 0 <= i < len(evals) for i in idx) for _, idx in terms):
        return False
    degree = max(len(idx) for _, idx in terms)
    if len(rounds) < 1 or len(rounds) != len(challenges) or any(not 1 <= len(g) <= degree + 1 for g in rounds):
        return False
    expected = (eval_univariate(rounds[0], 0) + eval_univariate(rounds[0], 1) if claim is None else claim) % P
    for g, r in zip(rounds, challenges):
        if (eval_univariate(g, 0) + eval_univariate(g, 1)) % P != expected:
            return False
        if multi_hash(g, 0) != r % P:
            return False
        expected = eval_univariate(g, r)
    total = 0
    for c, idx in terms:
        prod = c % P
        for i in idx:
            prod = prod * evals[i] % P
        total = (total + prod) % P
    return expected == total


# the R1CS zero-check eq(z, .) (Az * Bz - Cz) over the tables [Az, Bz, Cz] (Context.prove_r1cs_zerocheck): verify_sumcheck_zerocheck's terms
R1CS_ZEROCHECK_TERMS = [(1, (0, 1)), (P - 1, (2,))]


def verify_sumcheck_zerocheck(rounds: List[List[int]], challenges: List[int], evals: List[int], terms, z: List[int], claim=None) -> bool:
    """The verifier of a zero-check's transcript (Context.prove_zerocheck) on plain integers.  terms: [(coeff, (table
    indices ..)), ..] of 1 or 2 indices each as the prover took them; evals[m] the value of table m at the challenges; z the
    point of eq(z, .).  Every round vector has 1 .. D + 1 coefficients (D = the largest term degree + 1), python/sumcheck.py:55-70
    holds on the claim (the first round vector's own sum when none is given; a zero-check passes 0), and
    g_n(r_n) == eq(z, r) * sum_k c_k prod_j evals[t(k,j)] with eq(z, r) = prod_j (z_j r_j + (1 - z_j)(1 - r_j)), n products.  That
    evals[m] is table m's multilinear extension at the challenges is NOT checked here (Context.verify_sumcheck_sop_batch_device on
    the tables and Context.eq_table_device's table checks it on the device)."""
    if len(terms) < 1 or any(not 1 <= len(idx) <= 2 or any(not 0 <= i < len(evals) for i in idx) for _, idx in terms):
        return False
    degree = max(len(idx) for _, idx in terms) + 1
    if len(rounds) < 1 or len(rounds) != len(challenges) or len(z) != len(rounds) or any(not 1 <= len(g) <= degree + 1 for g in rounds):
        return False
    expected = (eval_univariate(rounds[0], 0) + eval_univariate(rounds[0], 1) if claim is None else claim) % P
    for g, r in zip(rounds, challenges):
        if (eval_univariate(g, 0) + eval_univariate(g, 1)) % P != expected:
            return False
        if multi_hash(g, 0) != r % P:
            return False
        expected = eval_univariate(g, r)
    total = 0
    for c, idx in terms:
        prod = c % P
        for i in idx:
            prod = prod * evals[i] % P
        total = (total + prod) % P
    eq_r = 1
    for zj, rj in zip(z, challenges):
        eq_r = eq_r * (zj * rj + (1 - zj) * (1 - rj)) % P
    return expected == eq_r * total % P


def _eq_table(point: List[int]) -> List[int]:
    """[eq(point, i) for i < 2^n], variable 1 = most significant index bit."""
    t = [1]
    for x in point:
        x %= P
        t = [v * f % P for v in t for f in ((1 - x) % P, x)]
    return t


def r1cs_matrix_evals(constraints, rx: List[int], ry: List[int]) -> List[int]:
    """[A~, B~, C~](rx, ry) of an R1CS given as R1cs.constraints(): the multilinear extensions of the three matrices, rows indexed by
    rx (len(rx) variables, 2^len(rx) >= the constraints) and columns -- wires -- by ry, variable 1 = most significant index bit:
    M~(rx, ry) = sum over the terms (coefficient c, wire y) of constraint i of c eq(rx, i) eq(ry, y).  One pass over the non-zeros."""
    if len(constraints) > 1 << len(rx) or any(w >> len(ry) for con in constraints for lc in con for _, w in lc):
        raise ValueError("more constraints than 2^len(rx) or a wire past 2^len(ry)")
    ex, ey = _eq_table(rx), _eq_table(ry)
    out = [0, 0, 0]
    for i, con in enumerate(constraints):
        for m in range(3):
            s = 0
            for c, w in con[m]:
                s += c * ey[w]
            out[m] = (out[m] + ex[i] * (s % P)) % P
    return out


def verify_r1cs_inner(constraints, rx: List[int], rho: List[int], claims_abc: List[int], rounds: List[List[int]], challenges: List[int],
                      evals: List[int]):
    """The verifier of the R1CS inner sumcheck (Context.prove_r1cs_inner) on plain integers.  claims_abc = [Az~(rx), Bz~(rx),
    Cz~(rx)], the zero-check's evals at its challenges rx; rho the three weights; evals = [T~(ry), w~(ry)] with ry = challenges.
    The degree-2 checks of verify_sumcheck_product with claim = sum_m rho_m claims_abc[m], then
    evals[0] == sum_m rho_m M_m~(rx, ry) from the public matrices (r1cs_matrix_evals).  -> the claim left on the witness,
    (ry, evals[1]): w~(ry) == evals[1] is one evaluation of the (committed) witness and NOT checked here; None on a rejection."""
    if len(rho) != 3 or len(claims_abc) != 3 or len(evals) != 2:
        return None
    claim = sum(r * v for r, v in zip(rho, claims_abc)) % P
    if not verify_sumcheck_product(rounds, challenges, evals, 2, claim):
        return None
    ry = [r % P for r in challenges]
    try:
        mats = r1cs_matrix_evals(constraints, rx, ry)
    except ValueError:
        return None
    if evals[0] % P != sum(r * v for r, v in zip(rho, mats)) % P:
        return None
    return ry, evals[1] % P


def _transcript_form(rounds: List[List[int]], challenges: List[int], width: int, evals: List[int]):
    """The checks of a transcript that read no relation, in the device verifiers' order: (round, check) of the first round vector
    whose length is outside 1 .. width (SHAPE), else of the first round with a coefficient or a challenge outside 0 .. r - 1
    (NON_CANONICAL), else (len(rounds), NON_CANONICAL) for such an evaluation; None when there is none."""
    for j, g in enumerate(rounds):
        if not 1 <= len(g) <= width:
            return j, N.GKR_VERIFY_SHAPE
    for j, (g, r) in enumerate(zip(rounds, challenges)):
        if any(not 0 <= c < P for c in g) or not 0 <= r < P:
            return j, N.GKR_VERIFY_NON_CANONICAL
    if any(not 0 <= e < P for e in evals):
        return len(rounds), N.GKR_VERIFY_NON_CANONICAL
    return None


def _transcript_rounds(rounds: List[List[int]], challenges: List[int], claim: int):
    """python/sumcheck.py:55-70 round by round on a transcript that passed _transcript_form: -> ((round, check) of the first
    failure -- ROUND_SUM before CHALLENGE within a round -- or None, the final claim g_n(r_n))."""
    expected = claim % P
    for j, (g, r) in enumerate(zip(rounds, challenges)):
        if (eval_univariate(g, 0) + eval_univariate(g, 1)) % P != expected:
            return (j, N.GKR_VERIFY_ROUND_SUM), expected
        if multi_hash(g, 0) != r:
            return (j, N.GKR_VERIFY_CHALLENGE), expected
        expected = eval_univariate(g, r)
    return None, expected


def verify_r1cs(constraints, z: List[int], rho: List[int], zc_rounds: List[List[int]], r_x: List[int], evals_abc: List[int],
                in_rounds: List[List[int]], r_y: List[int], evals_tw: List[int], witness=None):
    """The verifier of the R1CS zero-check and inner sumcheck, tied together, on plain integers: what
    Context.verify_r1cs_batch_device decides on the device.  constraints: R1cs.constraints(); z, rho: the verifier's own point
    and weights (reduced modulo r); zc_rounds, r_x, evals_abc: the zero-check's transcript, challenges and [v_A, v_B, v_C];
    in_rounds, r_y, evals_tw: the inner sumcheck's and [e_T, e_w]; witness: None or the n_wires values (at most 2^n_y).  Proof elements
    are taken as they are: one outside 0 .. r - 1 is NON_CANONICAL.  -> (stage, round, check) of the first failure, (0, 0, 0) for
    an accepted proof:
      stage 1  verify_sumcheck_zerocheck's relations with R1CS_ZEROCHECK_TERMS and claim 0: SHAPE (rows of 1 .. 4), NON_CANONICAL
               (a round's coefficients and challenge; evals_abc at round n), per round ROUND_SUM then CHALLENGE, EVALUATION (round n)
               for g_n(r_n) != eq(z, r_x) (v_A v_B - v_C);
      stage 2  verify_r1cs_inner's transcript part: the same on rows of 1 .. 3 with claim sum_m rho_m v_m, evals_tw at round n_y,
               EVALUATION (round n_y) for g(r) != e_T e_w;
      stage 3  MATRIX (round n_y): e_T != sum_m rho_m M_m~(r_x, r_y) (r1cs_matrix_evals);
      stage 4  with a witness, WITNESS (round n_y): e_w != w~(r_y), the witness zero-padded to 2^n_y values.
    Without a witness the claim (r_y, e_w) is the caller's to settle, as with verify_r1cs_inner."""
    n, n_y = len(z), len(r_y)
    if len(rho) != 3 or len(evals_abc) != 3 or len(evals_tw) != 2 or len(zc_rounds) != n or len(r_x) != n or len(in_rounds) != n_y or n < 1 or n_y < 1:
        raise ValueError("n round vectors and challenges with three evaluations, n_y with two, three weights expected")
    z, rho = [v % P for v in z], [v % P for v in rho]
    # stage 1
    bad = _transcript_form(zc_rounds, r_x, 4, evals_abc)
    if bad is None:
        bad, last = _transcript_rounds(zc_rounds, r_x, 0)
    if bad is None:
        total = 0
        for c, idx in R1CS_ZEROCHECK_TERMS:
            prod = c
            for i in idx:
                prod = prod * evals_abc[i] % P
            total = (total + prod) % P
        eq_r = 1
        for zj, rj in zip(z, r_x):
            eq_r = eq_r * (zj * rj + (1 - zj) * (1 - rj)) % P
        if last != eq_r * total % P:
            bad = (n, N.GKR_VERIFY_EVALUATION)
    if bad is not None:
        return (1,) + bad
    # stage 2
    bad = _transcript_form(in_rounds, r_y, 3, evals_tw)
    if bad is None:
        bad, last = _transcript_rounds(in_rounds, r_y, sum(r * v for r, v in zip(rho, evals_abc)))
    if bad is None and last != evals_tw[0] * evals_tw[1] % P:
        bad = (n_y, N.GKR_VERIFY_EVALUATION)
    if bad is not None:
        return (2,) + bad
    # stage 3
    if evals_tw[0] != sum(r * v for r, v in zip(rho, r1cs_matrix_evals(constraints, r_x, r_y))) % P:
        return 3, n_y, N.GKR_VERIFY_MATRIX
    # stage 4
    if witness is not None:
        w = [int(v) % P for v in witness]
        if len(w) > 1 << n_y:
            raise ValueError("a witness of at most 2^n_y values expected")
        if evals_tw[1] != mle_eval(w + [0] * ((1 << n_y) - len(w)), r_y):
            return 4, n_y, N.GKR_VERIFY_WITNESS
    return 0, 0, 0


class _TreeGate:
    """What differs between the tree arguments (the C++ statement: csrc/tree_rounds.h and its gates): W tables per proof -- head
    4 W values, table w at [4 w, 4 w + 4); a layer's 2 W values, the halves of table w at 2 w, 2 w + 1 --, whether a lambda is
    drawn per layer, the zero-check's claim and the gate on a layer's values, form(head, claimed) -> the first failed check of
    the head or 0, and the text for a proof of another shape."""

    def __init__(self, W, draws_lambda, claim, gate, form, expected):
        self.W, self.draws_lambda, self.claim, self.gate, self.form, self.expected = W, draws_lambda, claim, gate, form, expected


def _verify_tree(head: List[int], layers, gate: _TreeGate, tables, claimed):
    """The one chain of both tree arguments: tables: the W input tables or None; claimed: the W claimed root values or None.
    -> (check, layer, round) as verify_grand_product and verify_fraction_sum document it."""
    n, W = len(layers) + 2, gate.W
    if len(head) != 4 * W or any(len(lay) != 3 or len(lay[0]) != k or len(lay[1]) != k or len(lay[2]) != 2 * W
                                 for k, lay in enumerate(layers, start=2)):
        raise ValueError(gate.expected)
    for k, (rounds, _, _) in enumerate(layers, start=2):
        for j, g in enumerate(rounds):
            if not 1 <= len(g) <= 4:
                return N.GKR_VERIFY_SHAPE, k, j
    if any(not 0 <= h < P for h in head) or (claimed is not None and any(not 0 <= s < P for s in claimed)):
        return N.GKR_VERIFY_NON_CANONICAL, 0, 0
    for k, (rounds, challenges, vals) in enumerate(layers, start=2):
        bad = _transcript_form(rounds, challenges, 4, vals)
        if bad is not None:
            return bad[1], k, bad[0]
    check = gate.form(head, claimed)
    if check:
        return check, 0, 0
    z = [multi_hash(head, 0)]
    z.append(multi_hash([z[0]], 0))
    lam = multi_hash([z[1]], 0) if gate.draws_lambda else 0
    claims = [mle_eval(head[4 * w:4 * w + 4], z) for w in range(W)]
    for k, (rounds, challenges, vals) in enumerate(layers, start=2):
        bad, last = _transcript_rounds(rounds, challenges, gate.claim(claims, lam))
        if bad is not None:
            return bad[1], k, bad[0]
        eq_r = 1
        for zj, rj in zip(z, challenges):
            eq_r = eq_r * (zj * rj + (1 - zj) * (1 - rj)) % P
        if last != eq_r * gate.gate(vals, lam) % P:
            return N.GKR_VERIFY_FINAL_CLAIM, k, k
        tau = multi_hash(list(vals), 0)
        claims = [(vals[2 * w] + tau * (vals[2 * w + 1] - vals[2 * w])) % P for w in range(W)]
        z = [tau] + list(challenges)
        lam = multi_hash([tau], 0) if gate.draws_lambda else 0
    if tables is not None and any(c != mle_eval(t, z) for c, t in zip(claims, tables)):
        return N.GKR_VERIFY_EVALUATION, n, n
    return 0, 0, 0


_GRAND_PRODUCT = _TreeGate(
    1, False, lambda c, lam: c[0], lambda v, lam: v[0] * v[1] % P,
    lambda head, claimed: N.GKR_VERIFY_PRODUCT if claimed is not None and claimed[0] != head[0] * head[1] % P * head[2] % P * head[3] % P else 0,
    "four head values and, for layer k = 2 .., k round vectors, k challenges and two values expected")


def verify_grand_product(head: List[int], layers, table=None, product=None):
    """The verifier of a grand product proof (Context.prove_grand_product) on plain integers: what
    Context.verify_grand_product_batch_device decides on the device.  head: L_2, four values; layers[k - 2] = (rounds, challenges,
    (a_k, b_k)) of the zero-check of layer k = 2 .. n - 1; table: the 2^n values V, or None (the last claim c_n = V~(z^(n)) is then
    the caller's to settle); product: the claimed product, or None.  Proof elements are taken as they are: one outside
    0 .. r - 1 is NON_CANONICAL.  -> (check, layer, round) of the first failure, (0, 0, 0) for an accepted proof:
      SHAPE          a round vector of layer k, round j, with a length outside 1 .. 4: at (k, j);
      NON_CANONICAL  a head entry or the claimed product at (0, 0); else the first layer k with a round's coefficients or
                     challenge at (k, j), or its a_k, b_k at (k, k);
      PRODUCT        product != head[0] head[1] head[2] head[3]: at (0, 0);
      per layer k, with zeta_1 = multi_hash(head, 0), zeta_2 = multi_hash([zeta_1], 0), z^(2) = (zeta_1, zeta_2), c_2 = L_2~(z^(2)):
                     ROUND_SUM then CHALLENGE round by round against c_k at (k, j); FINAL_CLAIM at (k, k) for
                     g_k(r_k) != eq(z^(k), r^(k)) a_k b_k; then tau_k = multi_hash([a_k, b_k], 0), c_{k+1} = a_k + tau_k (b_k - a_k),
                     z^(k+1) = (tau_k, r^(k)_1 .. r^(k)_k);
      EVALUATION     with a table: c_n != V~(z^(n)): at (n, n)."""
    return _verify_tree(head, layers, _GRAND_PRODUCT, None if table is None else [table], None if product is None else [product])


def fraction_root(head: List[int]):
    """(P, Q) of a fractional sum's head p_2[0..3], q_2[0..3] by the tree rule: level 2 -> level 1 -> level 0."""
    p, q = head[:4], head[4:]
    p1 = [(p[i] * q[i + 2] + p[i + 2] * q[i]) % P for i in range(2)]
    q1 = [q[i] * q[i + 2] % P for i in range(2)]
    return (p1[0] * q1[1] + p1[1] * q1[0]) % P, q1[0] * q1[1] % P


def _fraction_form(head, claimed):
    root = fraction_root(head)
    if root[1] == 0:
        return N.GKR_VERIFY_ZERO_DENOMINATOR
    return N.GKR_VERIFY_FRACTION_SUM if claimed is not None and tuple(claimed) != root else 0


_FRACTION_SUM = _TreeGate(
    2, True, lambda c, lam: c[0] + lam * c[1], lambda v, lam: v[0] * v[3] + v[1] * v[2] + lam * v[2] % P * v[3], _fraction_form,
    "eight head values and, for layer k = 2 .., k round vectors, k challenges and four values expected")


def verify_fraction_sum(head: List[int], layers, numerators=None, denominators=None, sums=None):
    """The verifier of a fractional sum (LogUp) proof (Context.prove_fraction_sum) on plain integers: what
    Context.verify_fraction_sum_batch_device decides on the device.  head: p_2 then q_2, eight values; layers[k - 2] = (rounds,
    challenges, (a0, a1, b0, b1)) of the zero-check of layer k = 2 .. n - 1; numerators, denominators: the 2^n values N and D, or
    both None (the last claims cp_n = N~(z^(n)), cq_n = D~(z^(n)) are then the caller's to settle); sums: the claimed (P, Q), or
    None.  Proof elements are taken as they are: one outside 0 .. r - 1 is NON_CANONICAL.  -> (check, layer, round) of the first
    failure, (0, 0, 0) for an accepted proof:
      SHAPE             a round vector of layer k, round j, with a length outside 1 .. 4: at (k, j);
      NON_CANONICAL     a head entry or a claimed sum at (0, 0); else the first layer k with a round's coefficients or challenge
                        at (k, j), or one of its four values at (k, k);
      ZERO_DENOMINATOR  the head's Q (fraction_root) is 0: at (0, 0);
      FRACTION_SUM      sums != the head's (P, Q), as a pair: at (0, 0);
      per layer k, with zeta_1 = multi_hash(head, 0), zeta_2 = multi_hash([zeta_1], 0), z^(2) = (zeta_1, zeta_2),
                        lambda_2 = multi_hash([zeta_2], 0), cp_2 = p_2~(z^(2)), cq_2 = q_2~(z^(2)): ROUND_SUM then CHALLENGE round
                        by round against cp_k + lambda_k cq_k at (k, j); FINAL_CLAIM at (k, k) for
                        g_k(r_k) != eq(z^(k), r^(k)) (a0 b1 + a1 b0 + lambda_k b0 b1); then tau_k = multi_hash([a0, a1, b0, b1], 0),
                        cp_{k+1} = a0 + tau_k (a1 - a0), cq_{k+1} = b0 + tau_k (b1 - b0), z^(k+1) = (tau_k, r^(k)_1 .. r^(k)_k),
                        lambda_{k+1} = multi_hash([tau_k], 0);
      EVALUATION        with tables: cp_n != N~(z^(n)) or cq_n != D~(z^(n)): at (n, n)."""
    if (numerators is None) != (denominators is None) or (sums is not None and len(sums) != 2):
        raise ValueError("both tables or neither, and two claimed sums or None expected")
    return _verify_tree(head, layers, _FRACTION_SUM, None if numerators is None else [numerators, denominators], sums)


def lookup_pair(witness: List[int], table: List[int], mult: List[int], alpha: int):
    """(N, D) of a lookup (include/gkr_amd.h, LOOKUP): 2^L entries each, L = max(n_w, n_t) + 1; (1, alpha - W[i]) then (0, 1) on the
    first half, (-M[j], alpha - T[j]) then (0, 1) on the second."""
    half = max(len(witness), len(table))
    if len(witness) < 4 or len(table) < 4 or len(witness) & (len(witness) - 1) or len(table) & (len(table) - 1) or len(mult) != len(table):
        raise ValueError("a witness of 2^n_w values, a table and multiplicities of 2^n_t values, n_w, n_t >= 2, expected")
    num = [1] * len(witness) + [0] * (half - len(witness)) + [-int(m) % P for m in mult] + [0] * (half - len(table))
    den = [(alpha - int(w)) % P for w in witness] + [1] * (half - len(witness)) + [(alpha - int(t)) % P for t in table] + [1] * (half - len(table))
    return num, den


def verify_lookup(witness: List[int], table: List[int], mult: List[int], alpha: int, head: List[int], layers):
    """The verifier of a lookup proof (Context.prove_lookup) on plain integers: what Context.verify_lookup_batch_device decides on the
    device.  verify_fraction_sum's verdict on the pair lookup_pair(witness, table, mult, alpha), without claimed sums, with one
    addition: LOOKUP at (0, 0) where the head's P (fraction_root) is not 0 -- after SHAPE, NON_CANONICAL and ZERO_DENOMINATOR, before
    the layers' relations and EVALUATION."""
    num, den = lookup_pair(witness, table, mult, alpha)
    if len(layers) + 2 != len(num).bit_length() - 1:
        raise ValueError("max(n_w, n_t) - 1 layers expected")
    verdict = verify_fraction_sum(head, layers, num, den, None)
    if verdict[0] in (N.GKR_VERIFY_SHAPE, N.GKR_VERIFY_NON_CANONICAL, N.GKR_VERIFY_ZERO_DENOMINATOR):
        return verdict
    return (N.GKR_VERIFY_LOOKUP, 0, 0) if fraction_root(head)[0] != 0 else verdict


def verify(proof: Proof, circuit: GKRCircuit) -> bool:
    """python/gkr.py:202-231 on the Rust-shaped proof."""
    L = circuit.depth()
    if proof.depth != L + 1 or proof.k != circuit.get_k_list():
        return False
    if len(proof.z[0]) != proof.k[0] or any(x % P for x in proof.z[0]):
        return False                       # the Rust prover fixes z[0] = 0 (prover.rs:16-21)
    m = eval_expansion(proof.d, proof.z[0])
    for i in range(L):
        k = proof.k[i + 1]
        rounds, rs = proof.sumcheck_proofs[i], proof.sumcheck_r[i]
        if len(rounds) != 2 * k or len(rs) != 2 * k:
            return False
        ok, last = verify_sumcheck(m, rounds, rs)
        if not ok:
            return False
        b_star, c_star = rs[:k], rs[k:]
        q = proof.q[i]
        q0, q1 = eval_univariate(q, 0), eval_univariate(q, 1)
        add, mult = wiring_at(circuit.layer[i], proof.z[i], b_star, c_star)
        if last != (add * (q0 + q1) + mult * q0 % P * q1) % P:
            return False
        if proof.r[i] % P != multi_hash(rounds[-1], 0):
            return False
        if [x % P for x in proof.z[i + 1]] != [(bi + proof.r[i] * (ci - bi)) % P for bi, ci in zip(b_star, c_star)]:
            return False
        m = eval_univariate(q, proof.r[i])
    return m == eval_expansion(proof.input_func, proof.z[L])
