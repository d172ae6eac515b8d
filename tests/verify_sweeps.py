"""Generators shared by the verifier sweeps (test_verifier_sweep.py on the CPU, test_gpu_verify_sweep.py on the device): every
single-element change of a proof in gkr_proof_buf layout, and the closed-form model of its verdict.

A proof is the nine arrays [coeffs, lens, challenges, q, q_len, z, r, d_coeffs, input_coeffs] with the proof as first axis.
The model follows the order of the relations in csrc/verify_core.h (which is the reference's, python/gkr.py:202-231):

  * nothing reads D[S] for S != 0 (z[0] = 0 makes every other monomial vanish), slot t < 3 - len of a round vector, or slot
    t < k + 1 - q_len of q: a changed value there is accepted -- unless it is >= r in D, whose canonical scan covers the table;
  * every other element is read by exactly one relation first, and x + 1 there is a rejection;
  * the modulus r in a read element is check 2 at the element's layer for the scanned arrays (round coefficients, challenges,
    q, D at layer 0, input_func at layer L), check 7 for r*, check 3 for z[0] and check 8 at layer i for z[i + 1].
"""

from typing import List, NamedTuple, Tuple

import numpy as np

from gkr_amd import GKRCircuit, Layer
from gkr_amd.field import MODULUS

MASK64 = (1 << 64) - 1
COEFFS, LENS, CHALLENGES, Q, Q_LEN, Z, R_STAR, D, INPUT = range(9)
FIELD_ARRAYS = (COEFFS, CHALLENGES, Q, Z, R_STAR, D, INPUT)
NAMES = ["sumcheck_coeffs", "sumcheck_len", "sumcheck_r", "q", "q_len", "z", "r", "d_coeffs", "input_coeffs"]
ACCEPTED = (True, 0, 0)


def limbs(v):
    """Any 256-bit integer as four uint64 limbs, NOT reduced (field.to_limbs reduces: it cannot make an element >= r)."""
    return np.array([(v >> (64 * i)) & MASK64 for i in range(4)], dtype=np.uint64)


def value(x):
    return sum(int(w) << (64 * i) for i, w in enumerate(x))


R_LIMBS = limbs(MODULUS)


def circuit_of(layers, n_inputs):
    ks = [max(0, (len(l[0]) - 1).bit_length()) for l in layers] + [max(0, (n_inputs - 1).bit_length())]
    return GKRCircuit([Layer(ks[i], *layers[i]) for i in range(len(layers))], ks[-1])


class Element(NamedTuple):
    arr: int                   # which of the nine arrays
    index: Tuple[int, ...]     # the element's index behind the proof axis
    layer: int                 # the layer whose relation reads it first
    read: bool                 # does any relation read its value?  (x + 1 is rejected iff read)
    mod_verdict: Tuple[bool, int, int]   # the verdict with the modulus r in its place


def elements(ks, arrs, b=0) -> List[Element]:
    """Every field element of proof b, in the arrays' order.  Reads the proof's own lengths: they decide which slots are used."""
    L = len(ks) - 1
    sl, ql = arrs[LENS][b], arrs[Q_LEN][b]
    out = []
    row = 0
    for i in range(L):
        for j in range(2 * ks[i + 1]):
            for t in range(3):
                used = t >= 3 - int(sl[row])
                out.append(Element(COEFFS, (row, t), i, used, (False, i, 2) if used else ACCEPTED))
            row += 1
    row = 0
    for i in range(L):
        for j in range(2 * ks[i + 1]):
            out.append(Element(CHALLENGES, (row,), i, True, (False, i, 2)))
            row += 1
    qo = 0
    for i in range(L):
        for t in range(ks[i + 1] + 1):
            used = t >= ks[i + 1] + 1 - int(ql[i])
            out.append(Element(Q, (qo + t,), i, used, (False, i, 2) if used else ACCEPTED))
        qo += ks[i + 1] + 1
    zo = 0
    for i in range(L + 1):
        for j in range(ks[i]):
            out.append(Element(Z, (zo + j,), max(i - 1, 0), True, (False, 0, 3) if i == 0 else (False, i - 1, 8)))
        zo += ks[i]
    for i in range(L):
        out.append(Element(R_STAR, (i,), i, True, (False, i, 7)))
    for s in range(1 << ks[0]):
        out.append(Element(D, (s,), 0, s == 0, (False, 0, 2)))
    for s in range(1 << ks[L]):
        out.append(Element(INPUT, (s,), L, True, (False, L, 2)))
    return out


def replicate(arrs, n, b=0):
    """Proof b of the arrays, n times."""
    return [np.ascontiguousarray(np.repeat(a[b:b + 1], n, axis=0)) for a in arrs]


def element_sweep(arrs, elems, mode, b=0):
    """A batch of len(elems) copies of proof b, copy e with element e replaced: by x + 1 mod r ("plus1") or by r ("mod")."""
    bad = replicate(arrs, len(elems), b)
    for e, el in enumerate(elems):
        at = (e,) + el.index
        bad[el.arr][at] = R_LIMBS if mode == "mod" else limbs((value(bad[el.arr][at]) + 1) % MODULUS)
    return bad


def length_cases(ks, arrs, b=0):
    """[(array, index, new length)]: every sumcheck_len as each of 0..5 and every q_len as each of 0..7, its own value left out."""
    L = len(ks) - 1
    cases = []
    for row in range(arrs[LENS].shape[1]):
        cases += [(LENS, (row,), v) for v in range(6) if v != int(arrs[LENS][b, row])]
    for i in range(L):
        cases += [(Q_LEN, (i,), v) for v in range(8) if v != int(arrs[Q_LEN][b, i])]
    return cases


def length_sweep(arrs, cases, b=0):
    bad = replicate(arrs, len(cases), b)
    for e, (arr, index, v) in enumerate(cases):
        bad[arr][(e,) + index] = v
    return bad


def q_grown_over_zeros(ks, arrs, case, b=0):
    """Is the case a q_len grown, inside its k + 1 slots, over leading slots that are zero?  Then q is the same polynomial."""
    arr, (i,), v = case
    if arr != Q_LEN:
        return False
    k, old = ks[i + 1], int(arrs[Q_LEN][b, i])
    qo = sum(ks[j + 1] + 1 for j in range(i))
    return old < v <= k + 1 and not arrs[Q][b, qo + k + 1 - v:qo + k + 1 - old].any()


def positions(n, wanted=(0, 255, 256, -1)):
    """The wanted indices that exist in a table of n entries (-1: the last), without repeats, ascending."""
    return sorted({p % n for p in wanted if -n <= p < n})
