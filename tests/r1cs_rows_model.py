"""Integer model of the R1CS zero-check's tables (include/gkr_amd.h, gkr_r1cs_csr_* / gkr_r1cs_rows_device), straight from
R1cs.constraints(): constraints = [(A, B, C)], each a list of (coefficient, wire).

  rows(constraints, witness, n)       -> [Az, Bz, Cz], each 2^n integers: entry i = sum coeff * witness[wire] mod r over the
                                         combination of constraint i, zero for i >= len(constraints)
  first_bad(constraints, witness, n)  -> the lowest constraint index with Az[i] * Bz[i] != Cz[i], or None
  csr(constraints)                    -> ([(row_ptr, terms, long_rows)] per matrix, pool): the flattening of r1cs.cpp restated"""

from oracle.field import P

LONG_ROW = 32            # GKR_R1CS_LONG_ROW: a row with MORE terms than this is a long row


def table_log2(n_constraints):
    n = 2
    while (1 << n) < n_constraints:
        n += 1
    return n


def rows(constraints, witness, n):
    assert len(constraints) <= 1 << n
    out = [[0] * (1 << n) for _ in range(3)]
    for i, con in enumerate(constraints):
        for m in range(3):
            out[m][i] = sum(c * witness[w] for c, w in con[m]) % P
    return out


def first_bad(constraints, witness, n):
    a, b, c = rows(constraints, witness, n)
    for i in range(len(constraints)):
        if a[i] * b[i] % P != c[i]:
            return i
    return None


def csr(constraints):
    """One pool for the three matrices: 1, r - 1, then the other non-zero coefficients in order of first appearance (constraint by
    constraint, A, B, C, a combination's terms in their order).  A zero coefficient's term is dropped; a repeated wire stays."""
    pool, index = [1, P - 1], {1: 0, P - 1: 1}
    mats = [([0], [], []) for _ in range(3)]
    for i, con in enumerate(constraints):
        for m in range(3):
            row_ptr, terms, long_rows = mats[m]
            kept = 0
            for c, w in con[m]:
                c %= P
                if c == 0:
                    continue
                if c not in index:
                    index[c] = len(pool)
                    pool.append(c)
                terms.append((w, index[c]))
                kept += 1
            row_ptr.append(len(terms))
            if kept > LONG_ROW:
                long_rows.append(i)
    return mats, pool
