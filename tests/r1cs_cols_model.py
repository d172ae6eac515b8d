"""Integer model of the R1CS inner sumcheck's table (include/gkr_amd.h, gkr_r1cs_csc_* / gkr_r1cs_cols_device), straight from
R1cs.constraints(): constraints = [(A, B, C)], each a list of (coefficient, wire).

  n_y_of(n_wires)                               -> max(2, ceil(log2 n_wires)): T and the padded witness have 2^n_y entries
  csc(constraints, n_wires)                     -> ([(col_ptr, terms, long_cols)] per matrix, pool): the column-major flattening of
                                                   r1cs.cpp restated -- the records of r1cs_rows_model.csr, its pool, sorted
                                                   stably by wire, the ROW in a record's first field
  cols_table(constraints, n_wires, rx, rho, n_y) -> T, 2^n_y integers: T[y] = sum_m rho_m sum_i M_m[i][y] eq(rx, i) mod r, zero for
                                                   y >= n_wires
  eq_table(rx)                                  -> [eq(rx, i)], variable 1 = most significant index bit"""

from oracle.field import P
from r1cs_rows_model import csr

LONG_COL = 32            # GKR_R1CS_LONG_COL: a column with MORE records than this is a long column


def n_y_of(n_wires):
    n = 2
    while (1 << n) < n_wires:
        n += 1
    return n


def eq_table(rx):
    t = [1]
    for x in rx:
        t = [v * f % P for v in t for f in ((1 - x) % P, x % P)]
    return t


def csc(constraints, n_wires):
    mats, pool = csr(constraints)
    out = []
    for row_ptr, terms, _ in mats:
        cols = [[] for _ in range(n_wires)]
        for i in range(len(row_ptr) - 1):
            for w, c in terms[row_ptr[i]:row_ptr[i + 1]]:          # rows ascending, a row's records in the CSR order: a stable sort
                cols[w].append((i, c))
        col_ptr, recs, long_cols = [0], [], []
        for y, col in enumerate(cols):
            recs.extend(col)
            col_ptr.append(len(recs))
            if len(col) > LONG_COL:
                long_cols.append(y)
        out.append((col_ptr, recs, long_cols))
    return out, pool


def cols_table(constraints, n_wires, rx, rho, n_y):
    assert n_wires <= 1 << n_y and len(constraints) <= 1 << len(rx)
    e = eq_table(rx)
    t = [0] * (1 << n_y)
    for i, con in enumerate(constraints):
        for m in range(3):
            f = rho[m] * e[i] % P
            if f:
                for c, w in con[m]:
                    t[w] = (t[w] + c * f) % P
    return t
