"""R1CS for the tests of the oracle's R1CS tables (tests/test_oracle_r1cs_c.py) and of the device's at multi-block sizes
(tests/test_gpu_r1cs_sizes.py).

Small systems as Python lists, the form R1cs.build and the integer models take: coeff, random_constraints, flatten.

Large systems as numpy arrays -- a million constraints as Python lists cost more than the kernels under test: generate() gives the
flat form gkr_r1cs_build reads (counts[3 * n_constraints], wires[], coefficient limbs), build_r1cs() hands it to the library as it
is, and witness() makes a satisfying witness with the C oracle alone (ogkr_r1cs_rows, ogkr_fr_mul_many, ogkr_fr_add_many).

The construction, with n_in input wires, K = n_wires - n_in output wires and base(i) = i mod (K - 1) for every constraint but the
last, whose base is K - 1 and belongs to it alone:

  wire 0 is the constant 1, wires 1 .. n_in - 1 are inputs;
  A_i = s_i * Abase_base(i), B_i = Bbase_base(i), both combinations over the wires below n_in with wire 0 in every one of them;
  C_i = [(s_i, 0), (s_i, n_in + base(i))]; s_i is 1 or r - 1 mostly, 2 or random now and then, r - 2 in one run of 600 constraints;
  wire n_in + k = (Abase_k . w)(Bbase_k . w) - 1, so A_i w * B_i w = s_i (w[n_in + k] + 1) = C_i w.

So wire 0 has a record in every constraint of A, B and C (n_constraints / 2048 segments per matrix at the default segment length),
base coefficients are 1 or r - 1 nine times in ten (the addition side) beside 2, r - 2, 0 and random ones, with one run of bases
whose coefficients are all 2 or r - 2; long rows of 33, 64, 65, 129 and 4097 terms (and rows of exactly 32, which are not long)
sit on bases scattered over the whole range, the last constraint's included, more of them in A than in B and none in C; K sets
n_wires independently of n_constraints (K - 1 < n_constraints: an output wire is read by several rows; K > n_constraints: the
last output wires by none)."""

import ctypes

import numpy as np

from gkr_amd import _native as N
from gkr_amd.convert import R1cs
from oracle import cdense
from oracle.field import P

LONG = N.GKR_R1CS_LONG_ROW
SEG = N.GKR_R1CS_COL_SEGMENT
NO_BAD = 0xFFFFFFFF
COEFF_MIX = ["ones", "minus_ones", "random", "minus_one_and_two"]
LONG_LENGTHS = [LONG + 1, 64, 65, LONG, 129]                    # terms of a long base row, wire 0 included (LONG itself: not long)
MANY = 4097                                                      # the several-thousand-term rows


# ---- small systems as lists -------------------------------------------------------------------------------------------------------------
def coeff(kind, rng):
    if kind == "ones":
        return 1
    if kind == "minus_ones":
        return P - 1
    if kind == "random":
        return rng.randrange(1, P)
    return (P - 1, 2)[rng.randrange(2)]


def random_constraints(rng, n_constraints, n_wires, kind, longest=4, zeros=False):
    """Rows of 0 .. longest terms (a wire may repeat); zeros: about one coefficient in eight is 0."""
    def c():
        return 0 if zeros and rng.randrange(8) == 0 else coeff(kind, rng)
    return [tuple([(c(), rng.randrange(n_wires)) for _ in range(rng.randrange(longest + 1))] for _ in range(3)) for _ in range(n_constraints)]


def flatten(constraints):
    """[(A, B, C)] of [(coefficient, wire)] -> (counts, wires, coefficient limbs), R1cs.build's flattening."""
    counts = np.array([len(lc) for con in constraints for lc in con], dtype=np.uint32)
    wires = np.array([w for con in constraints for lc in con for _, w in lc], dtype=np.uint32)
    coeffs = [c for con in constraints for lc in con for c, _ in lc]
    return counts, wires, cdense.to_limbs(coeffs) if coeffs else np.zeros((0, 4), dtype=np.uint64)


def constraints_of(counts, wires, coeffs, first):
    """flatten the other way round, for the first `first` constraints."""
    out, pos = [], 0
    for i in range(first):
        con = []
        for m in range(3):
            k = int(counts[3 * i + m])
            raw = np.ascontiguousarray(coeffs[pos:pos + k]).tobytes()              # (little-endian limbs: the value's 32 bytes)
            con.append([(int.from_bytes(raw[32 * t:32 * t + 32], "little"), int(wires[pos + t])) for t in range(k)])
            pos += k
        out.append(tuple(con))
    return out


# ---- large systems as arrays ------------------------------------------------------------------------------------------------------------
def limbs(value):
    return cdense.to_limbs([value])[0]


def _segments(starts, lens):
    """The indices starts[i] .. starts[i] + lens[i] - 1 of every i, one after the other."""
    lens = lens.astype(np.int64)
    return np.repeat(starts.astype(np.int64) - (np.cumsum(lens) - lens), lens) + np.arange(int(lens.sum()), dtype=np.int64)


def _coefficients(rng, count, seed, weights):
    """`count` coefficient limbs drawn with `weights` from 1, r - 1, 2, r - 2, 0, random; -> (limbs, kinds)."""
    consts = cdense.to_limbs([1, P - 1, 2, P - 2, 0])
    kinds = rng.choice(6, size=count, p=weights)
    out = cdense.fill_table(count, seed)
    fixed = kinds < 5
    out[fixed] = consts[kinds[fixed]]
    return out, kinds


class System:
    """generate()'s result: the flat form (counts, wires, coeffs), the base rows it was made from and where its records lie."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def flat(self):
        return self.counts, self.wires, self.coeffs

    def record(self, i, m, t=0):
        """The index of record t of constraint i in matrix m."""
        assert t < int(self.counts[3 * i + m])
        return int(self.offset[i]) + int(self.counts[3 * i:3 * i + m].sum()) + t

    def nonzero_terms(self):
        """(n_constraints, 3): the terms the library keeps per row (a zero coefficient's record is dropped)."""
        matrix = np.repeat(np.arange(3 * self.n_constraints), self.counts)
        return np.bincount(matrix[self.coeffs.any(axis=1)], minlength=3 * self.n_constraints).reshape(-1, 3)

    def long_rows(self):
        """Per matrix, the rows with more than GKR_R1CS_LONG_ROW terms, ascending."""
        nz = self.nonzero_terms()
        return [np.flatnonzero(nz[:, m] > LONG) for m in range(3)]

    def long_columns(self):
        """Per matrix, the number of columns with more than GKR_R1CS_LONG_COL kept records."""
        matrix = np.repeat(np.tile(np.arange(3), self.n_constraints), self.counts)
        keep = self.coeffs.any(axis=1)
        return [int((np.bincount(self.wires[keep & (matrix == m)], minlength=1) > N.GKR_R1CS_LONG_COL).sum()) for m in range(3)]

    def column_lengths(self, wire):
        """Per matrix, the kept records of one wire's column."""
        matrix = np.repeat(np.tile(np.arange(3), self.n_constraints), self.counts)
        keep = (self.wires == wire) & self.coeffs.any(axis=1)
        return np.bincount(matrix[keep], minlength=3).tolist()


def generate(n_constraints, n_wires, seed, n_in=1024):
    K = n_wires - n_in
    assert K >= 64 and n_constraints >= 2 * MANY
    rng = np.random.default_rng(seed)
    base_of = np.arange(n_constraints, dtype=np.int64) % (K - 1)
    base_of[-1] = K - 1
    used = min(K - 1, n_constraints - 1)                         # the bases below this one have a row (base K - 1 has the last)
    # -- the base rows: wire 0 and 1 .. 3 (A), 0 .. 2 (B) inputs; the long ones
    len_a = 1 + rng.integers(1, 4, size=K)
    len_b = 1 + rng.integers(0, 3, size=K)
    long_a = np.unique(np.concatenate([rng.integers(0, used, size=150), [0, used - 1]]))
    long_b = np.unique(rng.integers(0, used, size=60))
    len_a[long_a] = np.resize(LONG_LENGTHS, len(long_a))
    len_b[long_b] = np.resize(LONG_LENGTHS[::-1], len(long_b))
    len_a[K - 1] = MANY                                          # the last constraint's own base
    len_a[long_a[len(long_a) // 2]] = MANY
    len_b[long_b[len(long_b) // 3]] = MANY - 1000
    ptr_a, ptr_b = (np.concatenate([[0], np.cumsum(l)]).astype(np.int64) for l in (len_a, len_b))
    weights = [0.45, 0.45, 0.03, 0.03, 0.01, 0.03]
    wires_a, wires_b = (rng.integers(1, n_in, size=int(p[-1])).astype(np.uint32) for p in (ptr_a, ptr_b))
    coef_a, kinds_a = _coefficients(rng, int(ptr_a[-1]), seed + 1, weights)
    coef_b, kinds_b = _coefficients(rng, int(ptr_b[-1]), seed + 2, weights)
    run = slice(int(ptr_a[used // 2]), int(ptr_a[min(used // 2 + 300, used)]))          # a run of bases on the product side
    coef_a[run] = cdense.to_limbs([2, P - 2])[rng.integers(0, 2, size=run.stop - run.start)]
    for k in long_a.tolist() + [K - 1]:                          # (a zero coefficient would shorten a long row)
        at = slice(int(ptr_a[k]), int(ptr_a[k + 1]))
        coef_a[at][kinds_a[at] == 4] = limbs(P - 2)
    for k in long_b.tolist():
        at = slice(int(ptr_b[k]), int(ptr_b[k + 1]))
        coef_b[at][kinds_b[at] == 4] = limbs(2)
    # wire 0: the first record of a B row, the first or the last of an A row, with 1 or r - 1
    zero_a = np.where(np.arange(K) % 2 == 0, ptr_a[:-1], ptr_a[1:] - 1)
    wires_a[zero_a], wires_b[ptr_b[:-1]] = 0, 0
    coef_a[zero_a] = cdense.to_limbs([1, P - 1])[rng.integers(0, 2, size=K)]
    coef_b[ptr_b[:-1]] = cdense.to_limbs([1, P - 1])[rng.integers(0, 2, size=K)]
    # -- s_i
    s, _ = _coefficients(rng, n_constraints, seed + 3, [0.47, 0.47, 0.03, 0.0, 0.0, 0.03])
    s[n_constraints // 3:n_constraints // 3 + 600] = limbs(P - 2)
    # -- the constraints
    la, lb = len_a[base_of], len_b[base_of]
    total = la + lb + 2
    offset = np.cumsum(total) - total
    counts = np.stack([la, lb, np.full(n_constraints, 2)], axis=1).astype(np.uint32).reshape(-1)
    records = int(total.sum())
    wires, coeffs = np.zeros(records, dtype=np.uint32), np.zeros((records, 4), dtype=np.uint64)
    dst, src = _segments(offset, la), _segments(ptr_a[base_of], la)
    wires[dst] = wires_a[src]
    coeffs[dst] = cdense.fr_mul_many(coef_a[src], s[np.repeat(np.arange(n_constraints), la)])
    dst, src = _segments(offset + la, lb), _segments(ptr_b[base_of], lb)
    wires[dst] = wires_b[src]
    coeffs[dst] = coef_b[src]
    at = offset + la + lb
    wires[at], wires[at + 1] = 0, (n_in + base_of).astype(np.uint32)
    coeffs[at], coeffs[at + 1] = s, s
    return System(n_constraints=n_constraints, n_wires=n_wires, n_in=n_in, K=K, base_of=base_of, offset=offset, counts=counts, wires=wires,
                  coeffs=coeffs, base=((len_a, wires_a, coef_a), (len_b, wires_b, coef_b)), long_bases=(long_a, long_b))


def witness(system, kind, seed):
    """A witness (n_wires, 4) that satisfies the system: inputs of `kind` ("random", "all_max": every input r - 1, "bits": 0 or 1,
    "small": below 2^16), the output wires from the rows oracle on the base rows and a Hadamard product."""
    n_in, K = system.n_in, system.K
    w = cdense.fill_table(n_in, seed)
    if kind == "all_max":
        w[:] = limbs(P - 1)
    elif kind in ("bits", "small"):
        w[:, 1:] = 0
        w[:, 0] &= np.uint64(1 if kind == "bits" else 0xFFFF)
    else:
        assert kind == "random", kind
    w[0] = limbs(1)
    n = max(0, (K - 1).bit_length())
    sides = []
    for lens, wires, coeffs in system.base:                      # base rows k as matrix A of a system of K constraints over the inputs
        counts = np.stack([lens, np.zeros_like(lens), np.zeros_like(lens)], axis=1).reshape(-1)
        sides.append(cdense.r1cs_rows_raw(counts, wires, coeffs, n_in, w, n)[0, :K])
    out = cdense.fr_add_many(cdense.fr_mul_many(sides[0], sides[1]), np.tile(limbs(P - 1), (K, 1)))
    return np.concatenate([w, out])


def bad_rows(rows, n_constraints):
    """The constraints with Az * Bz != Cz in the rows oracle's tables (3, 2^n, 4), ascending."""
    return np.flatnonzero((cdense.fr_mul_many(rows[0, :n_constraints], rows[1, :n_constraints]) != rows[2, :n_constraints]).any(axis=1))


def first_bad(rows, n_constraints):
    """The lowest of them, or NO_BAD."""
    bad = bad_rows(rows, n_constraints)
    return int(bad[0]) if len(bad) else NO_BAD


def build_r1cs(counts, wires, coeffs, n_wires):
    """gkr_r1cs_build on the arrays as they are -> R1cs (the library copies them)."""
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    wires = np.ascontiguousarray(wires, dtype=np.uint32)
    coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64)
    assert counts.size % 3 == 0 and int(counts.sum(dtype=np.uint64)) == wires.size == coeffs.shape[0]
    h = ctypes.c_void_p()
    rc = N.lib().gkr_r1cs_build(ctypes.c_uint32(n_wires), ctypes.c_uint32(1), ctypes.c_uint32(1), ctypes.c_uint32(1), ctypes.c_size_t(counts.size // 3),
                                counts.ctypes.data_as(ctypes.c_void_p), wires.ctypes.data_as(ctypes.c_void_p),
                                coeffs.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h))
    assert rc == 0, ("gkr_r1cs_build", rc)
    return R1cs(h)
