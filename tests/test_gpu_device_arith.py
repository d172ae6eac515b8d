"""The field arithmetic the MI355X runs, unit by unit ON THE DEVICE (gkr_devtest_*, csrc/kernels_selftest.hip), against
Python big integers.

The CPU tests of test_host_library.py run the HOST twins of fr32.h; the kernels run the gfx950 inline-asm forms, the
eight-lane MiMC7 code (mimc_lanes.h) and the short reductions of the matrix-core passes, which sumcheck parity checks
only end to end -- on random tables, where a carry or borrow chain hits an exact limb value with probability ~2^-32.
Here every primitive gets (1) crafted edges: limb boundaries, runs of all-ones limbs, Montgomery products whose value
before the final subtraction is p - 1, p or p + 1, the largest inputs each bound allows; (2) for the lane code, the
edge placed in every pair of neighbouring groups of a wave; (3) >= 2^16 random cases, all compared bit for bit
(lazy_reduce_partial32: mod p and below 2^256, which is all it promises)."""

import ctypes
import random

import numpy as np
import pytest

from gkr_amd import Context, GkrError
from gkr_amd import _native as N
from oracle import mimc7
from oracle.field import P

pytestmark = pytest.mark.gpu

R = 1 << 256
RM = R % P                     # Montgomery form of 1
RINV = pow(R, -1, P)
R2 = R * R % P
PINV = pow(P, -1, R)
NRAND = 1 << 16

# op codes of include/gkr_amd.h (the enums' order)
(F_ADD, F_SUB, F_MONT_MUL, F_MUL, F_TO_MONT, F_FROM_MONT, F_MUL_FIXED, F_MUL_FIXED2, F_FOLD_FIXED, F_FOLD_FIXED2) = range(10)
(L_MAC_S, L_MAC_V, L_MAC_SEL, L_MAC_V_HI, L_MAC2_S, L_MAC3_S, L_MAC4_S, L_WSUM4, L_WSUM8, L_ACC_SUM) = range(10)
(RED_FULL, RED_K8, RED_PARTIAL32) = range(3)
(X_MF274, X_CROSS, X_LAZY, X_LAZY_K8, X_PARTIAL32, X_ADD_HI, X_ACC_ADD9, X_ACC_RED9, X_ADD256, X_SUB256, X_COND_SUB) = range(11)
X_IN = [9, 17, 17, 17, 17, 26, 17, 9, 16, 16, 8]
X_OUT = [8, 8, 8, 8, 8, 17, 9, 8, 8, 9, 8]
(N_MONT_MUL, N_ADD3, N_CS_P, N_CS_2P, N_RESOLVE, N_PERM, N_MH1, N_MH2, N_MH3, N_GROUP_SUM) = range(10)


def _enc(vals, limbs=8):
    return np.frombuffer(b"".join(int(v).to_bytes(4 * limbs, "little") for v in vals), dtype=np.uint32).copy()


def _dec(arr, limbs=8):
    b = np.ascontiguousarray(arr, dtype=np.uint32).tobytes()
    w = 4 * limbs
    return [int.from_bytes(b[i:i + w], "little") for i in range(0, len(b), w)]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


@pytest.fixture(scope="module")
def ctx():
    with Context(0) as c:
        yield c


def field(ctx, op, a, b, r=None):
    n = len(a)
    out = np.zeros((2 if op in (F_MUL_FIXED2, F_FOLD_FIXED2) else 1) * n * 8, dtype=np.uint32)
    rc = N.lib().gkr_devtest_field(ctx._h, op, _p(_enc(a)), _p(_enc(b)), _p(_enc(r)) if r is not None else None, ctypes.c_size_t(n), _p(out))
    assert rc == 0, (rc, ctx.last_error() if hasattr(ctx, "last_error") else "")
    return _dec(out)


def lazy(ctx, op, red, a, b, rows, length):
    out = np.zeros(rows * 4 * 8, dtype=np.uint32)
    rc = N.lib().gkr_devtest_lazy(ctx._h, op, red, _p(_enc(a)), _p(_enc(b)) if b is not None else None, ctypes.c_size_t(rows),
                                  ctypes.c_size_t(length), _p(out))
    assert rc == 0, rc
    o = _dec(out)
    return [o[4 * i:4 * i + 4] for i in range(rows)]


def reduce_(ctx, op, xs):
    out = np.zeros(len(xs) * X_OUT[op], dtype=np.uint32)
    rc = N.lib().gkr_devtest_reduce(ctx._h, op, _p(_enc(xs, X_IN[op])), ctypes.c_size_t(len(xs)), _p(out))
    assert rc == 0, rc
    return _dec(out, X_OUT[op])


def lanes(ctx, op, x, y=None, z=None):
    n = len(x) // 8 if op == N_GROUP_SUM else len(x)
    out = np.zeros(len(x) * 8, dtype=np.uint32)
    enc = [_enc(v) if v is not None else None for v in (x, y, z)]
    rc = N.lib().gkr_devtest_lanes(ctx._h, op, _p(enc[0]), _p(enc[1]), _p(enc[2]), ctypes.c_size_t(n), _p(out))
    assert rc == 0, rc
    return _dec(out)


# ---------------------------------------------------------------- inputs
def _edges():
    e = {0, 1, 2, P - 1, P - 2, RM, R2, P >> 1, (P + 1) >> 1}
    for k in range(32, 254):
        e.update(((1 << k) - 1, 1 << k))
    top = P >> 224
    for i in range(7):                          # runs of all-ones limbs i .. j below p
        for j in range(i, 7):
            run = (1 << (32 * (j + 1))) - (1 << (32 * i))
            e.update((run, run | ((top - 1) << 224), run | (top << 224) if (run | (top << 224)) < P else run))
    return sorted(v for v in e if v < P)


EDGES = _edges()


def _final_subtraction_pairs(rng, count=40):
    """(a, b) below p whose Montgomery product a b / 2^256 before its final conditional subtraction is p - 1, p or p + 1:
    a b = t 2^256 - M p with M < 2^256 the product's own reduction multiplier (M = -a b / p mod 2^256)."""
    pairs = []
    while len(pairs) < count:
        t = P + rng.choice((-1, 0, 1))
        b = rng.randrange(P // 2, P)
        m0 = t * R * pow(P, -1, b) % b            # t R - M p = 0 (mod b)
        m = R - b + ((m0 - (R - b)) % b)          # the one such M in [R - b, R)
        if m >= R:
            continue
        num = t * R - m * P
        if num <= 0 or num % b:
            continue
        a = num // b
        if a < P and (a * b + ((-a * b * PINV) % R) * P) == t * R:
            pairs.append((a, b))
    return pairs


def _pairs(rng, n_rand=NRAND):
    sample = EDGES[::3]
    pairs = [(a, b) for a in sample for b in sample]
    pairs += _final_subtraction_pairs(rng)
    pairs += [(rng.randrange(P), rng.randrange(P)) for _ in range(n_rand)]
    pairs += [(rng.choice(EDGES), rng.randrange(P)) for _ in range(4096)]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _pad_waves(vals, fill):
    return vals + [fill] * ((-len(vals)) % 64)


# ---------------------------------------------------------------- fr32.h, one element per thread
@pytest.mark.parametrize("op", [F_ADD, F_SUB, F_MONT_MUL, F_MUL, F_TO_MONT, F_FROM_MONT])
def test_field_ops_match_bigints(ctx, op):
    rng = random.Random(100 + op)
    a, b = _pairs(rng)
    got = field(ctx, op, a, b)
    want = {F_ADD: lambda x, y: (x + y) % P, F_SUB: lambda x, y: (x - y) % P, F_MONT_MUL: lambda x, y: x * y * RINV % P,
            F_MUL: lambda x, y: x * y % P, F_TO_MONT: lambda x, y: x * RM % P, F_FROM_MONT: lambda x, y: x * RINV % P}[op]
    bad = [(hex(x), hex(y)) for x, y, g in zip(a, b, got) if g != want(x, y)]
    assert not bad, (len(bad), bad[:4])


def test_final_subtraction_pairs_are_what_they_claim():
    rng = random.Random(5)
    for a, b in _final_subtraction_pairs(rng, 12):
        t = (a * b + ((-a * b * PINV) % R) * P) >> 256
        assert t in (P - 1, P, P + 1) and a < P and b < P


@pytest.mark.parametrize("op", [F_MUL_FIXED, F_MUL_FIXED2, F_FOLD_FIXED, F_FOLD_FIXED2])
def test_fixed_multiplier_ops_match_bigints(ctx, op):
    """The fold kernels' fixed-multiplier product: the table built on the device by make_fixed_mul from one challenge per
    wave (edges, then random), the single and the paired forms."""
    rng = random.Random(200 + op)
    a, b = _pairs(rng)
    a, b = _pad_waves(a, 0), _pad_waves(b, P - 1)
    waves = len(a) // 64
    rs = [EDGES[w % len(EDGES)] if w < 2 * len(EDGES) else rng.randrange(P) for w in range(waves)]
    got = field(ctx, op, a, b, rs)
    n = len(a)
    bad = []
    for i in range(n):
        r = rs[i // 64]
        if op == F_MUL_FIXED:
            w = [a[i] * r % P]
        elif op == F_MUL_FIXED2:
            w = [a[i] * r % P, b[i] * r % P]
        elif op == F_FOLD_FIXED:
            w = [(a[i] + r * (b[i] - a[i])) % P]
        else:
            w = [(a[i] + r * (b[i] - a[i])) % P, (b[i] + r * (a[i] - b[i])) % P]
        g = [got[i]] + ([got[n + i]] if len(w) == 2 else [])
        if g != w:
            bad.append((i, hex(a[i]), hex(b[i]), hex(r)))
    assert not bad, (len(bad), bad[:4])


def test_device_and_host_twins_agree(ctx):
    """The gfx950 forms and the host forms (gkr_selftest_mul / _fold / _dot) on the same inputs."""
    lib = N.lib()
    rng = random.Random(300)
    a, b = _pairs(rng, 200)
    a, b = a[-600:], b[-600:]
    dev = field(ctx, F_MUL, a, b)
    for x, y, d in zip(a, b, dev):
        o = np.zeros(8, dtype=np.uint32)
        assert lib.gkr_selftest_mul(_p(_enc([x])), _p(_enc([y])), _p(o)) == 0
        assert _dec(o)[0] == d
    a64, b64 = _pad_waves(a[:128], 1), _pad_waves(b[:128], 2)
    rs = [P - 1, rng.randrange(P)]
    dev = field(ctx, F_FOLD_FIXED, a64, b64, rs)
    for i in range(128):
        o = np.zeros(8, dtype=np.uint32)
        assert lib.gkr_selftest_fold(_p(_enc([a64[i]])), _p(_enc([b64[i]])), _p(_enc([rs[i // 64]])), _p(o)) == 0
        assert _dec(o)[0] == dev[i]
    rows, length = 64, 8
    av = [rng.choice(EDGES) if rng.random() < 0.3 else rng.randrange(P) for _ in range(rows * length)]
    bv = [rng.choice(EDGES) if rng.random() < 0.3 else rng.randrange(P) for _ in range(rows * length)]
    got = lazy(ctx, L_MAC_V, RED_FULL, av, [x * RM % P for x in bv], rows, length)
    for r in range(rows):
        o = np.zeros(8, dtype=np.uint32)
        assert lib.gkr_selftest_dot(_p(_enc(av[r * length:(r + 1) * length])), _p(_enc(bv[r * length:(r + 1) * length])),
                                    ctypes.c_size_t(length), _p(o)) == 0
        assert _dec(o)[0] == got[r][0]


# ---------------------------------------------------------------- lazy dot products
def _operands(rng, n):
    return [rng.choice(EDGES) if rng.random() < 0.25 else (P - 1 if rng.random() < 0.1 else rng.randrange(P)) for _ in range(n)]


LAZY_CASES = [(L_MAC_S, RED_FULL, 16), (L_MAC_S, RED_K8, 8), (L_MAC_S, RED_PARTIAL32, 32), (L_MAC_V, RED_FULL, 3), (L_MAC_V, RED_K8, 8),
              (L_MAC_V, RED_PARTIAL32, 32), (L_MAC_SEL, RED_FULL, 7), (L_MAC_SEL, RED_K8, 8), (L_MAC_V_HI, RED_FULL, 9),
              (L_MAC_V_HI, RED_PARTIAL32, 16), (L_MAC2_S, RED_K8, 8), (L_MAC2_S, RED_FULL, 5), (L_MAC3_S, RED_FULL, 6),
              (L_MAC3_S, RED_PARTIAL32, 32), (L_MAC4_S, RED_K8, 8), (L_MAC4_S, RED_FULL, 4), (L_WSUM4, RED_K8, 4),
              (L_WSUM8, RED_K8, 8), (L_WSUM8, RED_PARTIAL32, 8), (L_ACC_SUM, RED_FULL, 33), (L_MAC_V, RED_FULL, 600)]


@pytest.mark.parametrize("op,red,length", LAZY_CASES, ids=lambda v: str(v))
def test_lazy_dot_products_match_bigints(ctx, op, red, length):
    """One dot product per thread through the kernels' unreduced 544-bit accumulators, every accumulate form and every
    reduction (lazy_reduce_k8 at its eight products, lazy_reduce_partial32 at its 32 terms); all operands p - 1 in the
    first rows (every column at its largest), edges and random after."""
    rng = random.Random(400 + 17 * op + red + length)
    rows = max(64, min(NRAND // length, 8192)) if length < 100 else 64
    uniform = op in (L_MAC_S, L_MAC2_S, L_MAC3_S, L_MAC4_S, L_WSUM4, L_WSUM8)
    waves = (rows + 63) // 64
    a = _operands(rng, rows * length)
    b = None if op == L_ACC_SUM else _operands(rng, (waves if uniform else rows) * length)
    a[:2 * length] = [P - 1] * (2 * length)
    if b is not None:
        b[:length] = [P - 1] * length
    got = lazy(ctx, op, red, a, b, rows, length)
    chains = {L_MAC2_S: 2, L_MAC3_S: 3, L_MAC4_S: 4}.get(op, 1)
    bad = []
    for r in range(rows):
        ar = a[r * length:(r + 1) * length]
        if op == L_ACC_SUM:
            want = [sum(ar) % P, 0, 0, 0]
        else:
            br = b[(r // 64 if uniform else r) * length:][:length]
            if op == L_MAC_SEL:
                sa = sum(x * y for t, (x, y) in enumerate(zip(ar, br)) if (r + t) % 3 != 0)
                sb = sum(x * y for t, (x, y) in enumerate(zip(ar, br)) if (r + t) % 3 == 0)
                want = [sa * RINV % P, sb * RINV % P, 0, 0]
            elif op == L_MAC_V_HI:
                s = sum(x * y for x, y in zip(ar, br)) + sum(x << 256 for t, x in enumerate(ar) if (r + t) & 1)
                want = [s * RINV % P, 0, 0, 0]
            else:
                want = [sum(ar[t] * br[(t + c) % length] for t in range(length)) * RINV % P if c < chains else 0 for c in range(4)]
        g = got[r]
        if red == RED_PARTIAL32 and op != L_ACC_SUM:
            ok = all(v < R for v in g) and [v % P for v in g] == want
        else:
            ok = g == want
        if not ok:
            bad.append(r)
    assert not bad, (len(bad), bad[:4])


# ---------------------------------------------------------------- raw-limb reductions and carry chains
def _mf274_cases(rng):
    top = (1 << 274) - 1
    qmax = top // P
    qs = [0, 1, 2, 3, qmax, qmax - 1, qmax // 2] + [1 << k for k in range(0, qmax.bit_length())] + [rng.randrange(qmax) for _ in range(200)]
    xs = [q * P + d for q in qs for d in (0, 1, P - 1, P - 2, P // 2)]
    xs += [top, top - 1, top - P, 0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P, (1 << 256) - 1, 1 << 256, (1 << 273)]
    xs += [rng.randrange(1 << 274) for _ in range(NRAND)] + [rng.randrange(P) for _ in range(1024)]
    return [x for x in xs if 0 <= x <= top]


def _check(pairs):
    bad = [(hex(x), hex(g), hex(w)) for x, g, w in pairs if g != w]
    assert not bad, (len(bad), bad[:3])


def test_mf_reduce_274(ctx):
    xs = _mf274_cases(random.Random(500))
    _check(zip(xs, reduce_(ctx, X_MF274, xs), [x % P for x in xs]))


def test_cross_reduce(ctx):
    """The cross pass's block reduction at the largest sum its blocks produce (2048 products of (p - 1)^2) and below."""
    rng = random.Random(501)
    big = 2048 * (P - 1) ** 2
    xs = [big, big - 1, big - P, 2048 * P * P - 1 if 2048 * P * P - 1 < (1 << 519) else big, (1 << 519) - 1, 0, 1, P, P * P, (P - 1) ** 2]
    xs += [k * (P - 1) ** 2 + d for k in (1, 2, 8, 32, 1024, 2047) for d in (0, 1, P - 1)]
    xs += [sum(rng.randrange(P) * rng.randrange(P) for _ in range(4)) * rng.randrange(1, 512) for _ in range(1024)]
    xs += [rng.randrange(big) for _ in range(NRAND)]
    _check(zip(xs, reduce_(ctx, X_CROSS, xs), [x * RINV % P for x in xs]))


def test_lazy_reductions(ctx):
    rng = random.Random(502)
    full = [(1 << 544) - 1, (1 << 544) - (1 << 256), 0, 1, P, (P - 1) ** 2, ((1 << 288) - 1) << 256]
    full += [rng.randrange(1 << 544) for _ in range(NRAND)] + [rng.randrange(1 << 300) for _ in range(4096)]
    _check(zip(full, reduce_(ctx, X_LAZY, full), [x * RINV % P for x in full]))
    b8 = 8 * P * P
    k8 = [b8 - 1, 8 * (P - 1) ** 2, b8 - P, 0, 1, (P - 1) ** 2, 7 * (P - 1) ** 2 + (P - 1) * (P - 2)]
    k8 += [rng.randrange(b8) for _ in range(NRAND)] + [sum(rng.randrange(P) * rng.randrange(P) for _ in range(8)) for _ in range(2048)]
    _check(zip(k8, reduce_(ctx, X_LAZY_K8, k8), [x * RINV % P for x in k8]))
    b32 = 32 * P << 256
    p32 = [b32 - 1, b32 - (1 << 256), (32 * P - 1) << 256, 0, 1, 32 * (P - 1) ** 2, (P - 1) << 256, ((1 << 256) - 1) + ((32 * P - 1) << 256)]
    p32 += [rng.randrange(b32) for _ in range(NRAND)]
    got = reduce_(ctx, X_PARTIAL32, p32)
    bad = [hex(x) for x, g in zip(p32, got) if g >= R or g % P != x * RINV % P]
    assert not bad, (len(bad), bad[:3])


def test_carry_chains_of_the_accumulators(ctx):
    """lazy_add_hi's and acc_add_fr<9>'s padded carry chains (inline asm) with a carry through every limb, and add256 /
    sub256 / cond_sub_mod with all-ones and all-zero runs."""
    rng = random.Random(503)
    ones = (1 << 544) - 1
    accs = [ones - ((1 << 256) * k) for k in (0, 1, 2)] + [((1 << 288) - 1) << 256, ((1 << 256) - 1) << 256, 0, ones >> 1]
    accs += [(((1 << (32 * j)) - 1) << 256) | rng.randrange(1 << 256) for j in range(1, 10)]
    xs = [P - 1, 1, 0, (1 << 32) - 1, (P >> 32) << 32]
    cases = [(acc, x, on) for acc in accs for x in xs for on in (0, 1)]
    cases += [(rng.randrange(1 << 544), rng.randrange(P), rng.randrange(2)) for _ in range(NRAND)]
    enc = [acc | (x << 544) | (on << 800) for acc, x, on in cases]
    got = reduce_(ctx, X_ADD_HI, enc)
    _check(zip(enc, got, [(acc + (x << 256) * on) % (1 << 544) for acc, x, on in cases]))
    acc9 = [(1 << 288) - 1, (1 << 288) - P, ((1 << 32) - 1) << 256, (1 << 256) - 1, 0] + [(1 << 288) - (1 << (32 * j)) for j in range(9)]
    cases = [(a, x) for a in acc9 for x in xs] + [(rng.randrange(1 << 288), rng.randrange(P)) for _ in range(NRAND)]
    enc = [a | (x << 288) for a, x in cases]
    _check(zip(enc, reduce_(ctx, X_ACC_ADD9, enc), [(a + x) % (1 << 288) for a, x in cases]))
    r9 = acc9 + [rng.randrange(1 << 288) for _ in range(NRAND)]
    _check(zip(r9, reduce_(ctx, X_ACC_RED9, r9), [x % P for x in r9]))
    vals = [0, 1, (1 << 256) - 1, (1 << 255), P, P - 1, 2 * P - 1] + [(1 << (32 * j)) - 1 for j in range(1, 8)] + [(1 << 256) - (1 << (32 * j)) for j in range(1, 8)]
    pairs = [(a, b) for a in vals for b in vals] + [(rng.randrange(R), rng.randrange(R)) for _ in range(NRAND)]
    enc = [a | (b << 256) for a, b in pairs]
    _check(zip(enc, reduce_(ctx, X_ADD256, enc), [(a + b) % R for a, b in pairs]))
    _check(zip(enc, reduce_(ctx, X_SUB256, enc), [((a - b) % R) | ((0xFFFFFFFF if a < b else 0) << 256) for a, b in pairs]))
    cs = [0, 1, P - 1, P, P + 1, 2 * P - 1] + [v for v in EDGES] + [v + P for v in EDGES if v + P < 2 * P] + [rng.randrange(2 * P) for _ in range(NRAND)]
    _check(zip(cs, reduce_(ctx, X_COND_SUB, cs), [x % P for x in cs]))


def test_out_of_bound_inputs_are_rejected(ctx):
    lib = N.lib()
    out = np.zeros(64, dtype=np.uint32)
    for op, x in ((X_MF274, 1 << 274), (X_CROSS, 1 << 519), (X_LAZY_K8, 8 * P * P), (X_PARTIAL32, 32 * P << 256), (X_COND_SUB, 2 * P)):
        assert lib.gkr_devtest_reduce(ctx._h, op, _p(_enc([x], X_IN[op])), ctypes.c_size_t(1), _p(out)) == N.GKR_ERR_INVALID
    assert lib.gkr_devtest_field(ctx._h, F_ADD, _p(_enc([P])), _p(_enc([0])), None, ctypes.c_size_t(1), _p(out)) == N.GKR_ERR_INVALID
    assert lib.gkr_devtest_lanes(ctx._h, N_MONT_MUL, _p(_enc([3 * P])), _p(_enc([1])), None, ctypes.c_size_t(1), _p(out)) == N.GKR_ERR_INVALID
    assert lib.gkr_devtest_lanes(ctx._h, N_ADD3, _p(_enc([R - 1])), _p(_enc([1])), _p(_enc([0])), ctypes.c_size_t(1), _p(out)) == N.GKR_ERR_INVALID
    big = np.zeros(64 * 8, dtype=np.uint32)
    assert lib.gkr_devtest_lazy(ctx._h, L_MAC_V, RED_K8, _p(_enc([1] * 9)), _p(_enc([1] * 9)), ctypes.c_size_t(1), ctypes.c_size_t(9), _p(big)) == N.GKR_ERR_INVALID


# ---------------------------------------------------------------- the eight-lane MiMC7 code
def l_mont(a, b):
    return (a * b + ((-a * b * PINV) % R) * P) >> 256


def l_cs(x, m):
    return x - m if x >= m else x


CTS_M = [c * RM % P for c in mimc7.CTS]


def l_perm(x, k):
    h = 0
    for i in range(mimc7.NROUNDS):
        t = l_cs(x + k if i == 0 else h + k + CTS_M[i], 2 * P)
        t2 = l_mont(t, t)
        t4 = l_mont(t2, t2)
        t6 = l_mont(t4, t2)
        h = l_mont(t6, t)
    return l_cs(h + k, 2 * P)


def l_multi_hash(arr):
    r = 0
    for e in arr:
        a = l_cs(l_mont(e, R2), P)
        h = l_perm(a, r)
        r = l_cs(l_cs(r + a + h, 2 * P), P)
    return l_cs(l_mont(r, 1), P)


@pytest.mark.parametrize("which", [N_CS_P, N_CS_2P])
def test_lanes_cond_sub_keeps_borrows_in_their_group(ctx, which):
    """A borrow that runs through group g's top lane (top limb equal to m's, x < m) next to group g + 1 at, just above or
    just below m -- for g = 0 .. 6, across the 16-lane row boundary (1 -> 2, 3 -> 4, 5 -> 6) too; both sides of m on
    both sides; then a ragged last wave and random waves."""
    m = P if which == N_CS_P else 2 * P
    rng = random.Random(600 + which)
    top = (m >> 224) << 224
    xs = []
    for g in range(7):
        for victim in (m, m + 1, m - 1, m + 12345, m + (1 << 224), top + (1 << 224) - 1, top | ((1 << 224) - 1)):
            for left in (top | 5, top, m - 1, top | ((m & ((1 << 224) - 1)) - 1)):
                wave = [rng.randrange(3 * P) for _ in range(8)]
                wave[g], wave[g + 1] = left, victim
                xs += wave
                wave = list(wave)
                wave[g], wave[g + 1] = victim, left   # the other order: the sensitive group below
                xs += wave
    vals = [m, m - 1, m + 1, top, top | 5, top + (1 << 224) - 1, R - 1, 0]
    xs += [rng.choice(vals) if rng.random() < 0.5 else rng.randrange(R) for _ in range(NRAND)]
    xs += [top | 5, m + 7, top, m, m - 1]   # ragged last wave (five groups)
    got = lanes(ctx, which, xs)
    bad = [(i, hex(x), hex(g)) for i, (x, g) in enumerate(zip(xs, got)) if g != l_cs(x, m)]
    assert not bad, (len(bad), bad[:4])


def test_lanes_add3_and_resolve_carries(ctx):
    """Sums whose carries run through all-ones limbs inside a group, beside groups that carry; deferred per-lane carries
    (resolve_carries' own input) with runs of all-ones limbs above them."""
    rng = random.Random(610)
    xs, ys, zs = [], [], []
    for g in range(8):
        for start in range(8):
            for end in range(start, 7):
                run = (1 << (32 * (end + 1))) - (1 << (32 * start))
                for _ in range(2):
                    wave = [(rng.randrange(1 << 250), rng.randrange(1 << 250), rng.randrange(1 << 250)) for _ in range(8)]
                    low = rng.randrange(1 << (32 * start)) if start else 0
                    wave[g] = (run, (1 << (32 * start)) - low if start else 1, low)   # the carry into `start` walks to `end`
                    if g < 7:
                        wave[g + 1] = ((1 << 32) - 1, 1, 0)
                    for x, y, z in wave:
                        xs.append(x), ys.append(y), zs.append(z)
    for _ in range(NRAND):
        x, y = rng.randrange(1 << 255), rng.randrange(1 << 254)
        xs.append(x), ys.append(y), zs.append(rng.randrange(R - x - y))
    got = lanes(ctx, N_ADD3, xs, ys, zs)
    bad = [i for i, (x, y, z, g) in enumerate(zip(xs, ys, zs, got)) if g != x + y + z]
    assert not bad, (len(bad), bad[:4])
    # resolve_carries(limb + 2^32 carry): the carry of lane j - 1 arriving at a run of all-ones limbs j .. end
    lim, car, want = [], [], []
    for start in range(1, 8):
        for end in range(start - 1, 7):
            for _ in range(64):
                limbs = [rng.randrange(1 << 32) for _ in range(7)] + [rng.randrange(1 << 30)]
                carries = [rng.randrange(4) for _ in range(7)] + [0]
                for j in range(start, end + 1):
                    limbs[j] = (1 << 32) - 1
                carries[start - 1] = 1 + rng.randrange(3)
                x = sum(v << (32 * j) for j, v in enumerate(limbs))
                y = sum(v << (32 * j) for j, v in enumerate(carries))
                total = x + (y << 32)
                if total < R:
                    lim.append(x), car.append(y), want.append(total)
    got = lanes(ctx, N_RESOLVE, lim, car)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (len(bad), bad[:4])


def test_lanes_mont_mul(ctx):
    """The lanes' operand-scanning product at the bound (operands up to 3p - 1) and random: its exact representative."""
    rng = random.Random(620)
    e = [0, 1, 2, P - 1, P, P + 1, 2 * P - 1, 2 * P, 3 * P - 1, 3 * P - 2, RM, R2] + [v for v in EDGES[::7]]
    xs = [a for a in e for b in e] + [rng.randrange(3 * P) for _ in range(NRAND)]
    ys = [b for a in e for b in e] + [rng.randrange(3 * P) for _ in range(NRAND)]
    xs += [7] * 3
    ys += [3 * P - 1] * 3   # ragged last wave
    got = lanes(ctx, N_MONT_MUL, xs, ys)
    bad = [(hex(x), hex(y)) for x, y, g in zip(xs, ys, got) if g != l_mont(x, y)]
    assert not bad, (len(bad), bad[:4])
    assert all(g < 2.7 * P for g in got)


def test_lanes_permutation_and_multi_hash(ctx):
    """hash(x, k) of the lane code, bit for bit against a model of its representatives and mod p against mimc7; multi_hash of
    one to three elements against mimc7.multi_hash -- a few hundred hashes (165 us each), a ragged last wave."""
    rng = random.Random(630)
    e = [0, 1, P - 1, P - 2, RM]
    pairs = [(a, b) for a in e for b in e] + [(rng.randrange(P), rng.randrange(P)) for _ in range(163)]
    xs, ks = [a * RM % P for a, _ in pairs], [b * RM % P for _, b in pairs]
    got = lanes(ctx, N_PERM, xs, ks)
    for (a, b), x, k, g in zip(pairs, xs, ks, got):
        assert g == l_perm(x, k), (hex(a), hex(b))
        assert g % P == mimc7.mimc7_hash(a, b) * RM % P
    for n_el, op in ((1, N_MH1), (2, N_MH2), (3, N_MH3)):
        cols = [[rng.choice(e) if rng.random() < 0.3 else rng.randrange(P) for _ in range(45)] for _ in range(3)]
        got = lanes(ctx, op, cols[0], cols[1] if n_el > 1 else None, cols[2] if n_el > 2 else None)
        for i, g in enumerate(got):
            arr = [cols[c][i] for c in range(n_el)]
            assert g == mimc7.multi_hash(arr) == l_multi_hash(arr), (n_el, i)


def test_lanes_group_sum(ctx):
    rng = random.Random(640)
    n = NRAND // 8 + 3   # ragged last wave
    vals = [rng.choice(EDGES) if rng.random() < 0.3 else rng.randrange(P) for _ in range(8 * n)]
    vals[:8] = [P - 1] * 8
    got = lanes(ctx, N_GROUP_SUM, vals)
    for i in range(n):
        s = sum(vals[8 * i:8 * i + 8]) % P
        assert got[8 * i:8 * i + 8] == [s] * 8, i
