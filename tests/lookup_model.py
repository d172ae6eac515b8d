"""Integer model of the lookup argument (include/gkr_amd.h, gkr_lookup*), written from the protocol on fraction_sum_model and
independently of gkr_amd/verifier.py.

  h        the slot of a value among 2^s slots: over its four 64-bit limbs, least significant first, modulo 2^64:
           x = 0x9E3779B97F4A7C15; per limb x = (x ^ v_i) * 0xFF51AFD7ED558CCD, x ^= x >> 32; x *= 0xC4CEB9FE1A85EC53; x ^= x >> 29;
           the s most significant bits of x
  M        M[j] = #{i: W[i] = T[j]} if j is the lowest index with T's value T[j], else 0
  pair     L = max(n_w, n_t) + 1;  (N, D)[i] = (1, alpha - W[i]), i < 2^n_w, then (0, 1) up to 2^(L-1);
           (N, D)[2^(L-1) + j] = (-M[j], alpha - T[j]), j < 2^n_t, then (0, 1)
  proof    the fractional sum's proof of the pair, n = L
  verdict  the fractional sum's, without claimed sums, and LOOKUP at (0, 0) for a head whose P is not 0 -- where FRACTION_SUM
           stands in that order: after SHAPE, NON_CANONICAL, ZERO_DENOMINATOR, before the layers and EVALUATION."""

from fraction_sum_model import NON_CANONICAL, SHAPE, ZERO_DENOMINATOR, fraction_sum, head_root
from fraction_sum_model import model_verdict as fraction_verdict
from oracle.field import P

LOOKUP = 16
SEED = 20261021                                                    # of the instances the host and the GPU tests share
EMPTY = 0xFFFFFFFF
M64 = (1 << 64) - 1


def slot(v, log_slots):
    assert 0 <= v < 1 << 256 and 1 <= log_slots <= 32
    x = 0x9E3779B97F4A7C15
    for i in range(4):
        x = ((x ^ ((v >> (64 * i)) & M64)) * 0xFF51AFD7ED558CCD) & M64
        x ^= x >> 32
    x = (x * 0xC4CEB9FE1A85EC53) & M64
    x ^= x >> 29
    return x >> (64 - log_slots)


def multiplicities(W, T):
    """-> (M, missing, first_missing): the lowest index of a value of T takes the whole count."""
    first = {}
    for j, t in enumerate(T):
        first.setdefault(t, j)
    M, misses = [0] * len(T), []
    for i, w in enumerate(W):
        if w in first:
            M[first[w]] += 1
        else:
            misses.append(i)
    return M, len(misses), (misses[0] if misses else EMPTY)


def pair_log2(n_w, n_t):
    return max(n_w, n_t) + 1


def pair(W, T, M, alpha, n_w, n_t):
    assert len(W) == 1 << n_w and len(T) == 1 << n_t == len(M)
    half = 1 << (pair_log2(n_w, n_t) - 1)
    num = [1] * len(W) + [0] * (half - len(W)) + [(-m) % P for m in M] + [0] * (half - len(T))
    den = [(alpha - w) % P for w in W] + [1] * (half - len(W)) + [(alpha - t) % P for t in T] + [1] * (half - len(T))
    return num, den


def lookup(W, T, M, alpha, n_w, n_t, use_np=False):
    """fraction_sum_model.fraction_sum of the pair (its dict), with "pair" = (N, D)."""
    num, den = pair(W, T, M, alpha, n_w, n_t)
    if use_np:
        import numpy as np
        g = fraction_sum(np.array(num, dtype=object), np.array(den, dtype=object), pair_log2(n_w, n_t), use_np=True)
    else:
        g = fraction_sum(num, den, pair_log2(n_w, n_t))
    g["pair"] = (num, den)
    return g


def model_verdict(head, layers, W, T, M, alpha, n_w, n_t):
    num, den = pair(W, T, M, alpha, n_w, n_t)
    verdict = fraction_verdict(head, layers, num, den, None)
    if verdict[0] in (SHAPE, NON_CANONICAL, ZERO_DENOMINATOR):
        return verdict
    return (LOOKUP, 0, 0) if head_root(head)[0] != 0 else verdict


def plain_sum(num, den):
    """sum N / D by modular inverses (every D non-zero)."""
    return sum(x * pow(d, P - 2, P) for x, d in zip(num, den)) % P


# ---- the instances the tests run: (W, T) honest, and the dishonest (W, T, M) the verifier must answer with LOOKUP

def honest_instance(n_w, n_t, rng, duplicates=False):
    """A table of distinct values (duplicates: entries 1 and n - 1 repeat entry 0, entry 3 repeats entry 2) and a witness drawn from it."""
    T = []
    while len(T) < 1 << n_t:
        v = rng.randrange(P)
        if v not in T:
            T.append(v)
    if duplicates:
        T[1] = T[-1] = T[0]
        T[3] = T[2]
    W = [T[rng.randrange(len(T))] for _ in range(1 << n_w)]
    if duplicates:
        W[0], W[1], W[2] = T[0], T[0], T[2]
    return W, T


def fresh_alpha(W, T, rng):
    alpha = rng.randrange(P)
    while alpha in W or alpha in T:
        alpha = rng.randrange(P)
    return alpha


def dishonest_instances(n_w, n_t, rng):
    """-> {name: (W, T, M)}: "miss" one witness value outside the table (M counts the hits); "plus_one" M[j] + 1 at a used entry;
    "split_lossy" a duplicated value's count split over its copies with one hit lost on the way.  (A split that loses nothing is
    NOT dishonest: the copies' denominators are equal, so the sum stays zero -- split_instance below, which the tests hold to
    P = 0 and to an accepted proof.  "The lowest index takes the count" makes M a function of (W, T); soundness does not need it.)"""
    W, T = honest_instance(n_w, n_t, rng, duplicates=True)
    M, _, _ = multiplicities(W, T)
    out = {}
    Wm = list(W)
    v = rng.randrange(P)
    while v in T:
        v = rng.randrange(P)
    Wm[len(Wm) // 2] = v
    out["miss"] = (Wm, T, multiplicities(Wm, T)[0])
    j = next(j for j, m in enumerate(M) if m)
    out["plus_one"] = (W, T, M[:j] + [M[j] + 1] + M[j + 1:])
    split = list(M)
    assert split[0] >= 2 and split[1] == 0 and T[1] == T[0]
    split[0], split[1] = split[0] - 2, 1
    out["split_lossy"] = (W, T, split)
    return out


def split_instance(n_w, n_t, rng):
    """(W, T, M) with the count of a duplicated value split over its copies, nothing lost: other than multiplicities(W, T), and
    still a lookup that holds."""
    W, T = honest_instance(n_w, n_t, rng, duplicates=True)
    M, _, _ = multiplicities(W, T)
    assert M[0] >= 2 and M[1] == 0 and T[1] == T[0]
    M[0], M[1] = M[0] - 1, 1
    return W, T, M
