"""The one-column instances of the lookup's multiplicities that tests/test_gpu_lookup.py runs on the device against the integer
model and tests/test_oracle_lookup_c.py runs through the C oracle: keys chosen through the slot function so that all land in one
slot (the longest chain), in the last slot (the wrap) or in distinct slots; repeated table values; entries equal in seven limbs;
0 and r - 1; the first two-block launches; one value 2^12 times; 0, 1 and several misses."""

import random

from lookup_model import SEED, honest_instance, slot
from oracle.field import P


def _keys_in_slot(target, log_slots, count, rng, avoid=()):
    """`count` distinct values whose slot among 2^log_slots is `target`."""
    out = []
    while len(out) < count:
        v = rng.randrange(P)
        if slot(v, log_slots) == target and v not in out and v not in avoid:
            out.append(v)
    return out


def _distinct_slot_keys(log_slots, count, rng):
    out, used = [], set()
    while len(out) < count:
        v = rng.randrange(P)
        if slot(v, log_slots) not in used:
            used.add(slot(v, log_slots))
            out.append(v)
    return out


def draw(T, n_w, rng):
    return [T[rng.randrange(len(T))] for _ in range(1 << n_w)]


def _cases():
    """name -> (W, T): every case of section a. with one column."""
    rng = random.Random(SEED + 10)
    out = {}
    for n_t in (2, 3):
        s = n_t + 1
        T = _keys_in_slot(5 % (1 << s), s, 1 << n_t, rng)
        out["one slot, n_t = %d" % n_t] = (draw(T, 3, rng), T)
        T = _keys_in_slot((1 << s) - 1, s, 1 << n_t, rng)
        out["last slot, n_t = %d" % n_t] = (draw(T, 3, rng), T)
        T = _distinct_slot_keys(s, 1 << n_t, rng)
        out["distinct slots, n_t = %d" % n_t] = (draw(T, 3, rng), T)
    a, b, c = (rng.randrange(P) for _ in range(3))
    T = [a, b, a, c, b, b, a, a]                                   # a four times, b three times, c once
    out["repeated table values"] = ([a, a, b, c, a, b, b, a, c, c, a, b, a, a, b, c], T)
    base = rng.randrange(P >> 2)
    T = [base ^ (1 << (32 * limb + 5)) for limb in range(8)]       # any two differ in two limbs; each differs from base in one
    out["seven equal limbs"] = (draw(T, 4, rng) + [T[7 - i] for i in range(8)] + draw(T, 3, rng), T)
    T = [base, base ^ 1, base ^ (1 << 255 >> 2), base ^ (1 << 64)]
    out["one limb apart"] = (draw(T, 3, rng), T)
    T = [0, P - 1, 1, P - 2]
    out["0 and r - 1"] = ([0, P - 1, P - 1, 0, 0, 1, P - 2, 0], T)
    for n_w, n_t in ((2, 9), (9, 3), (10, 3)):
        W, T = honest_instance(n_w, n_t, rng)
        out["n_w = %d, n_t = %d" % (n_w, n_t)] = (W, T)
    W, T = honest_instance(2, 3, rng)
    out["one value 2^12 times"] = ([T[6]] * (1 << 12), T)
    # misses
    W, T = honest_instance(4, 3, rng)
    outside = [v for v in (rng.randrange(P) for _ in range(8)) if v not in T]
    out["one miss"] = (W[:11] + [outside[0]] + W[12:], T)
    out["several misses"] = ([outside[1]] + W[1:5] + [outside[2], outside[2]] + W[7:15] + [outside[3]], T)
    out["every entry a miss"] = (outside[:4], T[:4])
    chain = _keys_in_slot(9, 4, 8, rng)                            # slots 9 .. 15 and 0 occupied
    stray = _keys_in_slot(9, 4, 1, rng, avoid=chain)[0]            # probes all eight, then the empty slot 1
    out["a miss behind a full chain"] = ([chain[7], stray, chain[0], stray], chain)
    return out


CASES = _cases()
