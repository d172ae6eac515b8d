"""Model of the ballot carry / borrow lookahead of the eight-lane MiMC7 code (gkr_amd/csrc/mimc_lanes.h), on the CPU.

resolve_carries and cond_sub settle the carries (borrows) of all eight groups of a wave -- eight independent field
elements, eight different transcripts -- with one 64-bit add over ballots: bit 8g + j is lane j of group g.  A carry
that runs through a group's top lane must stop there; if it ripples into bit 8(g + 1) it changes the NEIGHBOURING
group's value.  This test reads the 64-bit statements of both functions out of the header, replays them in Python on
a wave of eight groups, and compares every group with big integers -- on the cases that put a carry exactly through
a top lane next to a group that is sensitive to it.  The device form is checked on the GPU by
tests/test_gpu_device_arith.py; this one fails without a GPU if a later edit brings the leak back.
"""

import os
import random
import re

import pytest

from oracle.field import P

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gkr_amd", "csrc", "mimc_lanes.h")
M32 = (1 << 32) - 1
M64 = (1 << 64) - 1


def _body(src, name):
    i = src.index("__device__ __forceinline__ uint32_t %s(" % name)
    j = src.index("\n}\n", i)
    return src[i:j]


def _u64_statements(body):
    """The function's `const uint64_t name = expr;` statements that do not take a ballot, as (name, python expr)."""
    out = []
    for name, expr in re.findall(r"const uint64_t (\w+)\s*=\s*([^;]+);", body):
        if "__ballot" in expr:
            continue
        py = re.sub(r"(0x[0-9a-fA-F]+|\d+)u?ll\b", r"\1", expr)
        assert re.fullmatch(r"[\w\s()<>&|^+~]*", py), "unexpected C in a lookahead statement: " + expr
        out.append((name, py))
    return out


def _replay(stmts, env):
    for name, expr in stmts:
        env[name] = eval(expr, {}, env) & M64   # every operator used (+ ^ & | <<) wraps like the device's 64-bit add
    return env


def _limbs(x):
    return [(x >> (32 * j)) & M32 for j in range(8)]


def _value(limbs):
    return sum(v << (32 * j) for j, v in enumerate(limbs))


def model_cond_sub(xs, m, stmts):
    """cond_sub(x, m) of mimc_lanes.h over one wave of eight groups: xs[g] is group g's value (< 2^256)."""
    mj = _limbs(m)
    lanes = [_limbs(x) for x in xs]
    g = p = 0
    d = {}
    for gi in range(8):
        for j in range(8):
            b = 8 * gi + j
            x = lanes[gi][j]
            d[b] = (x - mj[j]) & M32
            g |= int(x < mj[j]) << b
            p |= int(d[b] == 0) << b
    env = _replay(stmts, {"g": g, "p": p})
    bin_, out = env["bin"], env["out"]
    res = []
    for gi in range(8):
        if (out >> (8 * gi + 7)) & 1:
            res.append(xs[gi])
        else:
            res.append(_value([(d[8 * gi + j] - ((bin_ >> (8 * gi + j)) & 1)) & M32 for j in range(8)]))
    return res


def model_resolve(vals, stmts):
    """resolve_carries of mimc_lanes.h over one wave: vals[g][j] = limb + 2^32 * extra of lane j of group g."""
    g = p = 0
    s = {}
    for gi in range(8):
        for j in range(8):
            b = 8 * gi + j
            v = vals[gi][j]
            limb, extra = v & M32, v >> 32
            from_below = 0 if j == 0 else (vals[gi][j - 1] >> 32)
            s[b] = (limb + from_below) & M32
            g |= int(s[b] < limb) << b
            p |= int(s[b] == M32) << b
    env = _replay(stmts, {"g": g, "p": p})
    cin = env["cin"]
    return [_value([(s[8 * gi + j] + ((cin >> (8 * gi + j)) & 1)) & M32 for j in range(8)]) for gi in range(8)]


@pytest.fixture(scope="module")
def stmts():
    src = open(HEADER).read()
    cs, rc = _u64_statements(_body(src, "cond_sub")), _u64_statements(_body(src, "resolve_carries"))
    assert [n for n, _ in cs][-2:] == ["bin", "out"] and "gs" in dict(cs)
    assert [n for n, _ in rc][-1] == "cin" and "gs" in dict(rc)
    return {"cond_sub": cs, "resolve": rc}


def _want_cond_sub(xs, m):
    return [x - m if x >= m else x for x in xs]


def test_issue_repro(stmts):
    """A borrow through group 0's top lane (top limb equal to m's, x < m) must not reach group 1 (x = m + 12345)."""
    m = 2 * P
    x0 = ((m >> 224) << 224) | 5
    xs = [x0, m + 12345] + [0] * 6
    assert model_cond_sub(xs, m, stmts["cond_sub"]) == _want_cond_sub(xs, m)


def _adversarial_values(m, rng):
    top = (m >> 224) << 224
    return [m, m - 1, m + 1, top, top | rng.randrange(1 << 224), top + (1 << 224) - 1, top | 5,
            (m | ((1 << 192) - 1)) if (m | ((1 << 192) - 1)) < (1 << 256) else m, rng.randrange(1 << 256), rng.randrange(m),
            m + rng.randrange(1 << 64), (1 << 256) - 1, 0]


@pytest.mark.parametrize("which", ["p", "2p"])
def test_cond_sub_borrow_stays_in_its_group(which, stmts):
    """Every neighbouring pair (g, g + 1) -- across the 16-lane row boundary too -- with a borrow through g's top lane
    beside a group at, just above or just below m; then waves of adversarial and random groups."""
    m = P if which == "p" else 2 * P
    rng = random.Random(7 if which == "p" else 8)
    top = (m >> 224) << 224
    for gi in range(7):
        for victim in (m, m + 1, m - 1, m + 12345, m + (1 << 224), top + ((1 << 224) - 1)):
            for left in (top | 5, top, m - 1):
                xs = [rng.randrange(3 * P) for _ in range(8)]
                xs[gi], xs[gi + 1] = left, victim
                assert model_cond_sub(xs, m, stmts["cond_sub"]) == _want_cond_sub(xs, m), (gi, hex(victim), hex(left))
    for _ in range(3000):
        vals = _adversarial_values(m, rng)
        xs = [vals[rng.randrange(len(vals))] for _ in range(8)]
        assert model_cond_sub(xs, m, stmts["cond_sub"]) == _want_cond_sub(xs, m), [hex(x) for x in xs]


def _lanes_total(vals):
    return sum(v << (32 * j) for j, v in enumerate(vals))


def _random_group(rng):
    """Lane values of a sum below 2^256: random limbs, small deferred carries in lanes 0 .. 6 (what add3 / mont_mul leave)."""
    vals = [rng.randrange(1 << 32) + (rng.randrange(3) << 32) for _ in range(7)] + [rng.randrange(1 << 31)]
    return vals


def _run_group(rng, start, end):
    """Limbs start .. end all ones, a carry arriving at `start` from the lane below (its deferred carry, or its own sum)."""
    vals = [rng.randrange(1 << 32) for _ in range(8)]
    for j in range(start, end + 1):
        vals[j] = M32
    if start > 0:
        vals[start - 1] += 1 << 32
    if end < 7:
        vals[7] = rng.randrange(1 << 31)
    return vals


def test_resolve_carries_stay_in_their_group(stmts):
    """Runs of all-ones limbs inside a group that a carry walks through, beside groups that carry themselves -- every
    neighbouring pair (g, g + 1).  A group whose sum reaches 2^256 (outside the bound, so the run ends in the top lane)
    keeps its value mod 2^256 and leaves its neighbours alone."""
    rng = random.Random(11)
    for gi in range(7):
        for start in range(1, 8):
            for end in range(start, 8):
                groups = [_random_group(rng) for _ in range(8)]
                groups[gi] = _run_group(rng, start, end)
                groups[gi + 1] = _run_group(rng, 1, rng.randrange(1, 7)) if rng.random() < 0.5 else _random_group(rng)
                want = [_lanes_total(v) % (1 << 256) for v in groups]
                assert model_resolve(groups, stmts["resolve"]) == want, (gi, start, end)
    for _ in range(3000):
        groups = [_run_group(rng, rng.randrange(1, 8), 6) if rng.random() < 0.5 else _random_group(rng) for _ in range(8)]
        assert model_resolve(groups, stmts["resolve"]) == [_lanes_total(v) for v in groups]
