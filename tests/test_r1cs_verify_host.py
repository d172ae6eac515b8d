"""The R1CS verifier (include/gkr_amd.h, gkr_r1cs_matrix_evals_device / gkr_r1cs_verify*) as far as no device is needed: the
symbols, the argument checks that return before a device is touched, the integer model verifier.verify_r1cs -- the model the
device is held to (tests/test_gpu_r1cs_verify.py) -- on honest and tampered transcripts made by the zero-check and product models,
and the shared round relations (csrc/verify_rounds.h) in a stand-alone program under AddressSanitizer and UBSan (a child process:
no sanitizer goes near code loaded into python).

The tamper sweep's expected verdicts are worked out from the rules of the header, position by position (tamperings):
  a used slot + 1            the round's own sum moves by 1 (2 for the constant term): ROUND_SUM at that round;
  a challenge + 1            the round's sum still holds, its hash does not: CHALLENGE at that round;
  a length + 1               beyond the row's width SHAPE; else a leading zero joins the used slots -- same sum, same value at
                             r_j, another hash: CHALLENGE;
  a length - 1               0: SHAPE; else the leading coefficient (non-zero: the provers drop leading zeros) leaves the sum:
                             ROUND_SUM;
  v_A, v_B, v_C + 1          eq(z, r_x) (v_A v_B - v_C) moves by eq v_B, eq v_A, -eq -- non-zero on a sharp base: stage 1 EVALUATION;
  e_T, e_w + 1               e_T e_w moves by e_w, e_T -- non-zero on a sharp base: stage 2 EVALUATION."""

import ctypes
import os
import random
import re
import subprocess

import pytest

from gkr_amd import _native as N
from gkr_amd.field import MODULUS as P
from gkr_amd.verifier import R1CS_ZEROCHECK_TERMS, verify_r1cs, verify_r1cs_inner, verify_sumcheck_zerocheck
from product_model import product_sumcheck
from r1cs_cols_model import cols_table, n_y_of
from r1cs_rows_model import rows, table_log2
from zerocheck_model import zerocheck_sumcheck

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gkr_r1cs_matrix_evals_device", "gkr_r1cs_verify_batch_device", "gkr_r1cs_verify"]
SHAPE, NON_CANONICAL, ROUND_SUM, CHALLENGE, EVALUATION = (N.GKR_VERIFY_SHAPE, N.GKR_VERIFY_NON_CANONICAL, N.GKR_VERIFY_ROUND_SUM,
                                                          N.GKR_VERIFY_CHALLENGE, N.GKR_VERIFY_EVALUATION)


def test_the_symbols_are_declared_and_exported():
    header = open(os.path.join(REPO, "include", "gkr_amd.h")).read()
    lib = N.lib()
    for name in NAMES:
        assert name in N.SYMBOLS, name
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert re.search(r"GKR_VERIFY_MATRIX = 11\b", header) and re.search(r"GKR_VERIFY_WITNESS = 12\b", header)
    assert (N.GKR_VERIFY_MATRIX, N.GKR_VERIFY_WITNESS) == (11, 12)


def test_refusals_before_a_device_is_touched():
    """No context exists here (no device): `fake` stands for a context, a handle or an array that is never dereferenced -- every
    refusal below is decided from NULL pointers and the batch alone.  (A handle of another context, the 2^30 cap and the canonical
    checks need a real handle: tests/test_gpu_r1cs_verify.py.)"""
    lib = N.lib()
    word = (ctypes.c_uint64 * 512)()
    fake = ctypes.c_void_p(ctypes.addressof(word))
    INVALID = N.GKR_ERR_INVALID
    good = [fake, fake, fake, fake, 1, fake]                                # (ctx, rows, x, y, batch, out)
    for at in (0, 1, 2, 3, 5):
        args = list(good)
        args[at] = None
        assert lib.gkr_r1cs_matrix_evals_device(*args) == INVALID, at
    for batch in (0, -1, 65536, 1 << 30):
        assert lib.gkr_r1cs_matrix_evals_device(fake, fake, fake, fake, batch, fake) == INVALID, batch
    # (ctx, rows, batch, z, coeffs_x, len_x, r_x, evals_abc, rho, coeffs_y, len_y, r_y, evals_tw, d_witness, stride, accept, stage, round, check)
    good = [fake, fake, 1] + [fake] * 10 + [None, 0, fake, None, None, None]
    for at in (0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 15):
        args = list(good)
        args[at] = None
        assert lib.gkr_r1cs_verify_batch_device(*args) == INVALID, at
    for batch in (0, -1, 65536):
        args = list(good)
        args[2] = batch
        assert lib.gkr_r1cs_verify_batch_device(*args) == INVALID, batch
    # (ctx, r1cs, z, coeffs_x, len_x, r_x, evals_abc, rho, coeffs_y, len_y, r_y, evals_tw, witness, n_witness, accept, stage, round, check)
    good = [fake] * 12 + [None, 0, fake, None, None, None]
    for at in list(range(12)) + [14]:
        args = list(good)
        args[at] = None
        assert lib.gkr_r1cs_verify(*args) == INVALID, at
    assert not any(word), "nothing was written through a pointer"


# ---- the cases: a satisfied system for every (n, n_y) in 2 .. 4, a random and a boolean z ------------------------------------------------
def _system(rng, n_constraints, n_wires):
    """A random system and a witness that satisfies it: A and B are random combinations of 1 .. 3 terms, C = c w_k + (a b - c w_k) w_0
    with w_0 = 1.  Every wire value is non-zero."""
    w = [1] + [rng.randrange(1, P) for _ in range(n_wires - 1)]
    cons = []
    for _ in range(n_constraints):
        A = [(rng.randrange(1, P), rng.randrange(n_wires)) for _ in range(rng.randrange(1, 4))]
        B = [((1, P - 1, rng.randrange(1, P))[rng.randrange(3)], rng.randrange(n_wires)) for _ in range(rng.randrange(1, 4))]
        a, b = (sum(c * w[k] for c, k in lc) % P for lc in (A, B))
        k, c = rng.randrange(n_wires), rng.randrange(1, P)
        cons.append((A, B, [(c, k), ((a * b - c * w[k]) % P, 0)]))
    return cons, w


def _prove(cons, w, n_wires, z, rho):
    """The honest transcripts of the two sumchecks from the models: -> dict of verify_r1cs's arguments."""
    n, n_y = table_log2(len(cons)), n_y_of(n_wires)
    zc, r_x, abc, eq_r = zerocheck_sumcheck(rows(cons, w, n), R1CS_ZEROCHECK_TERMS, z, n)
    T = cols_table(cons, n_wires, r_x, rho, n_y)
    inner, r_y, tw = product_sumcheck([T, w + [0] * ((1 << n_y) - len(w))], n_y)
    return dict(z=list(z), rho=list(rho), zc=zc, r_x=r_x, abc=abc, inner=inner, r_y=r_y, tw=tw, eq_r=eq_r)


def _verdict(cons, p, witness=None):
    return verify_r1cs(cons, p["z"], p["rho"], p["zc"], p["r_x"], p["abc"], p["inner"], p["r_y"], p["tw"], witness)


def _cases():
    out = []
    for n in (2, 3, 4):
        for n_y in (2, 3, 4):
            for boolean in (False, True):
                rng = random.Random(20100 + 100 * n + 10 * n_y + boolean)
                n_constraints, n_wires = (1 << n) - n_y % 2, (1 << n_y) - n % 2              # the full table and one short of it
                cons, w = _system(rng, n_constraints, n_wires)
                assert table_log2(n_constraints) == n and n_y_of(n_wires) == n_y
                z = [rng.randrange(2) if boolean else rng.randrange(P) for _ in range(n)]
                rho = [rng.randrange(1, P) for _ in range(3)]
                out.append((("n%d-ny%d-%s" % (n, n_y, "bool" if boolean else "rand")), cons, w, n_wires, _prove(cons, w, n_wires, z, rho)))
    return out


@pytest.fixture(scope="module")
def cases():
    return _cases()


def tamperings(p):
    """Every single change of the sweep as (name, changed proof, expected (stage, round, check)): each slot, each challenge, each
    evaluation to x + 1 mod r, each length by +-1 (the list model of a length: + 1 takes the zero of the unused slot in front,
    - 1 drops the leading coefficient)."""
    out = []
    for stage, key, rkey, width in ((1, "zc", "r_x", 4), (2, "inner", "r_y", 3)):
        for j, g in enumerate(p[key]):
            for k in range(len(g)):
                q = dict(p, **{key: [list(v) for v in p[key]]})
                q[key][j][k] = (g[k] + 1) % P
                out.append(("%s[%d][%d]+1" % (key, j, k), q, (stage, j, ROUND_SUM)))
            q = dict(p, **{rkey: list(p[rkey])})
            q[rkey][j] = (p[rkey][j] + 1) % P
            out.append(("%s[%d]+1" % (rkey, j), q, (stage, j, CHALLENGE)))
            q = dict(p, **{key: [list(v) for v in p[key]]})
            q[key][j] = [0] + list(g)
            out.append(("len %s[%d]+1" % (key, j), q, (stage, j, SHAPE if len(g) == width else CHALLENGE)))
            q = dict(p, **{key: [list(v) for v in p[key]]})
            q[key][j] = list(g[1:])
            out.append(("len %s[%d]-1" % (key, j), q, (stage, j, SHAPE if len(g) == 1 else ROUND_SUM)))
    for m in range(3):
        q = dict(p, abc=list(p["abc"]))
        q["abc"][m] = (p["abc"][m] + 1) % P
        out.append(("abc[%d]+1" % m, q, (1, len(p["z"]), EVALUATION)))
    for m in range(2):
        q = dict(p, tw=list(p["tw"]))
        q["tw"][m] = (p["tw"][m] + 1) % P
        out.append(("tw[%d]+1" % m, q, (2, len(p["r_y"]), EVALUATION)))
    return out


def assert_sharp(p):
    """The base every expected verdict of the sweep rests on."""
    assert p["eq_r"] != 0 and p["abc"][0] != 0 and p["abc"][1] != 0 and all(p["rho"]) and p["tw"][0] != 0 and p["tw"][1] != 0
    assert all(g[0] != 0 or len(g) == 1 for g in p["zc"] + p["inner"]), "leading zeros are dropped"


def test_honest_transcripts_are_accepted(cases):
    for name, cons, w, n_wires, p in cases:
        assert _verdict(cons, p) == (0, 0, 0), name
        assert _verdict(cons, p, w) == (0, 0, 0), name
    assert sorted({(len(p["z"]), len(p["r_y"])) for _, _, _, _, p in cases}) == [(a, b) for a in (2, 3, 4) for b in (2, 3, 4)]


def test_every_tampering_is_rejected_where_the_rules_say(cases):
    total = 0
    for name, cons, w, n_wires, p in cases:
        assert_sharp(p)
        for what, q, want in tamperings(p):
            got = _verdict(cons, q, w)
            assert got == want, (name, what, got, want)
            total += 1
    assert total > 700


def test_the_model_agrees_with_the_two_verifiers_it_is_built_on(cases):
    """verify_r1cs accepts exactly what verify_sumcheck_zerocheck (claim 0) followed by verify_r1cs_inner accepts, honest and
    tampered alike (no witness: the two leave the claim on it open, as verify_r1cs does then)."""
    for name, cons, w, n_wires, p in cases:
        for what, q, _ in [("honest", p, None)] + tamperings(p):
            both = (verify_sumcheck_zerocheck(q["zc"], q["r_x"], q["abc"], R1CS_ZEROCHECK_TERMS, q["z"], 0)
                    and verify_r1cs_inner(cons, q["r_x"], q["rho"], q["abc"], q["inner"], q["r_y"], q["tw"]) is not None)
            assert (_verdict(cons, q) == (0, 0, 0)) == bool(both), (name, what)


def test_later_stages_and_non_canonical_elements(cases):
    """What the sweep cannot reach: a changed coefficient of the verifier's matrices (stage 3), a changed witness (stage 4, and
    accepted without one), a proof element outside 0 .. r - 1."""
    name, cons, w, n_wires, p = cases[8]
    n, n_y = len(p["z"]), len(p["r_y"])
    A, B, C = cons[1]
    other = list(cons)
    other[1] = ([((A[0][0] + 1) % P, A[0][1])] + A[1:], B, C)
    assert _verdict(other, p, w) == (3, n_y, N.GKR_VERIFY_MATRIX)
    w2 = list(w)
    w2[n_wires - 1] = (w2[n_wires - 1] + 1) % P
    assert _verdict(cons, p, w2) == (4, n_y, N.GKR_VERIFY_WITNESS) and _verdict(cons, p) == (0, 0, 0)
    for key, j, want in (("zc", 1, (1, 1, NON_CANONICAL)), ("inner", 0, (2, 0, NON_CANONICAL))):
        q = dict(p, **{key: [list(v) for v in p[key]]})
        q[key][j][-1] += P
        assert _verdict(cons, q, w) == want
    for key, j, want in (("r_x", n - 1, (1, n - 1, NON_CANONICAL)), ("abc", 2, (1, n, NON_CANONICAL)), ("r_y", 1, (2, 1, NON_CANONICAL)),
                         ("tw", 1, (2, n_y, NON_CANONICAL))):
        q = dict(p, **{key: list(p[key])})
        q[key][j] += P
        assert _verdict(cons, q, w) == want, key
    # SHAPE anywhere comes before NON_CANONICAL anywhere in the same transcript
    q = dict(p, zc=[list(v) for v in p["zc"]])
    q["zc"][0][0] += P
    q["zc"][n - 1] = []
    assert _verdict(cons, q, w) == (1, n - 1, SHAPE)


def test_a_broken_witness_fails_the_first_round_sum(cases):
    """The honest transcripts of a witness that breaks one constraint: the zero-check's claim is not zero."""
    for name, cons, w, n_wires, p in cases:
        if set(p["z"]) <= {0, 1}:
            continue                                                        # (a boolean z sees one row only)
        bad = list(w)
        k = cons[0][2][0][1]                                                # a wire of constraint 0's C
        bad[k] = (bad[k] + 1) % P
        q = _prove(cons, bad, n_wires, p["z"], p["rho"])
        assert _verdict(cons, q, bad) == (1, 0, ROUND_SUM), name
        assert _verdict(cons, q) == (1, 0, ROUND_SUM), name


def test_round_relations_stand_alone_under_address_and_ub_sanitizers(tmp_path):
    """tests/verify_rounds_selfcheck.cpp with csrc/verify_rounds.h (and csrc/keccak.cpp for the hash constants): the relations the
    device verifiers share, driven without a device; no sanitizer report.  A child process: nothing is loaded into this one."""
    exe = str(tmp_path / "verify_rounds_selfcheck")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-fno-omit-frame-pointer", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                            os.path.join(REPO, "tests", "verify_rounds_selfcheck.cpp"), os.path.join(REPO, "gkr_amd", "csrc", "keccak.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert out.returncode == 0 and "verify_rounds_selfcheck: ok" in out.stdout, out.stdout + out.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-3000:]
