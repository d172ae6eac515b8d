"""The five batch verifiers back to back on ONE context: gkr_verify_prepared, gkr_sumcheck_mle_verify_batch_device,
gkr_sumcheck_sop_verify_batch_device, gkr_r1cs_verify_batch_device and gkr_grand_product_verify_batch_device build their chunks
from the same pieces (csrc/verify_chunk.h), which hold what used to be each file's own: the side stream's fork and join on the
context's two aux events and the guard that joins it on every way out.  Each suite runs its verifier alone; here they follow one
another, in order and in reverse, with the hashes on the host threads and on the device, in one chunk and in several.

The shapes are the smallest the suites build: a golden circuit, the n = 3 golden transcripts of the plain and the sum-of-products
sumcheck, the R1CS `random-n3-ny2` (its two sets of round vectors differ in width and in length) and the n = 5 grand product.
A batch is one tampered proof, honest copies, one tampered proof, honest copies, one tampered proof; its size is a prime above
what verify_workspace_mb = 1 holds in a chunk, so that setting gives several chunks and a ragged last one (the chunk count is read
from the hash launches).  The expected verdicts are the models' of the sweep modules, position by position; the verifiers' own
output is never the reference."""

import contextlib
import random

import numpy as np
import pytest

import mle_verify_sweeps as mle
import sop_verify_sweeps as sop
from gkr_amd import Context
from gkr_amd.convert import R1cs
from gkr_amd.dropin import _arrays_of_proof, verify_native
from gkr_amd.field import MODULUS as P, to_limbs
from grand_product_model import CHALLENGE as GP_CHALLENGE, EVALUATION as GP_EVALUATION, ROUND_SUM as GP_ROUND_SUM, proof_arrays
from grand_product_sweeps import apply, tamperings
from helpers import ints, layers_of
from resident_tables import Resident
from sop_model import sop_degree, sop_sumcheck
from test_gpu_grand_product import _batch_of, _model, _table
from test_gpu_r1cs_verify import _model_verdict, _prove, _sweep, _upload, _verdicts, _verifier_systems
from verify_sweeps import ACCEPTED, CHALLENGES, COEFFS, INPUT, R_LIMBS, circuit_of, elements, limbs, replicate, value

pytestmark = pytest.mark.gpu

SETTINGS = [(-1, 0), (1, 0), (1, 1), (-1, 1)]            # (verify_device_hash_min, verify_workspace_mb)
NAMES = ["gkr", "plain", "sop", "r1cs", "grand_product"]


def _spread(first, middle, last, honest, size):
    """[first, honest .., middle, honest .., last] of `size` entries."""
    half = (size - 3) // 2
    return [first] + [honest] * half + [middle] + [honest] * (size - 3 - half) + [last]


def _with_check(sweep, check):
    return next(c for c in sweep if c.verdict[2] == check)


class Verifier:
    """One verifier's batch: `want`, the model's verdicts; attach(ctx, stack) -> a call that returns the device's."""
    hash_launches_per_chunk = 1


class Gkr(Verifier):
    size = 401

    def __init__(self, ctx, gkr_cases):
        case = next(c for c in gkr_cases if c["name"] == "r6_k54_mix_8")
        self.circuit = circuit_of(layers_of(case), len(case["inputs"]))
        ks = self.circuit.get_k_list()
        arrs = _arrays_of_proof(ctx.prove(self.circuit, ints(case["inputs"])))
        elems = elements(ks, arrs)
        first = next(e for e in elems if e.arr == COEFFS and e.read)          # r in a used slot: no hash for that round vector
        middle = [e for e in elems if e.arr == CHALLENGES][-1]               # the last challenge + 1
        last = [e for e in elems if e.arr == INPUT][-1]                      # r in the last input coefficient
        B = self.size
        self.arrs = replicate(arrs, B)
        self.arrs[COEFFS][(0,) + first.index] = R_LIMBS
        at = (B // 2,) + middle.index
        self.arrs[CHALLENGES][at] = limbs((value(self.arrs[CHALLENGES][at]) + 1) % P)
        self.arrs[INPUT][(B - 1,) + last.index] = R_LIMBS
        self.want = [ACCEPTED] * B
        self.want[0], self.want[B - 1] = first.mod_verdict, last.mod_verdict
        # (the model of x + 1 says "rejected"; where, is the host verifier's word)
        self.want[B // 2] = verify_native(self.circuit, self.arrs, index=B // 2, threads=0)
        assert middle.read and not self.want[B // 2][0] and not self.want[0][0] and not self.want[B - 1][0]

    def attach(self, ctx, stack):
        handle = stack.enter_context(ctx.prepare_verify(self.circuit))
        return lambda: ctx.verify_batch(handle, self.arrs)


class Plain(Verifier):
    size = 4001

    def __init__(self, ctx, mle_cases):
        case = next(c for c in mle_cases if c["n"] == 3)
        self.n, table = 3, ints(case["table"])
        C, L, R = mle.arrays_of(ints(case["proof"]), ints(case["r"]))
        sweep = mle.cases(C, L, R, True)
        batch = _spread(_with_check(sweep, mle.CHALLENGE), _with_check(sweep, mle.NON_CANONICAL), _with_check(sweep, mle.EVALUATION), sweep[0], self.size)
        self.T, self.C, self.L, self.R, self.claims = mle.build_batch(to_limbs(table), C, L, R, to_limbs([sum(table) % P])[0], batch)
        self.want = [c.verdict for c in batch]

    def attach(self, ctx, stack):
        dev = stack.enter_context(Resident(ctx, self.T))

        def run():
            accept, rnd, check, _ = ctx.verify_sumcheck_batch_device(dev.d, self.n, self.size, self.C, self.L, self.R, claims=self.claims)
            return [(bool(a), int(r), int(c)) for a, r, c in zip(accept, rnd, check)]
        return run


class Sop(Verifier):
    size = 2503

    def __init__(self, ctx, sop_cases):
        case = next(c for c in sop_cases if c["name"] == "AB-C" and c["n"] == 3)
        self.n, self.terms = 3, [(int(k), tuple(idx)) for k, idx in case["terms"]]
        tables = [ints(t) for t in case["tables"]]
        self.M = len(tables)
        proof, r, evals = sop_sumcheck(tables, self.terms, self.n)
        assert proof == ints(case["proof"]) and r == ints(case["r"])
        C, L, R = sop.arrays_of(proof, r, sop_degree(self.terms))
        sweep = sop.cases(C, L, R, evals, self.terms, True)
        batch = _spread(_with_check(sweep, sop.ROUND_SUM), _with_check(sweep, sop.CHALLENGE), _with_check(sweep, sop.EVALUATION), sweep[0], self.size)
        T1 = np.concatenate([to_limbs(t) for t in tables]).reshape(self.M, 1 << self.n, 4)
        self.T, self.C, self.L, self.R, self.claims = sop.build_batch(T1, C, L, R, to_limbs([int(case["claim"])])[0], batch)
        self.want = [c.verdict for c in batch]

    def attach(self, ctx, stack):
        dev = stack.enter_context(Resident(ctx, self.T))

        def run():
            res = ctx.verify_sumcheck_sop_batch_device(dev.d, self.n, self.M, self.terms, self.size, self.C, self.L, self.R, claims=self.claims)
            return [(bool(a), int(r), int(c)) for a, r, c in zip(res[0], res[1], res[2])]
        return run


class R1csProofs(Verifier):
    size = 1301
    hash_launches_per_chunk = 2                                              # rows of four slots, then rows of three

    def __init__(self, ctx):
        self.n_wires, self.cons, witness = _verifier_systems()["random-n3-ny2"]
        self.w = witness(0)
        rng = random.Random(28100)
        z, rho = [rng.randrange(P) for _ in range(3)], [rng.randrange(1, P) for _ in range(3)]
        self.r1cs = R1cs.build(self.n_wires, 1, 1, 1, self.cons)
        d_w = _upload(ctx, [self.w], self.n_wires, self.n_wires)
        try:
            with ctx.r1cs_rows(self.r1cs) as rows:
                zc, inner = _prove(ctx, self.r1cs, rows, d_w, 1, [z], [rho], self.n_wires)
        finally:
            ctx.free(d_w)
        szc, sinner = _sweep(zc, inner)                                      # entry 0 is the honest proof
        model = [_model_verdict(self.cons, z, rho, szc, sinner, e, self.w[:self.n_wires]) for e in range(szc[0].shape[0])]
        assert model[0] == (0, 0, 0)
        stage1 = next(e for e, v in enumerate(model) if v[0] == 1)
        stage2 = next(e for e, v in enumerate(model) if v[0] == 2)
        last = max(e for e, v in enumerate(model) if v != (0, 0, 0))
        idx = np.array(_spread(stage1, stage2, last, 0, self.size))
        self.zc, self.inner = tuple(np.ascontiguousarray(a[idx]) for a in szc), tuple(np.ascontiguousarray(a[idx]) for a in sinner)
        self.z = np.ascontiguousarray(np.repeat(to_limbs(z)[None], self.size, axis=0))
        self.rho = np.ascontiguousarray(np.repeat(to_limbs(rho)[None], self.size, axis=0))
        self.want = [model[e] for e in idx]

    def attach(self, ctx, stack):
        rows = stack.enter_context(ctx.r1cs_rows(self.r1cs))
        d_w = _upload(ctx, [self.w] * self.size, self.n_wires, self.n_wires)
        stack.callback(ctx.free, d_w)
        return lambda: _verdicts(ctx.verify_r1cs_batch_device(rows, self.size, self.z, self.zc, self.rho, self.inner, d_witness=d_w))


class GrandProduct(Verifier):
    size = 1301

    def __init__(self, ctx):
        self.n = n = 5
        table, g = _table(n, "random"), _model(n, "random")
        arrays = proof_arrays(g, n)
        sweep = tamperings(g, n, True, True)
        pick = [next((what, want) for _, what, want in sweep if want[0] == check) for check in (GP_CHALLENGE, GP_ROUND_SUM, GP_EVALUATION)]
        four = _batch_of(n, [(arrays, table, g["product"])] + [apply(what, arrays, table, g["product"]) for what, _ in pick])
        idx = np.array(_spread(1, 2, 3, 0, self.size))
        self.T, self.products, self.H, self.C, self.L, self.R, self.E = (np.ascontiguousarray(a[idx]) for a in four)
        self.want = [((0, 0, 0), pick[0][1], pick[1][1], pick[2][1])[e] for e in idx]

    def attach(self, ctx, stack):
        dev = stack.enter_context(Resident(ctx, self.T))

        def run():
            accept, layer, rnd, check, _ = ctx.verify_grand_product_batch_device(dev.d, self.n, self.size, self.H, self.C, self.L, self.R, self.E,
                                                                                 products=self.products)
            assert list(accept) == [int(c) == 0 for c in check]
            return [(int(c), int(l), int(r)) for c, l, r in zip(check, layer, rnd)]
        return run


@pytest.fixture(scope="module")
def world(gkr_cases, mle_cases):
    """The ONE context, the five batches (made once) and their calls on that context."""
    from conftest import load_golden
    with Context(0) as ctx, contextlib.ExitStack() as stack:
        verifiers = [Gkr(ctx, gkr_cases), Plain(ctx, mle_cases), Sop(ctx, load_golden("sop_sumcheck.json")["cases"]), R1csProofs(ctx), GrandProduct(ctx)]
        for v in verifiers:
            assert len(v.want) == v.size and v.want[0] != v.want[1] and v.want[v.size // 2] != v.want[1] and v.want[-1] != v.want[1]
            assert sum(w != v.want[1] for w in v.want) == 3, "three tampered proofs: the first, the middle and the last"
        yield ctx, verifiers, [v.attach(ctx, stack) for v in verifiers]


def _first_difference(got, want):
    return next(((i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w), None)


@contextlib.contextmanager
def _setting(ctx, hash_min, mb):
    ctx.set_option("verify_device_hash_min", hash_min)
    ctx.set_option("verify_workspace_mb", mb)
    try:
        yield
    finally:
        ctx.set_option("verify_device_hash_min", 0)
        ctx.set_option("verify_workspace_mb", 0)


@pytest.mark.parametrize("hash_min,mb", SETTINGS)
def test_in_turn_and_in_reverse_on_one_context(world, hash_min, mb):
    ctx, verifiers, calls = world
    order = list(range(5)) + list(range(4, -1, -1))
    with _setting(ctx, hash_min, mb):
        ctx.profile(1)
        try:
            for step, i in enumerate(order):
                ctx.profile_reset()
                got = calls[i]()
                launches = ctx.profile_get("verify_hash")["launches"]
                assert _first_difference(got, verifiers[i].want) is None, (NAMES[i], step, _first_difference(got, verifiers[i].want))
                per = verifiers[i].hash_launches_per_chunk
                if hash_min < 0:
                    assert launches == 0, (NAMES[i], launches)
                elif mb == 0:
                    assert launches == per, (NAMES[i], launches)
                else:                                                        # several chunks; a prime batch: the last one is ragged
                    assert launches % per == 0 and 2 <= launches // per < verifiers[i].size, (NAMES[i], launches)
        finally:
            ctx.profile(0)


@pytest.mark.parametrize("which", range(5), ids=NAMES)
def test_a_fresh_context_gives_the_same_verdicts(world, which):
    ctx, verifiers, calls = world
    with Context(0) as fresh, contextlib.ExitStack() as stack:
        call = verifiers[which].attach(fresh, stack)
        for hash_min, mb in SETTINGS:
            with _setting(fresh, hash_min, mb), _setting(ctx, hash_min, mb):
                alone, shared = call(), calls[which]()
            assert alone == shared, (NAMES[which], hash_min, mb, _first_difference(alone, shared))
            assert alone == verifiers[which].want, (NAMES[which], hash_min, mb)
