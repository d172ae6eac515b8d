"""GPU runs AT the size limits include/gkr_amd.h states (GKR_MAX_MLE_N, GKR_MAX_K_I, GKR_MAX_K_NEXT,
GKR_MAX_K_NEXT_DEVICE_TRANSCRIPT, GKR_MAX_BATCH, 65535 sumchecks per gkr_sumcheck_mle_batch_device call), where byte offsets
pass 2^32, grids reach their caps and dense tables reach GiBs -- what parity at smaller shapes cannot see.  Every output is
compared bit for bit with the C oracle or with a committed digest of its transcript (tests/golden/config_hashes.json, written
by tests/golden/make_config_hashes.py --limits).  Each case runs in a child process of its own (tests/limits_worker.py) and
prints its wall time."""
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _run(*args, timeout=600):
    t = time.time()
    out = subprocess.run([sys.executable, os.path.join(HERE, "limits_worker.py")] + [str(a) for a in args], capture_output=True,
                         text=True, timeout=timeout)
    print("\nlimits %s: %.1f s (child)" % (" ".join(map(str, args)), time.time() - t))
    if out.returncode < 0 or out.returncode in (134, 139):   # a child that faulted or aborted: start nothing more on the card
        pytest.exit("limits_worker.py %s ended by a signal (%d):\n%s" % (" ".join(map(str, args)), out.returncode, out.stdout + out.stderr[-4000:]),
                    returncode=3)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("OK"), out.stdout + out.stderr


# The transcript does not depend on the pass schedule, so every schedule reproduces the oracle's digest.  A fold pass that
# writes S entries reads up to 2^JIN * S; its lanes' 32-bit byte offsets passed 2^32 from S = 2^28 (rounds_per_pass 1 at
# n = 29 and 30, 2 at n = 30); rounds_per_pass 3 at n = 30 ends exactly at 2^32.
@pytest.mark.parametrize("n,options", [
    (30, ["rounds_per_pass=1"]), (30, ["rounds_per_pass=2"]), (30, ["rounds_per_pass=3"]), (30, ["rounds_per_pass=4"]),
    (30, ["no_mfma_fold=1"]), (30, ["mle_per_round=1"]), (30, ["fold_min_chunk=64"]), (30, ["fold_blocks=8192"]),
    (30, ["transcript=device"]),
    (29, []), (29, ["rounds_per_pass=1"]), (29, ["rounds_per_pass=2"]),
], ids=lambda x: x if isinstance(x, int) else ",".join(x) or "default")
def test_plain_sumcheck_at_the_largest_tables_on_every_schedule(n, options):
    _run("mle", n, *options)


@pytest.mark.parametrize("n", [2, 14])
def test_plain_sumcheck_batch_of_65535_tables(n):
    """The most sumchecks one gkr_sumcheck_mle_batch_device call takes; at n = 14, 2^30 - 2^14 values."""
    _run("mle-batch", n)


def test_prove_batch_of_4096_proofs():
    """GKR_MAX_BATCH proofs of the bench's proof-batch circuit in one gkr_prove_batch: every proof's arrays equal the oracle's
    (one digest over the batch), gkr_verify accepts a sample."""
    _run("prove-batch")


@pytest.mark.parametrize("k_i,k", [(28, 12), (28, 14), (20, 24), (28, 24)])
def test_layer_sumcheck_at_the_gate_and_value_limits(k_i, k):
    """2^28 gates on the segment passes (k = 12) and on the wide item passes (k = 14), the widest next layer (2^24 values),
    and both limits at once."""
    _run("layer", k_i, k, timeout=900)


def test_prove_with_an_input_layer_of_2_24_values():
    """gkr_prove of k = [18, 24, 24]: the line restriction and the Moebius transforms at GKR_MAX_K_NEXT; the proof, d and
    input_func against the oracle's digests, and gkr_verify accepts it."""
    _run("prove-wide", timeout=900)


def test_layer_device_transcript_at_its_limit():
    """GKR_TRANSCRIPT_DEVICE at k_next = GKR_MAX_K_NEXT_DEVICE_TRANSCRIPT (dense tables of 2^28 cells): the host
    transcript's bytes and the oracle's."""
    _run("layer-device-transcript", 16, 14)
