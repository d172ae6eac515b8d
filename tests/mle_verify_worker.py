"""Child process of tests/test_gpu_mle_verify.py: the plain sumcheck's verifier on ONE table at a size limit (n = 28: the first n
at which the streaming kernel's 32 source streams reach byte offsets past 2^32; n = 30: GKR_MAX_MLE_N), in a process of its own
like tests/limits_worker.py.  The table is filled on the device, proven, verified (accept), its last entry overwritten through
gkr_device_upload and the same transcript verified again (EVALUATION at round n).  Prints the wall times and OK, or what went wrong.

    python mle_verify_worker.py <n>"""
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gkr_amd import Context, synth  # noqa: E402
from gkr_amd import _native as N  # noqa: E402


def main():
    n = int(sys.argv[1])
    count = 1 << n
    bad = None
    with Context(0) as ctx:
        d = ctx.alloc(count * 32)
        try:
            ctx.fill_table(d, count, synth.SEED + 2)
            t = time.time()
            C, L, R = ctx.sumcheck_mle_batch_device(d, n, 1)
            t_prove = time.time() - t
            t = time.time()
            accept, rnd, check, claims = ctx.verify_sumcheck_batch_device(d, n, 1, C, L, R)
            t_verify = time.time() - t
            print("n = %d: prove %.2f s, verify %.2f s" % (n, t_prove, t_verify))
            if (bool(accept[0]), int(rnd[0]), int(check[0])) != (True, 0, 0):
                bad = "the honest transcript: (%s, %d, %d)" % (accept[0], rnd[0], check[0])
            again = ctx.verify_sumcheck_batch_device(d, n, 1, C, L, R, claims=claims)
            if not bad and (bool(again[0][0]), int(again[1][0]), int(again[2][0])) != (True, 0, 0):
                bad = "the honest transcript with its own sum as the claim: (%s, %d, %d)" % (again[0][0], again[1][0], again[2][0])
            # the last entry of the table, one more: one 32-byte upload at the table's end (byte offset 32 * (2^n - 1))
            last = ctx.download(ctypes.c_void_p(d.value + 32 * (count - 1)), (1, 4))
            last[0, 0] ^= np.uint64(1)
            ctx.upload(ctypes.c_void_p(d.value + 32 * (count - 1)), last)
            accept, rnd, check, _ = ctx.verify_sumcheck_batch_device(d, n, 1, C, L, R, claims=claims)
            if not bad and (bool(accept[0]), int(rnd[0]), int(check[0])) != (False, n, N.GKR_VERIFY_EVALUATION):
                bad = "the last entry changed: (%s, %d, %d)" % (accept[0], rnd[0], check[0])
        finally:
            ctx.free(d)
    print(bad if bad else "OK")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
