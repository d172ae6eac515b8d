"""The host side of the flag-in-word records that streaming passes of the plain sumcheck publish (gkr_amd/csrc/flagged_rec.h:
a 64-bit word is {data limb, ticket}, valid only with the expected ticket).  tests/flagged_rec_stress.cpp is a stand-alone program:
a writer thread fills records word by word in shuffled order with pauses, the reader polls with a cursor per table as the driver
does.  It checks that no table is totalled early, that the sums are those of a plain big-integer addition (random limbs, all-ones
limbs for the carries, all-zero data), stale tickets of earlier rounds, that ticket 0 is never issued, that a record left with one
old word never validates, and the 32-bit wrap of the ticket counter.  Built and run under ASan + UBSan and under TSan."""

import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.mark.parametrize("name,flags", [("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]),
                                        ("tsan", ["-fsanitize=thread"])])
def test_flagged_records_reader_against_writer(tmp_path, name, flags):
    exe = str(tmp_path / ("flagged_rec_stress_" + name))
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-pthread", "-Wall", *flags,
                           "-I", os.path.join(REPO, "gkr_amd", "csrc"), os.path.join(HERE, "flagged_rec_stress.cpp"), "-o", exe])
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout + out.stderr[-3000:]
    assert "Sanitizer" not in out.stderr, out.stderr[-3000:]
