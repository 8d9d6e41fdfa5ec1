"""The shared rules of a Levenberg-Marquardt step (csrc/relax_lm_rules.hpp: the quaternion step and normalisation, the
Jacobi scale, the clamped damping diagonal, the trust-region bookkeeping) on the host, without a device: a small program
(tests/lm_rules_driver.cpp) that includes only that header, built with the system g++ under the address and
undefined-behaviour sanitizers (host code only, a process of its own).  It checks the quaternion step against long double
(32 * 2^-53 per component), the normalisation against q / sqrt(n2) to the bit with a zero quaternion left alone, the clamp
and the scale against their defining expressions with NaN passing through, and lm_trust to the bit against a transcription
of the trust-region lines lm_solve had before the rules were shared, over 10 000 random sequences of accepted, rejected and
invalid steps."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "lm_rules_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("lm_rules")), "lm_rules_driver")
    # (-ffp-contract=off: the library's flag; the expressions are compared to the bit)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, SRC], check=True)
    return exe


@pytest.mark.parametrize("what", ["quat_plus", "quat_normalize", "diagonal", "trust"])
def test_lm_rules(driver, what):
    r = subprocess.run([driver, what], capture_output=True, text=True, timeout=240)
    print(r.stdout[-2000:])
    print(r.stderr[-4000:])
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    assert "FAIL" not in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr
    assert r.stdout.strip().splitlines()[-1] == "ok " + what
