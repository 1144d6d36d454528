"""GPU parity for the radix-2^3 row kernels (EM_NTT_R8=1), which the default
radix-2^2 dispatch never launches.  The variable is read once per process,
so each case runs in a fresh child that prints one SHA-256 per transform;
the parent compares against the test-side reference (quotient_reference.py),
not against the default kernels.

Sizes: 2^13, 2^14 and 2^16 give rows of (2^7, 2^6), (2^7, 2^7) and
(2^8, 2^8) — the three residues of logM mod 3: no tail, radix-2 tail and
radix-2^2 tail.
"""
import functools
import hashlib
import os
import random
import subprocess
import sys

import pytest

import quotient_reference as Q
from quotient_reference import R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# one line per (size, coset, inverse), in this order
_CHILD = r"""
import hashlib, random, sys
import ethrex_amd as ea
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
ea.set_device(0)
for log2 in map(int, sys.argv[1:]):
    n = 1 << log2
    rng = random.Random(300 + n)
    x = b"".join(rng.randrange(R).to_bytes(32, "big") for _ in range(n))
    plan = ea.NttPlan(n)
    for coset in (0, 1):
        for inverse in (False, True):
            plan.upload(x)
            (plan.run_coset if coset else plan.run)(inverse)
            print(n, coset, int(inverse),
                  hashlib.sha256(plan.download()).hexdigest())
    plan.destroy()
"""


@pytest.fixture(scope="module")
def gpu():
    import ethrex_amd
    if ethrex_amd.device_count() < 1:
        pytest.skip("no GPU")
    return ethrex_amd


@functools.lru_cache(maxsize=None)
def _want(log2):
    n = 1 << log2
    rng = random.Random(300 + n)
    x = [rng.randrange(R) for _ in range(n)]
    refs = {(0, 0): Q._ntt(x, False), (0, 1): Q._ntt(x, True),
            (1, 0): Q.coset_fwd(x), (1, 1): Q.coset_inv(x)}
    return [[str(n), str(coset), str(inverse),
             hashlib.sha256(Q.to_bytes(refs[coset, inverse])).hexdigest()]
            for coset in (0, 1) for inverse in (0, 1)]


def _run_child(log2s, **extra_env):
    env = dict(os.environ, **extra_env)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run([sys.executable, "-c", _CHILD] + [str(k) for k in log2s],
                         env=env, cwd=REPO, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    return [ln.split() for ln in out.stdout.strip().splitlines()]


def test_radix8_rows_match_reference(gpu):
    """EM_NTT_R8=1: plain and coset transforms, both directions, at the
    three row-length residues mod 3."""
    got = _run_child((13, 14, 16), EM_NTT_R8="1")
    assert got == [ln for k in (13, 14, 16) for ln in _want(k)]


def test_radix8_rows_unfused_coset_match_reference(gpu):
    """EM_NTT_R8=1 with EM_NTT_COSET_UNFUSED=1: the plain radix-2^3 kernel
    under the standalone coset scaling pass."""
    got = _run_child((13,), EM_NTT_R8="1", EM_NTT_COSET_UNFUSED="1")
    assert got == _want(13)
