"""CPU checks of the quotient reference (quotient_reference.py) that the
GPU parity tests lean on, and of witness.quotient_domain_b."""
import random

import pytest

import quotient_reference as Q
from quotient_reference import R


def _rand(rng, n):
    return [rng.randrange(R) for _ in range(n)]


def test_constants():
    assert pow(Q.W28, 1 << 28, R) == 1 and pow(Q.W28, 1 << 27, R) == R - 1
    # g^(2^k) != 1 for every k <= 28, so (g^n - 1) is invertible
    assert all(pow(Q.G, 1 << k, R) != 1 for k in range(29))


@pytest.mark.parametrize("n", [1, 2, 4, 16])
def test_fast_and_naive_agree(n):
    rng = random.Random(n)
    a, b, c = _rand(rng, n), _rand(rng, n), _rand(rng, n)
    assert Q.intt(a) == Q.naive_intt(a)
    assert Q.coset_fwd(a) == Q.naive_coset_fwd(a)
    assert Q.coset_inv(a) == Q.naive_coset_inv(a)
    assert Q.coset_inv(Q.coset_fwd(a)) == a
    assert Q.quotient(a, b, c) == Q.naive_quotient(a, b, c)
    sat = [x * y % R for x, y in zip(a, b)]
    assert Q.quotient(a, b, sat) == Q.naive_quotient(a, b, sat)


@pytest.fixture(scope="module")
def sat_1024():
    n = 1 << 10
    rng = random.Random(1024)
    a, b = _rand(rng, n), _rand(rng, n)
    c = [x * y % R for x, y in zip(a, b)]
    return a, b, c, rng.randrange(R)


def test_satisfied_system(sat_1024):
    a, b, c, x = sat_1024
    h = Q.quotient(a, b, c)
    assert h[-1] == 0
    assert Q.identity_holds(a, b, c, h, x)


def test_tampered_c_breaks_both(sat_1024):
    a, b, c, x = sat_1024
    bad = list(c)
    bad[17] = (bad[17] + 1) % R
    h = Q.quotient(a, b, bad)
    assert h[-1] != 0
    assert not Q.identity_holds(a, b, bad, h, x)


def test_quotient_domain_b():
    from ethrex_amd import witness
    from ethrex_amd.keccak import keccak256
    com = bytes(range(32))
    want = keccak256(com + b"ethrex_amd/quotient/b/v1")
    assert witness.quotient_domain_b(com) == want
    assert want != com and len(want) == 32
    with pytest.raises(ValueError):
        witness.quotient_domain_b(com[:31])
