"""Wrap vector v1 — the host definition, CPU only.

witness.wrap_vector is the product's pure-Python restatement of the device
expansion (NttPlan.fill_from_digests); here it is pinned against the
test-side restatement in wrap_reference.py, a committed golden, and the
properties the definition promises.
"""
import hashlib

import pytest

from ethrex_amd import witness
from ethrex_amd.keccak import keccak256
from wrap_reference import (R_BN254, ref_messages, ref_raw, ref_root,
                            ref_vector)

CASES = [(1, 1), (1, 4), (3, 2), (3, 64), (5, 64)]
DOMAIN = bytes(range(32))


def _digests(m, tag=b"wrap"):
    return [keccak256(tag + bytes([i])) for i in range(m)]


@pytest.mark.parametrize("m,n", CASES)
def test_wrap_vector_matches_restatement(m, n):
    hs = _digests(m)
    got = witness.wrap_vector(hs, DOMAIN, n)
    assert len(got) == 32 * n
    assert got == ref_vector(hs, DOMAIN, n)


@pytest.mark.parametrize("m,n", CASES)
def test_first_element_is_keccak256_of_block_message(m, n):
    """S_j[:32] == keccak256(M_j): e_{4j} is the block message's ordinary
    keccak256 digest read big-endian, before reduction"""
    hs = _digests(m)
    raw = ref_raw(hs, DOMAIN, n)
    msgs = ref_messages(hs, DOMAIN, n)
    assert len(msgs) == (n + 3) // 4
    for j, msg in enumerate(msgs):
        assert len(msg) == 112
        assert raw[4 * j].to_bytes(32, "big") == keccak256(msg)


@pytest.mark.parametrize("m,n", CASES)
def test_elements_canonical_and_reduction_exercised(m, n):
    hs = _digests(m)
    vec = witness.wrap_vector(hs, DOMAIN, n)
    elems = [int.from_bytes(vec[32 * i:32 * i + 32], "big") for i in range(n)]
    assert all(e < R_BN254 for e in elems)
    raw = ref_raw(hs, DOMAIN, n)
    assert elems == [v % R_BN254 for v in raw]
    if n >= 64:
        # r / 2^256 ~ 0.189: with 64 raw values a case without any value
        # >= r has probability 0.189^64 — the reduction must be exercised
        assert any(v >= R_BN254 for v in raw)
        # and more than one subtraction of r is needed somewhere
        assert any(v >= 2 * R_BN254 for v in raw)


def test_wrap_vector_golden():
    """sha256 of the (m=3, n=8) vector, produced by wrap_reference"""
    hs = [bytes([0x11 * (i + 1)]) * 32 for i in range(3)]
    want = ("e6412d436c7c014e7609aa76b099f454"
            "700f84cfa6106d9cf2cd3d1968d1a1c6")
    assert hashlib.sha256(ref_vector(hs, DOMAIN, 8)).hexdigest() == want
    assert hashlib.sha256(
        witness.wrap_vector(hs, DOMAIN, 8)).hexdigest() == want


def test_digest_count_is_bound():
    """[a, b, c] and [keccak256(a || b), c] share the tree root; the
    vectors still differ because m (and the per-block digest) is bound"""
    a, b, c = _digests(3)
    ab = keccak256(a + b)
    assert ref_root([a, b, c]) == ref_root([ab, c])
    assert witness.wrap_root([a, b, c]) == witness.wrap_root([ab, c])
    v3 = witness.wrap_vector([a, b, c], DOMAIN, 8)
    v2 = witness.wrap_vector([ab, c], DOMAIN, 8)
    assert v3 != v2
    # block 1 (elements 4..7) differs as well, not only block 0
    assert v3[128:] != v2[128:]


def test_every_digest_and_the_domain_are_bound():
    hs = _digests(5)
    base = witness.wrap_vector(hs, DOMAIN, 4)   # one block: uses hs[0] only
    for i in range(5):
        mod = list(hs)
        mod[i] = keccak256(b"other" + bytes([i]))
        assert witness.wrap_vector(mod, DOMAIN, 4) != base, i
    assert witness.wrap_vector(hs, bytes(32), 4) != base


def test_wrap_vector_rejects_bad_input():
    hs = _digests(2)
    with pytest.raises(ValueError):
        witness.wrap_vector([], DOMAIN, 4)
    with pytest.raises(ValueError):
        witness.wrap_vector(hs, DOMAIN, 3)
    with pytest.raises(ValueError):
        witness.wrap_vector(hs, DOMAIN[:31], 4)
