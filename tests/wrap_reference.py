"""Test-side restatement of "wrap vector v1" (DESIGN.md), shared by
test_wrap_vector.py (CPU) and test_gpu_wrap_binding.py (GPU).

Written independently of ethrex_amd.witness.wrap_vector: it goes through
padded byte strings and struct unpacking, keeps the raw (unreduced) values,
and shares only ethrex_amd.keccak.keccak_f1600 / keccak256, which the
canonical Keccak-256 vectors pin.
"""
import struct

from ethrex_amd.keccak import keccak256, keccak_f1600

# BN254 scalar field modulus
R_BN254 = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001


def ref_root(digests):
    level = list(digests)
    assert level
    while len(level) > 1:
        odd = level[-1] if len(level) % 2 else None
        level = [keccak256(a + b) for a, b in zip(level[0::2], level[1::2])]
        if odd is not None:
            level.append(odd)
    return level[0]


def ref_messages(digests, domain, n):
    """the 112-byte block messages M_j, j < ceil(n/4)"""
    m = len(digests)
    root = ref_root(digests)
    return [domain + root + struct.pack("<QQ", m, j) + digests[j % m]
            for j in range(-(-n // 4))]


def ref_squeeze(msg):
    """one rate-136 absorb of a 112-byte message with the original Keccak
    padding, one permutation, first 128 state bytes"""
    assert len(msg) == 112
    padded = msg + b"\x01" + b"\x00" * 22 + b"\x80"
    state = list(struct.unpack("<17Q", padded)) + [0] * 8
    keccak_f1600(state)
    return struct.pack("<16Q", *state[:16])


def ref_raw(digests, domain, n):
    """the n unreduced 256-bit integers (big-endian reading of each
    32-byte slice of the squeezed blocks)"""
    raw = []
    for msg in ref_messages(digests, domain, n):
        s = ref_squeeze(msg)
        raw += [int.from_bytes(s[k:k + 32], "big") for k in range(0, 128, 32)]
    return raw[:n]


def ref_vector(digests, domain, n):
    """n x 32-byte big-endian canonical elements"""
    return b"".join((v % R_BN254).to_bytes(32, "big")
                    for v in ref_raw(digests, domain, n))
