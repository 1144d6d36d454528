"""Test-side reference for the coset NTT and the Groth16 quotient
polynomial (DESIGN.md "Quotient polynomial"), shared by
test_quotient_reference.py (CPU) and test_gpu_quotient.py (GPU).

Python integers for g^(+-i), d and the pointwise step; oracle.fr_ntt for
the transforms.  The naive_* versions are pure-Python O(n^2) DFTs (n <= 16)
that pin this reference itself.
"""
import oracle

# BN254 scalar field modulus
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
# the coset generator: the multiplicative generator of Fr
G = 5
# 2^28-th root of unity, 5^((r-1)/2^28) (oracle/gen_constants.py)
W28 = pow(5, (R - 1) >> 28, R)


def to_ints(b):
    return [int.from_bytes(b[i:i + 32], "big") for i in range(0, len(b), 32)]


def to_bytes(v):
    return b"".join(x.to_bytes(32, "big") for x in v)


def root(n):
    """the library's n-th root W28^(2^(28-k)), n = 2^k"""
    k = n.bit_length() - 1
    assert n == 1 << k and k <= 28
    return pow(W28, 1 << (28 - k), R)


def _ntt(v, inverse):
    rc, out = oracle.fr_ntt(to_bytes(v), len(v), inverse)
    assert rc == 0
    return to_ints(out)


def intt(v):
    return _ntt(v, True)


def _powers(base, n):
    out, acc = [], 1
    for _ in range(n):
        out.append(acc)
        acc = acc * base % R
    return out


def coset_fwd(v):
    """A_j = sum_i a_i g^i w^(ij)"""
    return _ntt([x * p % R for x, p in zip(v, _powers(G, len(v)))], False)


def coset_inv(v):
    """a_i = g^-i n^-1 sum_j A_j w^(-ij)"""
    ginv = pow(G, R - 2, R)
    return [x * p % R for x, p in zip(_ntt(v, True), _powers(ginv, len(v)))]


def quotient(a, b, c):
    """h from three evaluation vectors (lists of ints), n coefficients"""
    n = len(a)
    d = pow(pow(G, n, R) - 1, R - 2, R)
    ab, bb, cb = (coset_fwd(intt(x)) for x in (a, b, c))
    return coset_inv([(x * y - z) * d % R for x, y, z in zip(ab, bb, cb)])


# ---- naive O(n^2) restatement (n <= 16) ----

def _naive_dft(v, w):
    n = len(v)
    return [sum(v[i] * pow(w, i * j, R) for i in range(n)) % R
            for j in range(n)]


def naive_coset_fwd(v):
    n = len(v)
    return _naive_dft([v[i] * pow(G, i, R) % R for i in range(n)], root(n))


def naive_coset_inv(v):
    n = len(v)
    ninv, ginv = pow(n, R - 2, R), pow(G, R - 2, R)
    t = _naive_dft(v, pow(root(n), R - 2, R))
    return [t[i] * ninv % R * pow(ginv, i, R) % R for i in range(n)]


def naive_intt(v):
    n = len(v)
    ninv = pow(n, R - 2, R)
    return [x * ninv % R for x in _naive_dft(v, pow(root(n), R - 2, R))]


def naive_quotient(a, b, c):
    n = len(a)
    assert n <= 16
    d = pow(pow(G, n, R) - 1, R - 2, R)
    ab, bb, cb = (naive_coset_fwd(naive_intt(x)) for x in (a, b, c))
    return naive_coset_inv([(x * y - z) * d % R
                            for x, y, z in zip(ab, bb, cb)])


# ---- the evaluation identity, independent of any coset code ----

def horner(coeffs, x):
    acc = 0
    for co in reversed(coeffs):
        acc = (acc * x + co) % R
    return acc


def identity_holds(a, b, c, h, x):
    """A(x) B(x) - C(x) == H(x) (x^n - 1), A/B/C the interpolants"""
    n = len(a)
    lhs = (horner(intt(a), x) * horner(intt(b), x) - horner(intt(c), x)) % R
    return lhs == horner(h, x) * (pow(x, n, R) - 1) % R
