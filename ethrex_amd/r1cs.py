"""Product-chain circuit v1: a deterministic, satisfiable synthetic R1CS.

Used by Mi355Backend(composition="r1cs") and by the tests as a constraint
system whose A z, B z, C z really satisfy (A z) (.) (B z) = C z, with the
sparsity of a real circuit (a few entries per row, mostly +-1 coefficients,
every row reaching back into earlier wires).

Definition.  Parameters (n_cons, k, fan_in, seed); all arithmetic mod the
BN254 scalar field modulus R.

  variables   m = 1 + k + n_cons:  z[0] = 1, z[1..k] the free inputs,
              z[1+k+i] = (A_i . z) * (B_i . z)   for i = 0 .. n_cons-1
  constraint  row i of A and of B has fan_in entries with columns in
              [0, 1+k+i) — only wires that exist before wire 1+k+i, so z is
              computed in one forward pass; a column may repeat in a row.
              Row i of C is the single entry (1+k+i, coefficient 1).

Draw order (this fixes the bytes).  rng = random.Random(seed); for i = 0 ..
n_cons-1, for the matrix A then B, for j = 0 .. fan_in-1:
    col = rng.randrange(1 + k + i)
    u   = rng.randrange(16)
    coeff = 1                      if u < 7        (7/16)
            R - 1                  if 7 <= u < 11  (4/16)
            rng.randrange(2, 17)   if 11 <= u < 14 (3/16, small integers)
            rng.randrange(R)       otherwise       (2/16, full width)
No other draw is made.  random.Random(int) and randrange are specified by
CPython (MT19937 + rejection sampling over getrandbits) and stable across
Python 3 releases.
"""
import random

# BN254 scalar field modulus
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001

VERSION = 1


def _coeff(rng):
    u = rng.randrange(16)
    if u < 7:
        return 1
    if u < 11:
        return R - 1
    if u < 14:
        return rng.randrange(2, 17)
    return rng.randrange(R)


def chain_circuit(n_cons: int, k: int, fan_in: int, seed: int):
    """-> ((A, B, C), witness): each matrix a CSR triple (row_offs, cols,
    coeffs) of Python integers with n_cons rows over m = 1 + k + n_cons
    columns; witness(inputs) maps the k free inputs to the full vector z
    (a list of m integers) that satisfies the system."""
    if n_cons < 0 or k < 0 or fan_in < 1:
        raise ValueError("chain_circuit: need n_cons >= 0, k >= 0, fan_in >= 1")
    rng = random.Random(seed)
    a = ([0], [], [])
    b = ([0], [], [])
    c = ([0], [], [])
    for i in range(n_cons):
        avail = 1 + k + i
        for offs, cols, coeffs in (a, b):
            for _ in range(fan_in):
                cols.append(rng.randrange(avail))
                coeffs.append(_coeff(rng))
            offs.append(len(cols))
        c[1].append(avail)
        c[2].append(1)
        c[0].append(i + 1)

    def witness(inputs):
        if len(inputs) != k:
            raise ValueError(f"chain_circuit: need {k} free inputs")
        z = [1] + [x % R for x in inputs]
        for i in range(n_cons):
            lo, hi = i * fan_in, (i + 1) * fan_in
            az = sum(co * z[cl] for cl, co in
                     zip(a[1][lo:hi], a[2][lo:hi])) % R
            bz = sum(co * z[cl] for cl, co in
                     zip(b[1][lo:hi], b[2][lo:hi])) % R
            z.append(az * bz % R)
        return z

    return (a, b, c), witness


def fr_bytes(values) -> bytes:
    """integers -> 32-byte big-endian elements, concatenated"""
    return b"".join(v.to_bytes(32, "big") for v in values)
