"""Test-side reference for the R1CS evaluation (DESIGN.md "R1CS
evaluation"), shared by test_r1cs_reference.py (CPU) and test_gpu_r1cs.py
(GPU): a Python-integer sparse matrix-vector product, independent of the
library and of ethrex_amd/r1cs.py's witness pass, and CSR byte helpers.
"""
# BN254 scalar field modulus
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001


def spmv(row_offs, cols, coeffs, z, n=None):
    """y_i = sum over the entries of row i of coeff * z[col] mod R; rows
    past the matrix, up to n, are zero"""
    rows = len(row_offs) - 1
    y = []
    for i in range(rows):
        acc = 0
        for e in range(row_offs[i], row_offs[i + 1]):
            acc += coeffs[e] * z[cols[e]]
        y.append(acc % R)
    if n is not None:
        assert rows <= n
        y += [0] * (n - rows)
    return y


def to_bytes(values):
    return b"".join(v.to_bytes(32, "big") for v in values)


def to_ints(b):
    return [int.from_bytes(b[i:i + 32], "big") for i in range(0, len(b), 32)]


def csr_from_rows(rows):
    """rows: a list of rows, each a list of (col, coeff) -> (row_offs,
    cols, coeffs)"""
    offs, cols, coeffs = [0], [], []
    for row in rows:
        for col, co in row:
            cols.append(col)
            coeffs.append(co)
        offs.append(len(cols))
    return offs, cols, coeffs
