"""Independent pure-Python reference for BN254 G2 (the Groth16 B-query).

Fq2 = Fq[u]/(u^2+1) as int pairs (c0, c1), the twist y^2 = x^3 + 3/(9+u),
affine add/double, double-and-add, the EIP-197 128-byte affine encoding
(x.c1 || x.c0 || y.c1 || y.c0, imaginary part first, zeros = identity), the
192-byte Jacobian partial (X || Y || Z, each c1 || c0; Z = 0 = identity),
naive MSM and the gen_points sequence.  Shares nothing with the kernels.
A point is None (identity) or ((x0, x1), (y0, y1)).
"""
P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617

B2 = (19485874751759354771024239261021720505790618469301721065564631296452457478373,
      266929791119991161246907387137283842545076965332900288569378510910307636690)
G2 = ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
       11559732032986387107991004021392285783925812861821192530917403151452391805634),
      (8495653923123431417604973247489272438418190587263600148770280649306958101930,
       4082367875863433681332203403145435568316851327593401208105741076214120093531))
# on the twist, NOT in the r-subgroup
OFF_SUBGROUP = ((1, 0),
                (18278151005453108793778860132295291098363647455926340152056652516292830556603,
                 5912654199736721486680175016176231956195085055698687135131307249486702594212))


def f2_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def f2_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def f2_neg(a):
    return ((-a[0]) % P, (-a[1]) % P)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def f2_inv(a):
    t = pow((a[0] * a[0] + a[1] * a[1]) % P, P - 2, P)
    return (a[0] * t % P, (-a[1] * t) % P)


def on_curve(pt):
    if pt is None:
        return True
    x, y = pt
    return f2_mul(y, y) == f2_add(f2_mul(f2_mul(x, x), x), B2)


def neg(pt):
    return None if pt is None else (pt[0], f2_neg(pt[1]))


def add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if f2_add(p[1], q[1]) == (0, 0):
            return None
        x2 = f2_mul(p[0], p[0])
        lam = f2_mul(f2_add(f2_add(x2, x2), x2), f2_inv(f2_add(p[1], p[1])))
    else:
        lam = f2_mul(f2_sub(q[1], p[1]), f2_inv(f2_sub(q[0], p[0])))
    x = f2_sub(f2_sub(f2_mul(lam, lam), p[0]), q[0])
    return (x, f2_sub(f2_mul(lam, f2_sub(p[0], x)), p[1]))


def _jac_to_affine(p):
    X, Y, Z = p
    if Z == (0, 0):
        return None
    zi = f2_inv(Z)
    zi2 = f2_mul(zi, zi)
    return (f2_mul(X, zi2), f2_mul(Y, f2_mul(zi2, zi)))


def _jac_dbl(p):
    # dbl-2009-l (a = 0) on (X, Y, Z); Z == (0, 0) is the identity
    X, Y, Z = p
    A = f2_mul(X, X)
    B = f2_mul(Y, Y)
    C = f2_mul(B, B)
    t = f2_add(X, B)
    D = f2_sub(f2_sub(f2_mul(t, t), A), C)
    D = f2_add(D, D)
    E = f2_add(f2_add(A, A), A)
    X3 = f2_sub(f2_mul(E, E), f2_add(D, D))
    C8 = f2_add(C, C)
    C8 = f2_add(C8, C8)
    C8 = f2_add(C8, C8)
    return (X3, f2_sub(f2_mul(E, f2_sub(D, X3)), C8), f2_mul(f2_add(Y, Y), Z))


def _jac_add_affine(p, q):
    # Jacobian + affine, textbook form; q is not the identity
    X1, Y1, Z1 = p
    if Z1 == (0, 0):
        return (q[0], q[1], (1, 0))
    Z2 = f2_mul(Z1, Z1)
    U2 = f2_mul(q[0], Z2)
    S2 = f2_mul(q[1], f2_mul(Z2, Z1))
    H = f2_sub(U2, X1)
    Rr = f2_sub(S2, Y1)
    if H == (0, 0):
        if Rr == (0, 0):
            return _jac_dbl(p)
        return ((1, 0), (1, 0), (0, 0))
    H2 = f2_mul(H, H)
    H3 = f2_mul(H2, H)
    V = f2_mul(X1, H2)
    X3 = f2_sub(f2_sub(f2_mul(Rr, Rr), H3), f2_add(V, V))
    Y3 = f2_sub(f2_mul(Rr, f2_sub(V, X3)), f2_mul(Y1, H3))
    return (X3, Y3, f2_mul(Z1, H))


def mul(k, pt):
    """k * pt, left-to-right double-and-add over the integer k >= 0 (no
    reduction); Jacobian inside, one inversion at the end"""
    if pt is None or k == 0:
        return None
    acc = ((1, 0), (1, 0), (0, 0))
    for i in range(k.bit_length() - 1, -1, -1):
        acc = _jac_dbl(acc)
        if (k >> i) & 1:
            acc = _jac_add_affine(acc, pt)
    return _jac_to_affine(acc)


def msm(points, scalars):
    """naive sum k_i * P_i, scalars reduced mod r"""
    acc = None
    for pt, k in zip(points, scalars):
        acc = add(acc, mul(k % R, pt))
    return acc


def in_subgroup(pt):
    return mul(R, pt) is None


def gen_points(start, n):
    """P_i = (start + i + 1) * G2"""
    out = []
    cur = mul(start + 1, G2)
    for _ in range(n):
        out.append(cur)
        cur = add(cur, G2)
    return out


# ---- encodings ----

def _f2_bytes(a):
    return a[1].to_bytes(32, "big") + a[0].to_bytes(32, "big")  # c1 || c0


def _f2_parse(b):
    return (int.from_bytes(b[32:64], "big"), int.from_bytes(b[0:32], "big"))


def encode(pt):
    if pt is None:
        return b"\x00" * 128
    return _f2_bytes(pt[0]) + _f2_bytes(pt[1])


def decode(b):
    assert len(b) == 128
    if b == b"\x00" * 128:
        return None
    return (_f2_parse(b[0:64]), _f2_parse(b[64:128]))


def encode_many(points):
    return b"".join(encode(p) for p in points)


def decode_many(b):
    return [decode(b[i:i + 128]) for i in range(0, len(b), 128)]


def encode_jac(pt):
    """a valid 192-byte Jacobian partial of pt (Z = 1)"""
    if pt is None:
        return b"\x00" * 192
    return _f2_bytes(pt[0]) + _f2_bytes(pt[1]) + _f2_bytes((1, 0))


def decode_jac(b):
    assert len(b) == 192
    X, Y, Z = _f2_parse(b[0:64]), _f2_parse(b[64:128]), _f2_parse(b[128:192])
    return _jac_to_affine((X, Y, Z))


def scalars_bytes(ks):
    return b"".join(k.to_bytes(32, "big") for k in ks)


def scalars_ints(b):
    return [int.from_bytes(b[i:i + 32], "big") for i in range(0, len(b), 32)]
