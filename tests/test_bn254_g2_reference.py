"""The pure-Python BN254 G2 reference checks itself, and the committed
constants header is checked against its generator and against the values.
"""
import importlib.util
import os
import re

import bn254_g2_reference as g2

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "ethrex_amd", "csrc", "bn254_g2_constants_dev.h")
GEN = os.path.join(REPO, "ethrex_amd", "tools", "gen_g2_constants.py")


def test_twist_constant():
    assert g2.f2_mul(g2.B2, (9, 1)) == (3, 0)


def test_generator():
    assert g2.on_curve(g2.G2)
    assert g2.mul(g2.R, g2.G2) is None
    assert g2.mul(g2.R - 1, g2.G2) == g2.neg(g2.G2)


def test_off_subgroup_point():
    assert g2.OFF_SUBGROUP[0] == (1, 0)
    assert g2.on_curve(g2.OFF_SUBGROUP)
    assert not g2.in_subgroup(g2.OFF_SUBGROUP)


def test_group_law_small():
    G = g2.G2
    assert g2.add(G, g2.neg(G)) is None
    assert g2.add(G, None) == G and g2.add(None, G) == G
    assert g2.add(G, G) == g2.mul(2, G)
    assert g2.add(g2.mul(2, G), G) == g2.mul(3, G)
    assert g2.add(g2.mul(12345, G), g2.mul(g2.R - 12345, G)) is None
    pts = g2.gen_points(5, 4)
    assert pts[0] == g2.mul(6, G) and pts[3] == g2.mul(9, G)


def test_encodings():
    pt = g2.mul(7, g2.G2)
    b = g2.encode(pt)
    assert len(b) == 128 and g2.decode(b) == pt
    # imaginary part first
    assert int.from_bytes(b[0:32], "big") == pt[0][1]
    assert int.from_bytes(b[32:64], "big") == pt[0][0]
    assert int.from_bytes(b[64:96], "big") == pt[1][1]
    assert int.from_bytes(b[96:128], "big") == pt[1][0]
    assert g2.encode(None) == b"\x00" * 128 and g2.decode(b"\x00" * 128) is None
    j = g2.encode_jac(pt)
    assert len(j) == 192 and g2.decode_jac(j) == pt
    assert g2.decode_jac(b"\x00" * 192) is None
    # a non-trivial Z: (X, Y, Z) = (x z^2, y z^3, z)
    z = (3, 5)
    z2 = g2.f2_mul(z, z)
    X, Y = g2.f2_mul(pt[0], z2), g2.f2_mul(pt[1], g2.f2_mul(z2, z))
    raw = g2._f2_bytes(X) + g2._f2_bytes(Y) + g2._f2_bytes(z)
    assert g2.decode_jac(raw) == pt
    ks = [0, 1, g2.R - 1, (1 << 256) - 1]
    assert g2.scalars_ints(g2.scalars_bytes(ks)) == ks


def test_msm_is_sum_of_muls():
    pts = g2.gen_points(0, 5) + [None]
    ks = [3, 0, g2.R - 1, g2.R + 2, (1 << 256) - 1, 9]
    acc = None
    for p, k in zip(pts, ks):
        acc = g2.add(acc, g2.mul(k % g2.R, p))
    assert g2.msm(pts, ks) == acc
    # (3*1 + 0 - 3 + 2*4 + k4*5) * G
    k = (3 - 3 + 8 + (((1 << 256) - 1) % g2.R) * 5) % g2.R
    assert acc == g2.mul(k, g2.G2)


def _gen_module():
    spec = importlib.util.spec_from_file_location("gen_g2_constants", GEN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_constants_header_matches_generator():
    with open(HEADER) as f:
        assert f.read() == _gen_module().emit()


def test_constants_header_values():
    with open(HEADER) as f:
        text = f.read()
    rinv = pow(1 << 261, -1, g2.P)

    def limbs(name):
        m = re.search(r"\b%s\[9\] = \{([^}]*)\}" % name, text)
        vals = [int(x.strip().rstrip("u"), 16) for x in m.group(1).split(",")]
        assert len(vals) == 9 and all(v < (1 << 29) for v in vals)
        mont = sum(v << (29 * i) for i, v in enumerate(vals))
        assert mont < g2.P
        return mont * rinv % g2.P

    assert (limbs("FQ9_G2_B0"), limbs("FQ9_G2_B1")) == g2.B2
    assert (limbs("FQ9_G2_GX0"), limbs("FQ9_G2_GX1")) == g2.G2[0]
    assert (limbs("FQ9_G2_GY0"), limbs("FQ9_G2_GY1")) == g2.G2[1]
    m = re.search(r"G2_ORDER\[4\] = \{([^}]*)\}", text)
    words = [int(x.strip().rstrip("ul"), 16) for x in m.group(1).split(",")]
    assert sum(w << (64 * i) for i, w in enumerate(words)) == g2.R
