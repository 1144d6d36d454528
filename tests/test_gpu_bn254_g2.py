"""GPU parity for BN254 G2 (the Groth16 B-query): the gfx950 Fq2/G2 path
through the C-ABI, bit-exact against the pure-Python reference
(tests/bn254_g2_reference.py).  EIP-197 byte semantics: 128-byte points,
imaginary part first, canonical coordinates, subgroup-checked mul/msm/upload.
"""
import pytest

import bn254_g2_reference as g2

pytestmark = pytest.mark.gpu

R = g2.R
ZERO = b"\x00" * 128


@pytest.fixture(scope="module")
def gpu():
    import ethrex_amd
    if ethrex_amd.device_count() < 1:
        pytest.skip("no GPU")
    ethrex_amd.set_device(0)
    return ethrex_amd


@pytest.fixture(scope="module")
def base256(gpu):
    """256 reference points (i+1)*G2, gen_fr scalars and the per-point
    products k_i * P_i, computed once and never modified"""
    pts = tuple(g2.gen_points(0, 256))
    ks = tuple(g2.scalars_ints(gpu.gen_fr(61, 256)))
    prods = tuple(g2.mul(k % R, p) for p, k in zip(pts, ks))
    return pts, ks, prods


def _sum(points):
    acc = None
    for p in points:
        acc = g2.add(acc, p)
    return acc


def _identity_expected(ks, start):
    """MSM over P_i = (start+i+1)*G2 is (sum k_i (start+i+1) mod r) * G2"""
    s = 0
    for i, k in enumerate(ks):
        s = (s + (k % R) * (start + i + 1)) % R
    return g2.encode(g2.mul(s, g2.G2))


def test_gen_points(gpu):
    for start in (0, 5):
        plan = gpu.Bn254G2MsmPlan(64)
        plan.gen_points(start)
        got = plan.download_points()
        plan.destroy()
        assert got == g2.encode_many(g2.gen_points(start, 64)), start


def test_add(gpu):
    G = g2.G2
    P2, P3 = g2.mul(2, G), g2.mul(3, G)
    cases = [(G, P2, P3),                 # G + 2G
             (P3, P3, g2.mul(6, G)),      # doubling
             (P3, None, P3), (None, P3, P3),
             (None, None, None),
             (P3, g2.neg(P3), None)]      # cancel
    for a, b, want in cases:
        rc, got = gpu.bn254_g2_add(g2.encode(a), g2.encode(b))
        assert rc == 0 and got == g2.encode(want)


def test_mul(gpu):
    P = g2.mul(3, g2.G2)
    for k in (0, 1, 2, 7, 255, R - 1, R, R + 5, (1 << 256) - 1):
        rc, got = gpu.bn254_g2_mul(g2.encode(P), k.to_bytes(32, "big"))
        assert rc == 0, hex(k)
        assert got == g2.encode(g2.mul(k % R, P)), hex(k)
    rc, got = gpu.bn254_g2_mul(ZERO, (5).to_bytes(32, "big"))
    assert rc == 0 and got == ZERO


def test_msm_one_shot(gpu, base256):
    pts, ks, prods = base256
    for n in (1, 2, 100, 256):
        rc, got = gpu.bn254_g2_msm(g2.encode_many(pts[:n]),
                                   g2.scalars_bytes(ks[:n]), n)
        assert rc == 0, n
        assert got == g2.encode(_sum(prods[:n])), n


def test_msm_one_shot_special(gpu, base256):
    """identity point, zero scalar, a duplicated point with equal scalars
    (same bucket in every window: the doubling branch) and a P / -P pair
    with equal scalars (the cancel branch)"""
    pts, ks, prods = base256
    pts, ks, prods = list(pts), list(ks), list(prods)
    pts[3], prods[3] = None, None
    ks[5], prods[5] = 0, None
    pts[11], ks[11], prods[11] = pts[10], ks[10], prods[10]
    pts[21], ks[21], prods[21] = g2.neg(pts[20]), ks[20], g2.neg(prods[20])
    rc, got = gpu.bn254_g2_msm(g2.encode_many(pts), g2.scalars_bytes(ks), 256)
    assert rc == 0
    assert got == g2.encode(_sum(prods))


def test_msm_plan_4096_c8(gpu):
    n = 4096
    plan = gpu.Bn254G2MsmPlan(n)
    plan.gen_points(3)
    scs = gpu.gen_fr(62, n)
    plan.upload_scalars(scs)
    got = plan.run()
    plan.destroy()
    assert got == _identity_expected(g2.scalars_ints(scs), 3)


def test_msm_plan_2_17_signed_c17(gpu):
    """n = 2^17 is the smallest n on the signed c=17 path; the first scalars
    exercise digit carry and the top window"""
    n = 1 << 17
    ks = g2.scalars_ints(gpu.gen_fr(63, n))
    special = [0, 1, R - 1, 1 << 16, (1 << 16) + 1, (1 << 17) - 1, 1 << 17,
               1 << 253, (1 << 253) - 1]
    ks[:len(special)] = special
    plan = gpu.Bn254G2MsmPlan(n)
    plan.gen_points(0)
    plan.upload_scalars(g2.scalars_bytes(ks))
    got = plan.run()
    t = plan.last_times()
    plan.destroy()
    assert got == _identity_expected(ks, 0)
    assert t["bucket_acc_ms"] > 0 and t["total_ms"] >= t["bucket_acc_ms"]


def test_run_async_equals_run(gpu):
    n = 2048
    plan = gpu.Bn254G2MsmPlan(n)
    plan.gen_points(0)
    scs = gpu.gen_fr(64, n)
    plan.upload_scalars(scs)
    want = plan.run()
    for _ in range(3):
        plan.run_async()
    got = plan.sync()
    plan.destroy()
    assert want == _identity_expected(g2.scalars_ints(scs), 0)
    assert got == want


def test_run_partial_halves(gpu):
    n = 512
    scs = gpu.gen_fr(65, n)
    full = gpu.Bn254G2MsmPlan(n)
    full.gen_points(0)
    full.upload_scalars(scs)
    want = full.run()
    full.destroy()
    acc = None
    for h in range(2):
        plan = gpu.Bn254G2MsmPlan(n // 2)
        plan.gen_points(h * (n // 2))
        plan.upload_scalars(scs[32 * h * (n // 2):32 * (h + 1) * (n // 2)])
        part = plan.run_partial()
        plan.destroy()
        assert len(part) == 192
        acc = g2.add(acc, g2.decode_jac(part))
    assert want == _identity_expected(g2.scalars_ints(scs), 0)
    assert g2.encode(acc) == want


def test_scalars_from_ntt(gpu, base256):
    pts, _, _ = base256
    n = 256
    nplan = gpu.NttPlan(n)
    nplan.upload(gpu.gen_fr(66, n))
    nplan.run()
    plan = gpu.Bn254G2MsmPlan(n)
    plan.gen_points(0)
    plan.scalars_from_ntt(nplan)
    got = plan.run()
    plan.destroy()
    ks = g2.scalars_ints(nplan.download())
    nplan.destroy()
    assert got == g2.encode(g2.msm(pts, ks))


def test_rejections(gpu):
    from ethrex_amd.lib import HipCoreError
    G = g2.encode(g2.G2)
    one = (1).to_bytes(32, "big")
    # flipped byte: off the curve
    bad = bytearray(G)
    bad[127] ^= 1
    bad = bytes(bad)
    rc, _ = gpu.bn254_g2_msm(bad, one, 1)
    assert rc == gpu.EM_ERR_POINT
    rc, _ = gpu.bn254_g2_add(bad, G)
    assert rc == gpu.EM_ERR_POINT
    # a coordinate equal to p: not canonical
    for slot in range(4):
        nc = bytearray(G)
        nc[32 * slot:32 * slot + 32] = g2.P.to_bytes(32, "big")
        nc = bytes(nc)
        rc, _ = gpu.bn254_g2_msm(nc, one, 1)
        assert rc == gpu.EM_ERR_INPUT, slot
        rc, _ = gpu.bn254_g2_add(nc, G)
        assert rc == gpu.EM_ERR_INPUT, slot
        rc, _ = gpu.bn254_g2_mul(nc, one)
        assert rc == gpu.EM_ERR_INPUT, slot
    # on the twist but outside the r-subgroup
    off = g2.encode(g2.OFF_SUBGROUP)
    rc, _ = gpu.bn254_g2_msm(off, one, 1)
    assert rc == gpu.EM_ERR_POINT
    assert "G2 point not in subgroup" in gpu.last_error()
    rc, _ = gpu.bn254_g2_mul(off, one)
    assert rc == gpu.EM_ERR_POINT
    plan = gpu.Bn254G2MsmPlan(2)
    with pytest.raises(HipCoreError) as ei:
        plan.upload_points(G + off)
    assert ei.value.rc == gpu.EM_ERR_POINT
    plan.destroy()
    # add checks on-curve only
    rc, got = gpu.bn254_g2_add(off, G)
    assert rc == 0 and got == g2.encode(g2.add(g2.OFF_SUBGROUP, g2.G2))
    rc, got = gpu.bn254_g2_add(off, off)
    assert rc == 0 and got == g2.encode(g2.add(g2.OFF_SUBGROUP,
                                               g2.OFF_SUBGROUP))


def test_upload_download_round_trip(gpu):
    n = 128
    pts = g2.gen_points(7, n)
    pts[9] = None
    raw = g2.encode_many(pts)
    plan = gpu.Bn254G2MsmPlan(n)
    plan.upload_points(raw)
    got = plan.download_points()
    plan.destroy()
    assert got == raw
