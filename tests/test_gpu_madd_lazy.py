"""GPU parity of the lazy signed mixed add in the BN254 bucket walk, at the
smallest shape on each BN254 path: n = 65537 (signed c=17, first n above the
c=8 cutoff) and n = 4096 (c=8).  MsmPlan.run() and run_async()/sync() vs the
CPU oracle, bit-exact, on inputs that drive the add's exceptional branches:
doubling at the start of every bucket run, P + (-P) cancellation mid-run
with the accumulator reloading afterwards, and the sign-recode boundary
digits of the signed config.
"""
import pytest

pytestmark = pytest.mark.gpu

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47

SIZES = (65537, 4096)


@pytest.fixture(scope="module")
def gpu():
    import ethrex_amd
    if ethrex_amd.device_count() < 1:
        pytest.skip("no GPU")
    ethrex_amd.set_device(0)
    return ethrex_amd


@pytest.fixture(scope="module")
def base(oracle_mod):
    """(points, scalars) for the largest size, computed once and sliced."""
    n = max(SIZES)
    return oracle_mod.gen_points(0, n), oracle_mod.gen_fr(42, n)


def _neg(pt):
    y = int.from_bytes(pt[32:64], "big")
    return pt[:32] + ((Q - y) % Q).to_bytes(32, "big")


def _sc(k):
    return (k % (1 << 256)).to_bytes(32, "big")


def _check(gpu, oracle_mod, pts, scs, n):
    rc, want = oracle_mod.g1_msm(pts, scs, n)
    assert rc == 0
    plan = gpu.MsmPlan(n)
    try:
        plan.upload_points(pts)
        plan.upload_scalars(scs)
        assert plan.run() == want, "run()"
        plan.run_async()
        plan.run_async()
        assert plan.sync() == want, "run_async()/sync()"
    finally:
        plan.destroy()


@pytest.mark.parametrize("n", SIZES)
def test_lazy_random(gpu, oracle_mod, base, n):
    """(a) random points and scalars."""
    pts, scs = base
    _check(gpu, oracle_mod, pts[:64 * n], scs[:32 * n], n)


@pytest.mark.parametrize("n", SIZES)
def test_lazy_all_identical(gpu, oracle_mod, base, n):
    """(b) every point and every scalar identical: each bucket run holds n
    copies of one point, so it starts with a doubling."""
    pts, scs = base
    _check(gpu, oracle_mod, pts[64 * 5:64 * 6] * n, scs[32 * 9:32 * 10] * n, n)


@pytest.mark.parametrize("n", SIZES)
def test_lazy_cancelling_pairs(gpu, oracle_mod, base, n):
    """(c) P, -P pairs with equal scalars share a bucket in every window:
    the accumulator returns to infinity mid-run and continues.  Few distinct
    points and scalars make the runs long; the odd tail point of n = 65537
    keeps the total non-trivial."""
    pts, scs = base
    out_p, out_s = bytearray(), bytearray()
    for i in range(n // 2):
        j = i % 7
        p = pts[64 * j:64 * j + 64]
        s = scs[32 * (i % 3):32 * (i % 3) + 32]
        out_p += p + _neg(p)
        out_s += s + s
    for i in range(n - 2 * (n // 2)):
        out_p += pts[64 * 11:64 * 12]
        out_s += scs[32 * 11:32 * 12]
    # a few unpaired points so the sum is not the identity
    for i in range(0, 64):
        out_p[64 * 2 * i + 64:64 * 2 * i + 128] = pts[64 * 20:64 * 21]
    _check(gpu, oracle_mod, bytes(out_p), bytes(out_s), n)


@pytest.mark.parametrize("n", SIZES)
def test_lazy_edge_scalars(gpu, oracle_mod, base, n):
    """(d) 0, 1, r-1, scalars whose 17-bit windows are all exactly 2^16
    (largest positive digit) or 2^16+1 (first negative digit, carries),
    all-ones windows (carry into every window) — over random and repeated
    points."""
    pts, scs = base
    w = 17
    nwin = 15
    half = sum((1 << 16) << (w * i) for i in range(nwin - 1))
    half1 = sum(((1 << 16) + 1) << (w * i) for i in range(nwin - 1))
    ones = (1 << (w * (nwin - 1))) - 1
    ones8 = (1 << 248) - 1
    edge = [0, 1, R - 1, R, half, half1, ones, ones8,
            (1 << 16), (1 << 16) + 1, (1 << 17) - 1, (1 << 253)]
    assert all(e < (1 << 256) for e in edge)
    out_s = bytearray(scs[:32 * n])
    out_p = bytearray(pts[:64 * n])
    for i in range(0, n, 3):
        out_s[32 * i:32 * i + 32] = _sc(edge[(i // 3) % len(edge)])
    # the same point under both boundary digits, next to each other
    for i in range(0, min(n, 4096), 6):
        out_p[64 * (i + 3):64 * (i + 4)] = out_p[64 * i:64 * (i + 1)]
    _check(gpu, oracle_mod, bytes(out_p), bytes(out_s), n)
