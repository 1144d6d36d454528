"""GPU parity of the bucket partition that groups the merged fixed-base
MSM's entries by bucket (three count/scan/scatter passes in place of the
pair sort).  Merged mode is forced with EM_MSM_FB and the unit size set to
256 entries with EM_MSM_FBM_TILE, so that regions split into many units at
these small n.  Every case holds run() and run_async()/sync() to the CPU
oracle, bit-exact, and to the bytes of a plan created with
EM_MSM_FBM_SORT=rocprim (the pair-sort chain).

Shapes: n = 1, 2, 255 and 2^10 + 1 (one entry, less than a block, more than
one block of pass A with a ragged tail) for c = 20, 22, 24 (3, 5 and 7
pass-A bits); then at c = 22 the inputs that pile entries up: one scalar
and one point repeated (one bucket per window), all-zero scalars (every
entry parked as a skip at key 0), scalars below 2^c (eleven of twelve
windows skip), every full window exactly 2^(c-1) (the maximum key: only the
top pass-A bin), and random scalars with the default unit size.
"""
import pytest

pytestmark = pytest.mark.gpu

CS = (20, 22, 24)
SIZES = (1, 2, 255, (1 << 10) + 1)
NMAX = 1 << 13


def _nwin(c):
    return (254 + c - 1) // c


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
    return oracle_mod.gen_points(0, NMAX), oracle_mod.gen_fr(42, NMAX)


def _sc(k):
    return k.to_bytes(32, "big")


def _run_plan(gpu, c, pts, scs, n):
    plan = gpu.MsmPlan(n)
    try:
        assert plan.fixed_base == c
        plan.upload_points(pts)
        plan.upload_scalars(scs)
        sync = plan.run()
        plan.run_async()
        plan.run_async()
        return sync, plan.sync()
    finally:
        plan.destroy()


def _check(gpu, monkeypatch, oracle_mod, c, pts, scs, n, tile="256"):
    rc, want = oracle_mod.g1_msm(pts, scs, n)
    assert rc == 0
    monkeypatch.setenv("EM_MSM_FB", str(c))
    monkeypatch.delenv("EM_MSM_FBM_SORT", raising=False)
    if tile is None:
        monkeypatch.delenv("EM_MSM_FBM_TILE", raising=False)
    else:
        monkeypatch.setenv("EM_MSM_FBM_TILE", tile)
    got_sync, got_async = _run_plan(gpu, c, pts, scs, n)
    assert got_sync == want, "run()"
    assert got_async == want, "run_async()/sync()"
    monkeypatch.setenv("EM_MSM_FBM_SORT", "rocprim")
    ref_sync, ref_async = _run_plan(gpu, c, pts, scs, n)
    assert got_sync == ref_sync, "run() vs pair-sort plan"
    assert got_async == ref_async, "run_async()/sync() vs pair-sort plan"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("c", CS)
def test_partition_random(gpu, monkeypatch, oracle_mod, base, c, n):
    pts, scs = base
    _check(gpu, monkeypatch, oracle_mod, c, pts[:64 * n], scs[:32 * n], n)


def test_partition_one_scalar_one_point(gpu, monkeypatch, oracle_mod, base):
    """n = 2^13 copies of one point and one scalar: each window's entries
    share one bucket, so a region holds many units that all reserve from
    the same bin."""
    pts, scs = base
    n = 1 << 13
    _check(gpu, monkeypatch, oracle_mod, 22, pts[64 * 5:64 * 6] * n,
           scs[32 * 9:32 * 10] * n, n)


def test_partition_all_zero(gpu, monkeypatch, oracle_mod, base):
    """All-zero scalars: every entry is a skip parked at key 0."""
    pts, _ = base
    n = 1 << 12
    _check(gpu, monkeypatch, oracle_mod, 22, pts[:64 * n], bytes(32 * n), n)


def test_partition_small_scalars(gpu, monkeypatch, oracle_mod, base):
    """Scalars below 2^c: eleven of the twelve windows are skips at key 0
    next to one window of live entries."""
    pts, scs = base
    n, c = 1 << 12, 22
    small = b"".join(
        _sc(int.from_bytes(scs[32 * i:32 * i + 32], "big") % (1 << c))
        for i in range(n))
    _check(gpu, monkeypatch, oracle_mod, c, pts[:64 * n], small, n)


def test_partition_top_bin_only(gpu, monkeypatch, oracle_mod, base):
    """Every full window exactly 2^(c-1): all live entries carry the
    maximum key and land in the top pass-A bin (the short top window is
    zero and skips)."""
    pts, _ = base
    n, c = 1 << 12, 22
    k = sum((1 << (c - 1)) << (c * w) for w in range(_nwin(c) - 1))
    _check(gpu, monkeypatch, oracle_mod, c, pts[:64 * n], _sc(k) * n, n)


def test_partition_default_tile(gpu, monkeypatch, oracle_mod, base):
    pts, scs = base
    n = 1 << 12
    _check(gpu, monkeypatch, oracle_mod, 22, pts[:64 * n], scs[:32 * n], n,
           tile=None)
