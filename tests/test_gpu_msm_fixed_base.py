"""GPU parity of the merged fixed-base geometry of the BN254 G1 MSM
(signed digits, one bucket space for all windows over the table
T[w*n + i] = 2^(c*w) * P_i), forced with EM_MSM_FB at the smallest shapes
at which the recode, the table or the walk can go wrong: n = 1, 2, 3,
2^10 + 1 and 2^13, against the CPU oracle, bit-exact.  Also: every entry
point agrees with the forced-off path byte for byte, sampled table rows
equal 2^(c*w) * P_i, and a plan whose table cannot fit falls back.  One
case at n = 2^23 holds the separate-window path with 16-bit sort keys to
the merged path, which is the default there.
"""
import pytest

pytestmark = pytest.mark.gpu

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47

CS = (20, 22, 24)
SIZES = (1, 2, 3, (1 << 10) + 1, 1 << 13)
NMAX = max(SIZES)


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


def _neg(pt):
    y = int.from_bytes(pt[32:64], "big")
    return pt[:32] + ((Q - y) % Q).to_bytes(32, "big")


def _sc(k):
    return k.to_bytes(32, "big")


def _plan(gpu, monkeypatch, c, n):
    monkeypatch.setenv("EM_MSM_FB", str(c))
    plan = gpu.MsmPlan(n)
    assert plan.fixed_base == c
    return plan


def _check(gpu, monkeypatch, oracle_mod, c, pts, scs, n):
    rc, want = oracle_mod.g1_msm(pts, scs, n)
    assert rc == 0
    plan = _plan(gpu, monkeypatch, c, n)
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
def test_fb_random(gpu, monkeypatch, oracle_mod, base, n):
    pts, scs = base
    _check(gpu, monkeypatch, oracle_mod, 20, pts[:64 * n], scs[:32 * n], n)


def _edge_scalars(c):
    nw = _nwin(c)
    half = 1 << (c - 1)
    every_half = sum(half << (c * w) for w in range(nw - 1))
    every_half1 = sum((half + 1) << (c * w) for w in range(nw - 1))
    ones = (1 << (c * (nw - 1))) - 1
    edge = [0, 1, R - 1, half, half + 1, (1 << c) - 1, every_half,
            every_half1, ones, R - 2, 1 << 253]
    assert all(e < R for e in edge)
    return edge


@pytest.mark.parametrize("c", CS)
def test_fb_edge_cases(gpu, monkeypatch, oracle_mod, base, c):
    """In one MSM of n = 2^10 + 1: the boundary scalars (carry into every
    window and into the top one, every window exactly 2^(c-1)), points at
    infinity, the same point twice with equal scalars (doubling inside a
    bucket) and P, -P with equal scalars (cancellation)."""
    pts, scs = base
    n = (1 << 10) + 1
    out_p = bytearray(pts[:64 * n])
    out_s = bytearray(scs[:32 * n])
    edge = _edge_scalars(c)
    for i in range(0, n, 3):
        out_s[32 * i:32 * i + 32] = _sc(edge[(i // 3) % len(edge)])
    # infinity mixed in (with live scalars)
    for i in range(7, n, 97):
        out_p[64 * i:64 * i + 64] = bytes(64)
    # the same point twice, equal scalars: slots 10/11 random scalar,
    # 12/13 and 15/16 boundary scalars
    for a, b, k in ((10, 11, None), (12, 13, edge[3]), (15, 16, edge[6])):
        out_p[64 * b:64 * b + 64] = out_p[64 * a:64 * a + 64]
        s = out_s[32 * a:32 * a + 32] if k is None else _sc(k)
        out_s[32 * a:32 * a + 32] = s
        out_s[32 * b:32 * b + 32] = s
    # P and -P, equal scalars
    for a, b, k in ((20, 21, None), (22, 23, edge[4]), (25, 26, edge[7])):
        out_p[64 * b:64 * b + 64] = _neg(bytes(out_p[64 * a:64 * a + 64]))
        s = out_s[32 * a:32 * a + 32] if k is None else _sc(k)
        out_s[32 * a:32 * a + 32] = s
        out_s[32 * b:32 * b + 32] = s
    _check(gpu, monkeypatch, oracle_mod, c, bytes(out_p), bytes(out_s), n)


def test_fb_all_identical(gpu, monkeypatch, oracle_mod, base):
    """One point, one scalar, n = 2^13 times: every bucket run starts with
    a doubling and is long enough to be cut into several walk slots."""
    pts, scs = base
    n = 1 << 13
    _check(gpu, monkeypatch, oracle_mod, 20, pts[64 * 5:64 * 6] * n,
           scs[32 * 9:32 * 10] * n, n)


def test_fb_entry_points_match_forced_off(gpu, monkeypatch, base):
    """run, run_async + sync, run_partial through g1_combine_cpu and
    scalars_from_ntt give the bytes of the EM_MSM_FB=0 path."""
    pts, scs = base
    n = (1 << 10) + 1
    m = 1 << 11
    nplan = gpu.NttPlan(m)
    nplan.upload(gpu.gen_fr(66, m))
    nplan.run(False)
    res = {}
    try:
        for mode in ("0", "22"):
            monkeypatch.setenv("EM_MSM_FB", mode)
            plan = gpu.MsmPlan(n)
            try:
                assert plan.fixed_base == int(mode)
                plan.upload_points(pts[:64 * n])
                plan.upload_scalars(scs[:32 * n])
                r = [plan.run()]
                plan.run_async()
                plan.run_async()
                r.append(plan.sync())
                r.append(gpu.g1_combine_cpu(plan.run_partial(), 1))
                plan.scalars_from_ntt(nplan, 5)
                r.append(plan.run())
                plan.run_async()
                r.append(plan.sync())
                res[mode] = r
            finally:
                plan.destroy()
    finally:
        nplan.destroy()
    assert res["0"][0] == res["0"][1] == res["0"][2]
    assert res["0"][3] == res["0"][4] != res["0"][0]
    assert res["22"] == res["0"]


def test_keys16_window_path_matches_merged_2_23(gpu, monkeypatch):
    """n = 2^23, the smallest size with 16-bit per-window sort keys: the
    EM_MSM_FB=0 plan (u16 digits, one sort per window, segmented offsets)
    gives, from run, run_async + sync and run_partial, the bytes of the
    default plan, which runs merged c = 22 there (its own recode, sort
    geometry and walk; pinned to the oracle by the small shapes above)."""
    n = 1 << 23
    scs = gpu.gen_fr(42, n)
    monkeypatch.delenv("EM_MSM_FB", raising=False)
    plan = gpu.MsmPlan(n)
    try:
        assert plan.fixed_base == 22
        plan.gen_points(0)
        plan.upload_scalars(scs)
        want = plan.run()
    finally:
        plan.destroy()
    monkeypatch.setenv("EM_MSM_FB", "0")
    plan = gpu.MsmPlan(n)
    try:
        assert plan.fixed_base == 0
        plan.gen_points(0)
        plan.upload_scalars(scs)
        assert plan.run() == want, "run()"
        t = plan.last_times()
        plan.run_async()
        plan.run_async()
        assert plan.sync() == want, "run_async()/sync()"
        assert gpu.g1_combine_cpu(plan.run_partial(), 1) == want, "partial"
    finally:
        plan.destroy()
    print("last_times (EM_MSM_FB=0, n=2^23):", t)
    assert t["digits_sort_ms"] > 0
    assert t["bucket_acc_ms"] > 0
    assert t["reduce_ms"] > 0
    assert t["total_ms"] >= t["bucket_acc_ms"]


@pytest.mark.parametrize("c", CS)
def test_fb_table_rows(gpu, monkeypatch, oracle_mod, c):
    """n = 257: for every window w, sampled rows of the table equal
    2^(c*w) * P_i; a base at infinity stays at infinity in every row."""
    n = 257
    pts = bytearray(oracle_mod.gen_points(3, n))
    pts[64 * 100:64 * 101] = bytes(64)
    pts = bytes(pts)
    plan = _plan(gpu, monkeypatch, c, n)
    try:
        plan.upload_points(pts)
        assert plan.fb_table_bytes == _nwin(c) * n * 72
        assert plan.last_times()["fb_precompute_ms"] > 0.0
        for w in range(_nwin(c)):
            k = _sc((1 << (c * w)) % R)
            for start, count in ((0, 2), (99, 3), (255, 2)):
                rows = plan.download_fb_rows(w, start, count)
                for j in range(count):
                    i = start + j
                    rc, want = oracle_mod.g1_mul(pts[64 * i:64 * i + 64], k)
                    assert rc == 0
                    assert rows[64 * j:64 * j + 64] == want, (w, i)
    finally:
        plan.destroy()


def test_fb_falls_back(gpu, monkeypatch, oracle_mod, base):
    """No room for the table (memory probe overridden), or table indices
    that would not fit below the sign bits: the plan reports fixed_base 0
    and runs the separate-window path."""
    pts, scs = base
    n = 1 << 10
    monkeypatch.setenv("EM_MSM_FB", "22")
    monkeypatch.setenv("EM_MSM_FB_FREE_BYTES", str(1 << 20))
    plan = gpu.MsmPlan(n)
    try:
        assert plan.fixed_base == 0
        plan.upload_points(pts[:64 * n])
        plan.upload_scalars(scs[:32 * n])
        rc, want = oracle_mod.g1_msm(pts[:64 * n], scs[:32 * n], n)
        assert rc == 0 and plan.run() == want
        assert plan.last_times()["fb_precompute_ms"] == 0.0
    finally:
        plan.destroy()
    # 13 windows * n >= 2^30 at c = 20; the memory probe is told there is
    # room, so only the index bound can refuse
    monkeypatch.setenv("EM_MSM_FB", "20")
    monkeypatch.setenv("EM_MSM_FB_FREE_BYTES", str(1 << 50))
    n_big = -(-(1 << 30) // 13)
    plan = gpu.MsmPlan(n_big)
    try:
        assert plan.fixed_base == 0
    finally:
        plan.destroy()
    # default selection leaves small plans on the separate-window path
    monkeypatch.delenv("EM_MSM_FB")
    monkeypatch.delenv("EM_MSM_FB_FREE_BYTES")
    plan = gpu.MsmPlan(n)
    try:
        assert plan.fixed_base == 0
    finally:
        plan.destroy()
