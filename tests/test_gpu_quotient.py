"""GPU parity for the coset NTT and the on-device Groth16 quotient
polynomial (QuotPlan), through the C ABI via ctypes, against the test-side
reference (quotient_reference.py: Python integers + oracle.fr_ntt), and
Mi355Backend(composition="quotient") end to end.

Sizes: 2^12 is the largest stage-by-stage size, 2^13 the smallest four-step
size (N1 != N2), 2^14 the square split, 2^15 the other parity; 2^25 (one
sparse case) is the two-level path.
"""
import ctypes
import hashlib
import os
import random
import subprocess
import sys

import pytest

import quotient_reference as Q
from quotient_reference import R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG2 = 13


@pytest.fixture(scope="module")
def gpu():
    import ethrex_amd
    if ethrex_amd.device_count() < 1:
        pytest.skip("no GPU")
    ethrex_amd.set_device(0)
    return ethrex_amd


def _rand(seed, n):
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(n)]


def _plan_coset(gpu, v, inverse):
    plan = gpu.NttPlan(len(v))
    try:
        plan.upload(Q.to_bytes(v))
        plan.run_coset(inverse)
        return Q.to_ints(plan.download())
    finally:
        plan.destroy()


def _quot(gpu, a, b, c=None, plan=None):
    """h through a QuotPlan; c=None => c = a (.) b on device"""
    q = plan or gpu.QuotPlan(len(a))
    try:
        q.upload(0, Q.to_bytes(a))
        q.upload(1, Q.to_bytes(b))
        if c is None:
            q.mul_ab_into_c()
        else:
            q.upload(2, Q.to_bytes(c))
        q.run()
        return Q.to_ints(q.download())
    finally:
        if plan is None:
            q.destroy()


# ---- 1. coset parity ----

@pytest.mark.parametrize("n", [1, 2, 4, 64, 1 << 12, 1 << 13, 1 << 14,
                               1 << 15])
def test_coset_parity(gpu, n):
    x = _rand(100 + n, n)
    fwd = _plan_coset(gpu, x, False)
    assert fwd == Q.coset_fwd(x)
    assert _plan_coset(gpu, x, True) == Q.coset_inv(x)
    assert _plan_coset(gpu, fwd, True) == x


_CHILD = r"""
import hashlib, random, sys
import ethrex_amd as ea
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
ea.set_device(0)
for n in (1 << 13, 1 << 14):
    rng = random.Random(100 + n)
    x = b"".join(rng.randrange(R).to_bytes(32, "big") for _ in range(n))
    for inverse in (False, True):
        plan = ea.NttPlan(n)
        plan.upload(x)
        plan.run_coset(inverse)
        print(n, int(inverse), hashlib.sha256(plan.download()).hexdigest())
        plan.destroy()
"""


def test_coset_unfused_route_is_byte_equal(gpu):
    """EM_NTT_COSET_UNFUSED=1 (read once per process, so a fresh child):
    the standalone scaling pass on the four-step path gives the bytes the
    fused route gives (both pinned to the reference)."""
    env = dict(os.environ, EM_NTT_COSET_UNFUSED="1")
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run([sys.executable, "-c", _CHILD], env=env, cwd=REPO,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = [ln.split() for ln in out.stdout.strip().splitlines()]
    want = []
    for n in (1 << 13, 1 << 14):
        x = _rand(100 + n, n)
        for inverse in (False, True):
            ref = Q.coset_inv(x) if inverse else Q.coset_fwd(x)
            want.append([str(n), str(int(inverse)),
                         hashlib.sha256(Q.to_bytes(ref)).hexdigest()])
    assert got == want


# ---- 2. plain transforms are untouched ----

def test_plain_and_coset_interleaved(gpu, oracle_mod):
    n = 1 << LOG2
    x = _rand(2, n)
    xb = Q.to_bytes(x)
    rc, plain_fwd = oracle_mod.fr_ntt(xb, n, False)
    assert rc == 0
    plan = gpu.NttPlan(n)
    try:
        plan.upload(xb)
        plan.run(False)
        assert plan.download() == plain_fwd
        plan.run(True)
        assert plan.download() == xb
        plan.run_coset(False)
        cf = plan.download()
        assert Q.to_ints(cf) == Q.coset_fwd(x)
        plan.run_coset(True)
        assert plan.download() == xb
        plan.run(False)                      # plain again, after coset use
        assert plan.download() == plain_fwd
        plan.run_coset(True)
        assert Q.to_ints(plan.download()) == \
            Q.coset_inv(Q.to_ints(plain_fwd))
        plan.upload(xb)
        plan.run(True)
        rc, plain_inv = oracle_mod.fr_ntt(xb, n, True)
        assert rc == 0 and plan.download() == plain_inv
    finally:
        plan.destroy()
    rc, one = gpu.coset_ntt(xb, n, False)
    assert rc == 0 and one == cf
    rc, back = gpu.coset_ntt(cf, n, True)
    assert rc == 0 and back == xb


# ---- 3. quotient parity, unsatisfied ----

@pytest.mark.parametrize("n", [1, 2, 8, 1 << 12, 1 << 13, 1 << 15])
def test_quotient_parity(gpu, n):
    a, b, c = _rand(3 * n, n), _rand(3 * n + 1, n), _rand(3 * n + 2, n)
    assert _quot(gpu, a, b, c) == Q.quotient(a, b, c)


# ---- 4. satisfied system ----

@pytest.mark.parametrize("n", [1 << 13, 1 << 15])
def test_satisfied_system(gpu, n):
    a, b = _rand(40 + n, n), _rand(41 + n, n)
    c = [x * y % R for x, y in zip(a, b)]
    h = _quot(gpu, a, b)
    assert h == Q.quotient(a, b, c)
    assert h[n - 1] == 0
    rng = random.Random(42 + n)
    for _ in range(2):
        assert Q.identity_holds(a, b, c, h, rng.randrange(R))


# ---- 5. edge values ----

def test_edge_values(gpu):
    n = 1 << LOG2
    b, c = _rand(50, n), _rand(51, n)
    q = gpu.QuotPlan(n)
    try:
        zero = [0] * n
        assert _quot(gpu, zero, b, c, plan=q) == Q.quotient(zero, b, c)
        top = [R - 1] * n
        assert _quot(gpu, top, top, top, plan=q) == Q.quotient(top, top, top)
        one = [1] * n
        assert _quot(gpu, one, one, plan=q) == zero
        last = [0] * (n - 1) + [R - 2]
        assert _quot(gpu, last, b, c, plan=q) == Q.quotient(last, b, c)
        assert _quot(gpu, b, c, last, plan=q) == Q.quotient(b, c, last)
    finally:
        q.destroy()


# ---- 6. load_from_ntt ----

def test_load_from_ntt(gpu):
    n = 1 << LOG2
    msgs = [bytes([i]) * (i + 1) for i in range(5)]
    offs = [0]
    for m in msgs:
        offs.append(offs[-1] + len(m))
    kp = gpu.KeccakPlan(offs[-1], len(msgs))
    nplan = gpu.NttPlan(n)
    q1, q2 = gpu.QuotPlan(n), gpu.QuotPlan(n)
    try:
        kp.upload(b"".join(msgs), offs)
        kp.run()
        nplan.fill_from_digests(kp, bytes(range(32)))   # input buffer
        a_bytes = nplan.download()
        q1.load_from_ntt(0, nplan)
        nplan.run(False)                                # work buffer
        b_bytes = nplan.download()
        q1.load_from_ntt(1, nplan)
        assert a_bytes != b_bytes
        q1.mul_ab_into_c()
        q1.run()
        q2.upload(0, a_bytes)
        q2.upload(1, b_bytes)
        q2.mul_ab_into_c()
        q2.run()
        h = q1.download()
        assert h == q2.download()
        a, b = Q.to_ints(a_bytes), Q.to_ints(b_bytes)
        assert Q.to_ints(h) == Q.quotient(
            a, b, [x * y % R for x, y in zip(a, b)])
    finally:
        q1.destroy()
        q2.destroy()
        nplan.destroy()
        kp.destroy()


# ---- 7. handoff into the MSM ----

def test_handoff_to_msm(gpu, oracle_mod):
    n = 1 << LOG2
    a, b, c = _rand(70, n), _rand(71, n), _rand(72, n)
    q = gpu.QuotPlan(n)
    mplan = gpu.MsmPlan(n)
    try:
        q.upload(0, Q.to_bytes(a))
        q.upload(1, Q.to_bytes(b))
        q.upload(2, Q.to_bytes(c))
        q.run()
        ptr, cnt = q.device_data()
        assert ptr.value and cnt == n
        mplan.gen_points(0)
        mplan.scalars_from_ntt(q, 0)
        got = mplan.run()
    finally:
        mplan.destroy()
        q.destroy()
    h_ref = Q.to_bytes(Q.quotient(a, b, c))
    rc, want = oracle_mod.g1_msm(oracle_mod.gen_points(0, n), h_ref, n)
    assert rc == 0 and got == want


# ---- 8. plan reuse and state ----

def test_plan_reuse_and_state(gpu):
    from ethrex_amd import lib
    n = 1 << LOG2
    q = gpu.QuotPlan(n)
    try:
        for seed in (80, 90):
            a, b, c = _rand(seed, n), _rand(seed + 1, n), _rand(seed + 2, n)
            assert _quot(gpu, a, b, c, plan=q) == Q.quotient(a, b, c)
            t = q.last_times()
            assert t["total_ms"] > 0 and all(v >= 0 for v in t.values())
        with pytest.raises(lib.HipCoreError) as ei:
            q.run()                       # slots were consumed
        assert ei.value.rc == lib.EM_ERR_INPUT
        q.upload(0, Q.to_bytes(a))
        q.upload(2, Q.to_bytes(c))
        with pytest.raises(lib.HipCoreError) as ei:
            q.run()                       # b missing
        assert ei.value.rc == lib.EM_ERR_INPUT
        q.upload(1, Q.to_bytes(b))
        q.run()
        assert Q.to_ints(q.download()) == Q.quotient(a, b, c)
    finally:
        q.destroy()


# ---- 9. prover ----

@pytest.fixture(scope="module")
def synth():
    from test_gpu_wrap_binding import _synthetic_input
    from ethrex_amd.prover import ExecBackend
    input_data, state = _synthetic_input()
    st = ExecBackend().execute(input_data)
    return input_data, state, st


def _want_proof(oracle_mod, a, b):
    n = len(a)
    h = Q.to_bytes(Q.quotient(a, b, [x * y % R for x, y in zip(a, b)]))
    rc, msm = oracle_mod.g1_msm(oracle_mod.gen_points(0, n), h, n)
    assert rc == 0
    return msm, hashlib.sha256(h).digest()


def test_prove_quotient_witness_binding(gpu, synth, oracle_mod):
    from ethrex_amd import witness
    from ethrex_amd.keccak import keccak256
    from ethrex_amd.prover import Mi355Backend
    from wrap_reference import ref_vector
    input_data, state, st = synth
    n = 1 << LOG2
    com = bytes.fromhex(st["commitment"])
    dom_b = keccak256(com + b"ethrex_amd/quotient/b/v1")
    assert witness.quotient_domain_b(com) == dom_b
    digests = [keccak256(s) for s in state]
    a = Q.to_ints(ref_vector(digests, com, n))
    b = Q.to_ints(ref_vector(digests, dom_b, n))
    backend = Mi355Backend(msm_log2=LOG2, binding="witness",
                           composition="quotient")
    proof = backend.prove(input_data, None)
    want_msm, want_digest = _want_proof(oracle_mod, a, b)
    assert proof["statement"] == st
    assert proof["msm"] == want_msm
    assert proof["ntt_digest"] == want_digest
    pb = bytes(backend.to_proof_bytes(proof, None)["Proof"]["proof"])
    assert len(pb) == 128 and pb[96:] == com
    # the skipped extra node changes the bound proof
    from test_gpu_wrap_binding import _synthetic_input
    in2, _ = _synthetic_input(extra=b"\x02")
    proof2 = backend.prove(in2, None)
    assert proof2["statement"] == st
    assert proof2["msm"] != proof["msm"]
    assert proof2["ntt_digest"] != proof["ntt_digest"]


def test_prove_quotient_seed_binding(gpu, synth, oracle_mod):
    from ethrex_amd.prover import Mi355Backend
    input_data, _, st = synth
    n = 1 << LOG2
    seed = int.from_bytes(bytes.fromhex(st["commitment"])[:8], "little")
    a = Q.to_ints(oracle_mod.gen_fr(seed, n))
    b = Q.to_ints(oracle_mod.gen_fr((seed + 1) % (1 << 64), n))
    proof = Mi355Backend(msm_log2=LOG2, composition="quotient").prove(
        input_data, None)
    want_msm, want_digest = _want_proof(oracle_mod, a, b)
    assert proof["statement"] == st
    assert proof["msm"] == want_msm and proof["ntt_digest"] == want_digest


def test_default_composition_is_direct(gpu, synth, oracle_mod):
    from ethrex_amd.prover import BackendError, Mi355Backend
    input_data, _, st = synth
    n = 1 << LOG2
    backend = Mi355Backend(msm_log2=LOG2)
    assert backend.composition == "direct"
    proof = backend.prove(input_data, None)
    seed = int.from_bytes(bytes.fromhex(st["commitment"])[:8], "little")
    rc, fwd = oracle_mod.fr_ntt(oracle_mod.gen_fr(seed, n), n, False)
    assert rc == 0
    rc, want_msm = oracle_mod.g1_msm(oracle_mod.gen_points(0, n), fwd, n)
    assert rc == 0 and proof["msm"] == want_msm
    assert proof["ntt_digest"] == hashlib.sha256(fwd).digest()
    with pytest.raises(BackendError):
        Mi355Backend(composition="h-only")


# ---- 10. errors ----

def test_errors(gpu):
    from ethrex_amd import lib
    L = lib._lib
    BAD = lib.EM_ERR_INPUT
    sz = ctypes.c_size_t
    # plan creation
    p = ctypes.c_void_p()
    assert L.ethrex_mi355_quot_plan_create(sz(8), None) == BAD
    for n in (0, 3, 12, 1 << 29):
        assert L.ethrex_mi355_quot_plan_create(sz(n), ctypes.byref(p)) == BAD
    assert L.ethrex_mi355_quot_plan_destroy(None) == BAD
    # coset entry points
    assert L.ethrex_mi355_ntt_run_coset(None, ctypes.c_int(0)) == BAD
    assert L.ethrex_mi355_bn254_fr_coset_ntt(None, sz(4), ctypes.c_int(0)) \
        == BAD
    four = (ctypes.c_uint8 * 128)()
    for n in (0, 3):
        assert L.ethrex_mi355_bn254_fr_coset_ntt(four, sz(n),
                                                 ctypes.c_int(0)) == BAD
    noncanon = (ctypes.c_uint8 * 128)(*(bytes(96) + R.to_bytes(32, "big")))
    assert L.ethrex_mi355_bn254_fr_coset_ntt(noncanon, sz(4),
                                             ctypes.c_int(0)) == BAD
    n = 4
    q = gpu.QuotPlan(n)
    nplan = gpu.NttPlan(n)
    try:
        good = Q.to_bytes([1, 2, 3, R - 1])
        gbuf = (ctypes.c_uint8 * len(good))(*good)
        out = (ctypes.c_uint8 * (32 * n))()
        ptr, cnt = ctypes.c_void_p(), sz(0)
        t5 = (ctypes.c_double * 5)()
        # null pointers
        assert L.ethrex_mi355_quot_upload(None, 0, gbuf) == BAD
        assert L.ethrex_mi355_quot_upload(q._p, 0, None) == BAD
        assert L.ethrex_mi355_quot_load_device(None, 0, ptr) == BAD
        assert L.ethrex_mi355_quot_load_device(q._p, 0, None) == BAD
        assert L.ethrex_mi355_quot_mul_ab_into_c(None) == BAD
        assert L.ethrex_mi355_quot_run(None) == BAD
        assert L.ethrex_mi355_quot_download(None, out) == BAD
        assert L.ethrex_mi355_quot_device_data(None, ctypes.byref(ptr),
                                               ctypes.byref(cnt)) == BAD
        assert L.ethrex_mi355_quot_last_times(None, t5) == BAD
        assert L.ethrex_mi355_quot_last_times(q._p, None) == BAD
        # which outside 0..2
        dptr, _ = nplan.device_data()
        for which in (-1, 3):
            assert L.ethrex_mi355_quot_upload(q._p, which, gbuf) == BAD
            assert L.ethrex_mi355_quot_load_device(q._p, which, dptr) == BAD
        # before any run
        assert L.ethrex_mi355_quot_download(q._p, out) == BAD
        assert L.ethrex_mi355_quot_device_data(
            q._p, ctypes.byref(ptr), ctypes.byref(cnt)) == BAD
        assert L.ethrex_mi355_quot_run(q._p) == BAD
        # non-canonical element on upload does not load the slot
        assert L.ethrex_mi355_quot_upload(q._p, 0, noncanon) == BAD
        q.upload(1, good)
        q.upload(2, good)
        assert L.ethrex_mi355_quot_run(q._p) == BAD
        assert L.ethrex_mi355_quot_mul_ab_into_c(q._p) == BAD  # a missing
        q.upload(0, good)
        q.run()
        # null outputs after a run
        assert L.ethrex_mi355_quot_download(q._p, None) == BAD
        assert L.ethrex_mi355_quot_device_data(q._p, None,
                                               ctypes.byref(cnt)) == BAD
        v = Q.to_ints(good)
        assert Q.to_ints(q.download()) == Q.quotient(v, v, v)
        # wrapper-level refusals
        with pytest.raises(lib.HipCoreError):
            q.upload(0, good[:-1])
        with pytest.raises(lib.HipCoreError):
            q.load_from_ntt(0, gpu.NttPlan(8))
    finally:
        nplan.destroy()
        q.destroy()


# ---- 11. two-level path, one large sparse case ----

def test_coset_2_25_sparse_dft_spot_check(gpu):
    n = 1 << 25
    w = Q.root(n)
    nz = {0: 5, 3: 7, 1 << 10: 12345, (1 << 24) + 17: R - 2,
          (1 << 25) - 1: 0xDEADBEEF, 8_675_309: 2, 4097: R - 1,
          (1 << 13) - 1: 1 << 200, 1 << 13: 3, (1 << 12) + 3: 11,
          31_337: 13, (1 << 20) + 5: 17, 1 << 24: 19, 12_345_678: 23,
          (1 << 25) - 4096: 29, 2: 31}
    assert len(nz) == 16
    elems = bytearray(32 * n)
    for i, v in nz.items():
        elems[32 * i:32 * (i + 1)] = v.to_bytes(32, "big")
    rng = random.Random(25)
    idxs = [0, 1, n - 1, n // 2] + [rng.randrange(n) for _ in range(12)]
    zeros = []
    while len(zeros) < 16:
        i = rng.randrange(n)
        if i not in nz:
            zeros.append(i)
    plan = gpu.NttPlan(n)
    try:
        plan.upload(bytes(elems))
        del elems
        plan.run_coset(False)
        fwd = plan.download()
        for j in idxs:
            want = sum(v * pow(Q.G, i, R) * pow(w, (i * j) % n, R)
                       for i, v in nz.items()) % R
            assert int.from_bytes(fwd[32 * j:32 * (j + 1)], "big") == want, \
                f"A[{j}] mismatch"
        del fwd
        plan.run_coset(True)
        back = plan.download()
    finally:
        plan.destroy()
    for i, v in nz.items():
        assert int.from_bytes(back[32 * i:32 * (i + 1)], "big") == v
    for i in zeros:
        assert back[32 * i:32 * (i + 1)] == bytes(32)
