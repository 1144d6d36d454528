"""GPU parity of the on-device R1CS evaluation (R1csPlan: A z, B z, C z over
packed sparse matrices), through the Python layer and the raw C ABI, against
r1cs_reference.spmv (Python integers), then through QuotPlan and
Mi355Backend(composition="r1cs") end to end.  Every comparison is for
equality over the whole vector.

T = 32 and CHUNK = 1024 mirror the library's short/long row threshold and
long-row chunk (R1CS_T_DEFAULT / R1CS_CHUNK_DEFAULT in api_ntt.hip); the
row-length list brackets both.
"""
import ctypes
import hashlib
import os
import random
import subprocess
import sys

import pytest

import quotient_reference as Q
import r1cs_reference as S
from r1cs_reference import R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 32
CHUNK = 1024
LENGTHS = [1, 7, 8, 9, 15, 16, 17, T - 1, T, T + 1, 63, 64, 65, 127, 128, 129,
           255, 256, 257, 1000, CHUNK - 1, CHUNK, CHUNK + 1, 4097]


@pytest.fixture(scope="module")
def gpu():
    import ethrex_amd
    if ethrex_amd.device_count() < 1:
        pytest.skip("no GPU")
    ethrex_amd.set_device(0)
    return ethrex_amd


def _coeff(rng):
    u = rng.randrange(8)
    if u < 3:
        return 1
    if u < 5:
        return R - 1
    if u == 5:
        return rng.randrange(0, 17)      # zero included
    return rng.randrange(R)


def _rows(rng, lengths, m, coeff=None):
    return [[(rng.randrange(m), coeff if coeff is not None else _coeff(rng))
             for _ in range(ln)] for ln in lengths]


def _eval(gpu, n, z, mat, which=0, plan=None):
    """M z through an R1csPlan -> list of n ints"""
    p = plan or gpu.R1csPlan(n, len(z))
    try:
        p.upload_matrix(which, mat[0], mat[1], S.to_bytes(mat[2]))
        p.upload_witness(S.to_bytes(z))
        p.eval(which)
        return S.to_ints(p.download(which))
    finally:
        if plan is None:
            p.destroy()


def _check(gpu, n, z, rows, which=0):
    mat = S.csr_from_rows(rows)
    assert _eval(gpu, n, z, mat, which) == S.spmv(*mat, z, n)


# ---- 1. tiny ----

def test_tiny_one_entry(gpu):
    for co, zv in ((1, 5), (R - 1, 5), (3, R - 1), (0, 7), (R - 2, R - 1)):
        _check(gpu, 1, [zv], [[(0, co)]])


def test_tiny_ramp_with_duplicates_and_zeros(gpu):
    rng = random.Random(11)
    m = 9
    z = [1] + [rng.randrange(R) for _ in range(m - 1)]
    rows = _rows(rng, range(64), m)
    rows[5] = [(3, 2), (3, R - 2), (3, 1), (4, 0), (3, R - 1)]   # sums to 0
    rows[6] = [(2, 0)] * 6
    rows[7] = [(8, R - 1)] * 7
    for which in range(3):
        _check(gpu, 64, z, rows, which)


# ---- 2. length boundaries, four coefficient sets ----

@pytest.mark.parametrize("mode", ["plus", "minus", "max", "random"])
def test_length_boundaries(gpu, mode):
    rng = random.Random(20)
    m = 5000
    coeff = {"plus": 1, "minus": R - 1, "max": R - 2, "random": None}[mode]
    if mode == "max":
        z = [R - 1] * m     # maximal operands through every accumulation
    else:
        z = [rng.randrange(R) for _ in range(m)]
    _check(gpu, 32, z, _rows(rng, LENGTHS, m, coeff))


# ---- 3. slice tails, short matrices ----

@pytest.mark.parametrize("n_rows", [63, 65, 64 * 5 + 1, 0])
def test_slice_tails(gpu, n_rows):
    n = 512
    rng = random.Random(30 + n_rows)
    m = 40
    z = [rng.randrange(R) for _ in range(m)]
    rows = _rows(rng, [rng.randrange(0, 6) for _ in range(n_rows)], m)
    mat = S.csr_from_rows(rows)
    got = _eval(gpu, n, z, mat)
    assert got == S.spmv(*mat, z, n)
    assert got[n_rows:] == [0] * (n - n_rows)


# ---- 4. one dense row next to many short ones; forced geometries ----

DENSE_M = 1 << 16
DENSE_SHORT = 1 << 13
DENSE_N = 1 << 14


def _dense_case():
    rng = random.Random(40)
    z = [rng.randrange(R) for _ in range(DENSE_M)]
    dense = [(c, _coeff(rng)) for c in range(DENSE_M)]
    rows = _rows(rng, [3] * (DENSE_SHORT // 2), DENSE_M) + [dense] + \
        _rows(rng, [3] * (DENSE_SHORT // 2), DENSE_M)
    return z, S.csr_from_rows(rows)


@pytest.fixture(scope="module")
def dense():
    z, mat = _dense_case()
    return z, mat, S.spmv(*mat, z, DENSE_N)


def test_dense_row_among_short_rows(gpu, dense):
    z, mat, want = dense
    assert _eval(gpu, DENSE_N, z, mat) == want


_CHILD = r"""
import hashlib, sys
sys.path.insert(0, sys.argv[1])
import ethrex_amd as ea
import r1cs_reference as S
from test_gpu_r1cs import _dense_case, DENSE_N
ea.set_device(0)
z, mat = _dense_case()
p = ea.R1csPlan(DENSE_N, len(z))
p.upload_matrix(1, mat[0], mat[1], S.to_bytes(mat[2]))
p.upload_witness(S.to_bytes(z))
p.eval(1)
print(hashlib.sha256(p.download(1)).hexdigest())
p.destroy()
"""


@pytest.mark.parametrize("env", [
    {"EM_R1CS_T": "0", "EM_R1CS_CHUNK": "64"},        # every row long
    {"EM_R1CS_T": "4294967295"},                      # every row short
    {"EM_R1CS_T": "8", "EM_R1CS_CHUNK": "4096"},
])
def test_forced_geometries_give_the_same_bytes(gpu, dense, env):
    """EM_R1CS_T / EM_R1CS_CHUNK are read once per process: a fresh child"""
    _, _, want = dense
    e = dict(os.environ, **env)
    e["PYTHONPATH"] = REPO + os.pathsep + e.get("PYTHONPATH", "")
    out = subprocess.run(
        [sys.executable, "-c", _CHILD, os.path.join(REPO, "tests")], env=e,
        cwd=REPO, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == hashlib.sha256(S.to_bytes(want)).hexdigest()


# ---- 5. dictionary extremes ----

def test_dictionary_all_distinct(gpu):
    rng = random.Random(50)
    m = 300
    z = [rng.randrange(R) for _ in range(m)]
    nnz = 1 << 14
    coeffs = rng.sample(range(2, 1 << 40), nnz - 3) + [0, 2 ** 253, R - 2]
    lengths = [16] * 1000 + [nnz - 16000]          # 1000 short + 1 long row
    it = iter(coeffs)
    rows = [[(rng.randrange(m), next(it)) for _ in range(ln)]
            for ln in lengths]
    assert len(set(coeffs)) == nnz
    _check(gpu, 1024, z, rows)


def test_dictionary_only_plus_minus_one(gpu):
    rng = random.Random(51)
    m = 300
    z = [rng.randrange(R) for _ in range(m)]
    rows = [[(rng.randrange(m), rng.choice((1, R - 1))) for _ in range(ln)]
            for ln in [5] * 200 + [700, 3, 0, 65]]
    _check(gpu, 256, z, rows)


# ---- 6. state and errors ----

def test_reupload_and_witness_invalidation(gpu):
    from ethrex_amd import lib
    rng = random.Random(60)
    n, m = 128, 50
    z1 = [rng.randrange(R) for _ in range(m)]
    z2 = [rng.randrange(R) for _ in range(m)]
    mat1 = S.csr_from_rows(_rows(rng, [4] * 100 + [200], m))
    mat2 = S.csr_from_rows(_rows(rng, [70, 0, 2], m))
    p = gpu.R1csPlan(n, m)
    try:
        assert _eval(gpu, n, z1, mat1, 2, plan=p) == S.spmv(*mat1, z1, n)
        t = p.last_times()
        assert t["c_ms"] > 0 and t["a_ms"] == 0 and t["b_ms"] == 0
        # another shape in the same slot: the old tail rows are zero again
        assert _eval(gpu, n, z1, mat2, 2, plan=p) == S.spmv(*mat2, z1, n)
        # a new witness keeps the matrix but not the result
        p.upload_witness(S.to_bytes(z2))
        for call in (lambda: p.download(2), lambda: p.device_data(2)):
            with pytest.raises(lib.HipCoreError) as ei:
                call()
            assert ei.value.rc == lib.EM_ERR_INPUT
        p.eval(2)
        assert S.to_ints(p.download(2)) == S.spmv(*mat2, z2, n)
        ptr, cnt = p.device_data(2)
        assert ptr.value and cnt == n
        # a matrix upload invalidates its own result only
        p.upload_matrix(0, *mat1[:2], S.to_bytes(mat1[2]))
        p.eval(0)
        p.upload_matrix(2, *mat1[:2], S.to_bytes(mat1[2]))
        with pytest.raises(lib.HipCoreError):
            p.download(2)
        assert S.to_ints(p.download(0)) == S.spmv(*mat1, z2, n)
        # wrapper-level refusals
        with pytest.raises(lib.HipCoreError):
            p.upload_witness(S.to_bytes(z2)[:-1])
        with pytest.raises(lib.HipCoreError):
            p.upload_matrix(0, mat1[0], mat1[1], S.to_bytes(mat1[2])[:-32])
        with pytest.raises(lib.HipCoreError):
            p.upload_matrix(0, [], [], b"")
        with pytest.raises(lib.HipCoreError):
            p.witness_from(gpu.NttPlan(32))          # 50 > 32
        with pytest.raises(lib.HipCoreError):
            gpu.QuotPlan(64).load_from_r1cs(0, p, 0)  # size mismatch
    finally:
        p.destroy()


def test_errors_raw_abi(gpu):
    from ethrex_amd import lib
    L = lib._lib
    BAD = lib.EM_ERR_INPUT
    sz = ctypes.c_size_t
    u64, u32, u8 = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint8
    ci = ctypes.c_int
    p = ctypes.c_void_p()
    for n, m in ((0, 4), (3, 4), (1 << 29, 4), (8, 0), (8, 1 << 32)):
        assert L.ethrex_mi355_r1cs_plan_create(sz(n), sz(m),
                                               ctypes.byref(p)) == BAD
    assert L.ethrex_mi355_r1cs_plan_create(sz(8), sz(4), None) == BAD
    assert L.ethrex_mi355_r1cs_plan_destroy(None) == BAD

    n, m = 8, 4
    plan = gpu.R1csPlan(n, m)
    P = plan._p
    try:
        offs = (u64 * 3)(0, 2, 3)
        cols = (u32 * 3)(0, 3, 1)
        coef = (u8 * 96)(*S.to_bytes([1, R - 1, 5]))
        zb = (u8 * 128)(*S.to_bytes([1, 2, 3, R - 1]))
        out = (u8 * (32 * n))()
        ptr, cnt = ctypes.c_void_p(), sz(0)
        t3 = (ctypes.c_double * 3)()
        up = L.ethrex_mi355_r1cs_upload_matrix
        ev = L.ethrex_mi355_r1cs_eval
        # null pointers
        assert up(None, ci(0), offs, cols, coef, sz(2)) == BAD
        assert up(P, ci(0), None, cols, coef, sz(2)) == BAD
        assert up(P, ci(0), offs, None, coef, sz(2)) == BAD
        assert up(P, ci(0), offs, cols, None, sz(2)) == BAD
        assert L.ethrex_mi355_r1cs_upload_witness(None, zb) == BAD
        assert L.ethrex_mi355_r1cs_upload_witness(P, None) == BAD
        assert L.ethrex_mi355_r1cs_witness_from_device(None, ptr, u64(0)) == BAD
        assert L.ethrex_mi355_r1cs_witness_from_device(P, None, u64(0)) == BAD
        assert ev(None, ci(0)) == BAD
        assert L.ethrex_mi355_r1cs_download(None, ci(0), out) == BAD
        assert L.ethrex_mi355_r1cs_device_data(
            None, ci(0), ctypes.byref(ptr), ctypes.byref(cnt)) == BAD
        assert L.ethrex_mi355_r1cs_last_times(None, t3) == BAD
        assert L.ethrex_mi355_r1cs_last_times(P, None) == BAD
        # which outside 0..2
        for which in (-1, 3):
            assert up(P, ci(which), offs, cols, coef, sz(2)) == BAD
            assert ev(P, ci(which)) == BAD
            assert L.ethrex_mi355_r1cs_download(P, ci(which), out) == BAD
            assert L.ethrex_mi355_r1cs_device_data(
                P, ci(which), ctypes.byref(ptr), ctypes.byref(cnt)) == BAD
        # eval needs the matrix and a witness
        assert ev(P, ci(0)) == BAD
        assert up(P, ci(0), offs, cols, coef, sz(2)) == 0
        assert ev(P, ci(0)) == BAD                     # no witness yet
        assert L.ethrex_mi355_r1cs_upload_witness(P, zb) == 0
        assert ev(P, ci(1)) == BAD                     # B not loaded
        assert L.ethrex_mi355_r1cs_download(P, ci(0), out) == BAD  # no eval
        assert L.ethrex_mi355_r1cs_device_data(
            P, ci(0), ctypes.byref(ptr), ctypes.byref(cnt)) == BAD
        assert ev(P, ci(0)) == 0
        assert L.ethrex_mi355_r1cs_download(P, ci(0), None) == BAD
        assert L.ethrex_mi355_r1cs_device_data(P, ci(0), None,
                                               ctypes.byref(cnt)) == BAD
        assert L.ethrex_mi355_r1cs_download(P, ci(0), out) == 0
        assert S.to_ints(bytes(out)) == \
            [(1 - (R - 1)) % R, 10] + [0] * (n - 2)
        # malformed matrices; each leaves the slot unloaded
        bad_cases = [
            ((u64 * 3)(1, 2, 3), cols, coef, 2),         # row_offs[0] = 1
            ((u64 * 3)(0, 3, 2), cols, coef, 2),         # decreasing
            ((u64 * 3)(0, 1, 1 << 32), cols, coef, 2),   # nnz = 2^32
            (offs, (u32 * 3)(0, m, 1), coef, 2),         # col = n_vars
            (offs, cols, (u8 * 96)(*S.to_bytes([1, R - 1]),
                                   *R.to_bytes(32, "big")), 2),  # coeff = r
            (offs, cols, (u8 * 96)(*([255] * 96)), 2),
            ((u64 * 10)(*([0] * 10)), cols, coef, 9),    # n_rows > n
        ]
        for o, c, k, rows in bad_cases:
            assert up(P, ci(0), offs, cols, coef, sz(2)) == 0
            assert ev(P, ci(0)) == 0
            assert up(P, ci(0), o, c, k, sz(rows)) == BAD
            assert ev(P, ci(0)) == BAD
            assert L.ethrex_mi355_r1cs_download(P, ci(0), out) == BAD
        # a non-canonical witness element unloads the witness
        assert up(P, ci(0), offs, cols, coef, sz(2)) == 0
        zbad = (u8 * 128)(*(bytes(96) + R.to_bytes(32, "big")))
        assert L.ethrex_mi355_r1cs_upload_witness(P, zbad) == BAD
        assert ev(P, ci(0)) == BAD
        assert L.ethrex_mi355_r1cs_upload_witness(P, zb) == 0
        assert ev(P, ci(0)) == 0
        # n_rows = 0 is legal: the zero vector
        assert up(P, ci(1), (u64 * 1)(0), cols, coef, sz(0)) == 0
        assert ev(P, ci(1)) == 0
        assert L.ethrex_mi355_r1cs_download(P, ci(1), out) == 0
        assert bytes(out) == bytes(32 * n)
    finally:
        plan.destroy()


# ---- 7. witness from a device vector ----

def test_witness_from_device(gpu):
    rng = random.Random(70)
    n_ntt = 1 << 13
    m, n = 100, 64
    mat = S.csr_from_rows(_rows(rng, [3] * 60 + [90], m))
    msgs = [bytes([i]) * (i + 1) for i in range(5)]
    offs = [0]
    for x in msgs:
        offs.append(offs[-1] + len(x))
    kp = gpu.KeccakPlan(offs[-1], len(msgs))
    nplan = gpu.NttPlan(n_ntt)
    p, p_host = gpu.R1csPlan(n, m), gpu.R1csPlan(n, m)
    try:
        p.upload_matrix(0, mat[0], mat[1], S.to_bytes(mat[2]))
        p_host.upload_matrix(0, mat[0], mat[1], S.to_bytes(mat[2]))
        kp.upload(b"".join(msgs), offs)
        kp.run()

        def both(offset):
            vec = nplan.download()
            zb = vec[32 * offset:32 * (offset + m)]
            p.witness_from(nplan, offset)
            p.eval(0)
            p_host.upload_witness(zb)
            p_host.eval(0)
            got = p.download(0)
            assert got == p_host.download(0)
            assert S.to_ints(got) == S.spmv(*mat, S.to_ints(zb), n)

        nplan.upload(gpu.gen_fr(7, n_ntt))
        nplan.run(False)                 # four-step: data in the work buffer
        both(0)
        both(37)
        both(n_ntt - m)
        nplan.fill_from_digests(kp, bytes(range(32)))   # input buffer
        both(0)
        both(4001)
        with pytest.raises(Exception):
            p.witness_from(nplan, n_ntt - m + 1)
    finally:
        p.destroy()
        p_host.destroy()
        nplan.destroy()
        kp.destroy()


# ---- 8. handoff into the quotient ----

@pytest.mark.parametrize("log2", [12, 13])
def test_handoff_to_quotient(gpu, log2):
    from ethrex_amd import r1cs as C
    n = 1 << log2
    k = 8
    mats, witness = C.chain_circuit(n, k, 3, 5)
    rng = random.Random(80 + log2)
    z = witness([rng.randrange(R) for _ in range(k)])
    a, b, c = (S.spmv(*mt, z, n) for mt in mats)
    assert [x * y % R for x, y in zip(a, b)] == c
    rp = gpu.R1csPlan(n, len(z))
    q = gpu.QuotPlan(n)
    try:
        for which, mt in enumerate(mats):
            rp.upload_matrix(which, mt[0], mt[1], S.to_bytes(mt[2]))
        rp.upload_witness(S.to_bytes(z))
        rp.eval_all()
        assert [S.to_ints(rp.download(w)) for w in range(3)] == [a, b, c]
        for which in range(3):
            q.load_from_r1cs(which, rp, which)
        q.run()
        h = Q.to_ints(q.download())
    finally:
        q.destroy()
        rp.destroy()
    assert h == Q.quotient(a, b, c)
    assert h[n - 1] == 0
    assert Q.identity_holds(a, b, c, h, rng.randrange(R))


# ---- 9. prover ----

LOG2 = 13


def _want_r1cs_proof(oracle_mod, free_bytes):
    from ethrex_amd import r1cs as C
    from ethrex_amd.prover import Mi355Backend as B
    n = 1 << LOG2
    assert (B.R1CS_K, B.R1CS_FAN_IN) == (64, 3)
    mats, witness = C.chain_circuit(n, B.R1CS_K, B.R1CS_FAN_IN, B.R1CS_SEED)
    z = witness(S.to_ints(free_bytes))
    a, b, c = (S.spmv(*mt, z, n) for mt in mats)
    assert [x * y % R for x, y in zip(a, b)] == c
    hv = Q.quotient(a, b, c)
    assert hv[n - 1] == 0
    h = Q.to_bytes(hv)
    rc, msm = oracle_mod.g1_msm(oracle_mod.gen_points(0, n), h, n)
    assert rc == 0
    return msm, hashlib.sha256(h).digest()


def test_prove_r1cs_witness_less_input(gpu, oracle_mod):
    from ethrex_amd.prover import Mi355Backend
    input_data = {"batch": 0, "blocks": [1, 2, 3]}
    n = 1 << LOG2
    backend = Mi355Backend(msm_log2=LOG2, composition="r1cs")
    proof = backend.prove(input_data, None)
    seed = backend._seed(input_data)
    want_msm, want_digest = _want_r1cs_proof(oracle_mod,
                                             oracle_mod.gen_fr(seed, 64))
    assert "statement" not in proof
    assert proof["msm"] == want_msm and proof["ntt_digest"] == want_digest
    # the witness binding has no digests to bind here: same proof
    assert Mi355Backend(msm_log2=LOG2, composition="r1cs",
                        binding="witness").prove(input_data, None) == proof
    # the other compositions still give what the reference gives
    rc, fwd = oracle_mod.fr_ntt(oracle_mod.gen_fr(seed, n), n, False)
    assert rc == 0
    rc, direct_msm = oracle_mod.g1_msm(oracle_mod.gen_points(0, n), fwd, n)
    assert rc == 0
    direct = Mi355Backend(msm_log2=LOG2).prove(input_data, None)
    assert direct == {"msm": direct_msm,
                      "ntt_digest": hashlib.sha256(fwd).digest()}
    qa = Q.to_ints(oracle_mod.gen_fr(seed, n))
    qb = Q.to_ints(oracle_mod.gen_fr((seed + 1) % (1 << 64), n))
    qh = Q.to_bytes(Q.quotient(qa, qb, [x * y % R for x, y in zip(qa, qb)]))
    rc, quot_msm = oracle_mod.g1_msm(oracle_mod.gen_points(0, n), qh, n)
    assert rc == 0
    quot = Mi355Backend(msm_log2=LOG2, composition="quotient").prove(
        input_data, None)
    assert quot == {"msm": quot_msm,
                    "ntt_digest": hashlib.sha256(qh).digest()}
    assert len({proof["msm"], direct["msm"], quot["msm"]}) == 3


def test_prove_r1cs_witness_binding_hoodi(gpu, oracle_mod):
    from ethrex_amd import witness as W
    from ethrex_amd.prover import Mi355Backend
    from wrap_reference import ref_vector
    fx = os.path.join(os.path.dirname(__file__), "golden",
                      "witness_hoodi_1265656.json.gz")
    state, headers, fbn = W.load_witness_fixture(fx)
    input_data = {
        "batch": 7,
        "witness": {"state": ["0x" + s.hex() for s in state],
                    "headers": ["0x" + h.hex() for h in headers]},
        "first_block_number": fbn,
    }
    backend = Mi355Backend(msm_log2=LOG2, binding="witness",
                           composition="r1cs")
    proof = backend.prove(input_data, None)
    st = proof["statement"]
    assert st == backend.execute(input_data)
    com = bytes.fromhex(st["commitment"])
    # the node digests through the batched keccak (pinned to the reference
    # by test_gpu_keccak.py); wrap vector v1's prefix does not depend on n
    offs = [0]
    for s in state:
        offs.append(offs[-1] + len(s))
    rc, dig = gpu.keccak256_batch(b"".join(state), offs, len(state))
    assert rc == 0
    digests = [dig[32 * i:32 * i + 32] for i in range(len(state))]
    free = ref_vector(digests, com, 64)
    want_msm, want_digest = _want_r1cs_proof(oracle_mod, free)
    assert proof["msm"] == want_msm and proof["ntt_digest"] == want_digest
    pb = bytes(backend.to_proof_bytes(proof, None)["Proof"]["proof"])
    assert len(pb) == 128 and pb[96:] == com


def test_prove_r1cs_binding_sees_every_node_byte(gpu):
    from ethrex_amd.prover import Mi355Backend
    from test_gpu_wrap_binding import _synthetic_input
    in1, _ = _synthetic_input(extra=b"\x01")
    in2, _ = _synthetic_input(extra=b"\x02")
    bound = Mi355Backend(msm_log2=LOG2, binding="witness", composition="r1cs")
    p1, p2 = bound.prove(in1, None), bound.prove(in2, None)
    assert p1["statement"] == p2["statement"]
    assert p1["msm"] != p2["msm"] and p1["ntt_digest"] != p2["ntt_digest"]
    seeded = Mi355Backend(msm_log2=LOG2, composition="r1cs")
    assert seeded.prove(in1, None) == seeded.prove(in2, None)
