"""GPU parity for the witness binding: k_keccak_pair / k_wrap_expand
(NttPlan.fill_from_digests) against the test-side restatement of wrap
vector v1 (wrap_reference.py), and Mi355Backend(binding="witness") end to
end against the oracle.

Digests are produced on device by the batched keccak plan (pinned by
test_gpu_keccak.py, not under test here); the reference digests are
keccak256 of the same messages.
"""
import ctypes
import hashlib
import os
import random

import pytest

from ethrex_amd.keccak import keccak256
from wrap_reference import ref_vector

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(__file__), "golden",
                       "witness_hoodi_1265656.json.gz")
DOMAIN = bytes(range(100, 132))
LOG2 = 13          # smallest fused four-step NTT size
FBN = 1000


@pytest.fixture(scope="module")
def gpu():
    import ethrex_amd
    if ethrex_amd.device_count() < 1:
        pytest.skip("no GPU")
    ethrex_amd.set_device(0)
    return ethrex_amd


def _keccak_plan(gpu, msgs):
    offs = [0]
    for m in msgs:
        offs.append(offs[-1] + len(m))
    kp = gpu.KeccakPlan(max(offs[-1], 1), len(msgs))
    kp.upload(b"".join(msgs), offs)
    kp.run()
    return kp


def _fill_download(gpu, kp, domain, n):
    nplan = gpu.NttPlan(n)
    try:
        nplan.fill_from_digests(kp, domain)
        assert nplan.last_fill_ms() > 0
        return nplan.download()
    finally:
        nplan.destroy()


# ---- the synthetic witness: a branch root over two account leaves, the
# parent header carrying that root, plus one extra node that nothing links
# to and build_node_map skips (EELS "extra unused trie node") ----

def _synthetic_input(extra=b"\x01", leaf_balance=7):
    from ethrex_amd import rlp, trie, witness
    leaf_a = rlp.encode([b"\x20" + b"\xab" * 31, trie.account_leaf(
        1, leaf_balance, witness.EMPTY_TRIE_HASH, bytes(32))])
    leaf_b = rlp.encode([b"\x20" + b"\xcd" * 31, trie.account_leaf(
        2, 9, witness.EMPTY_TRIE_HASH, bytes(32))])
    branch = rlp.encode([keccak256(leaf_a), keccak256(leaf_b)]
                        + [b""] * 14 + [b""])
    fields = [bytes(32)] * 3 + [keccak256(branch)] + [b""] * 4 \
        + [(FBN - 1).to_bytes(2, "big")]
    header = rlp.encode(fields)
    state = [branch, leaf_a, leaf_b, extra]
    return {
        "batch": 3,
        "witness": {"state": ["0x" + s.hex() for s in state],
                    "headers": ["0x" + header.hex()]},
        "first_block_number": FBN,
    }, state


@pytest.fixture(scope="module")
def synth():
    """the synthetic witness, its CPU statement, and the 2^13 reference
    vector (computed once: ~2k pure-Python permutations)"""
    from ethrex_amd.prover import ExecBackend
    input_data, state = _synthetic_input()
    st = ExecBackend().execute(input_data)
    assert st["n_witness_nodes"] == 4 and st["n_skipped"] == 1
    assert st["n_state_nodes_linked"] == 3 and st["n_accounts"] == 2
    n = 1 << LOG2
    vec = ref_vector([keccak256(s) for s in state],
                     bytes.fromhex(st["commitment"]), n)
    return input_data, state, st, vec


# ---- 1. expansion parity, no transform ----

@pytest.mark.parametrize("m,n", [(1, 1), (2, 2), (3, 4), (1, 64), (5, 64),
                                 (8, 64), (257, 64), (3, 1024)])
def test_fill_matches_reference(gpu, m, n):
    rng = random.Random(1000 * m + n)
    msgs = [bytes(rng.randrange(256) for _ in range(rng.randrange(1, 200)))
            for _ in range(m)]
    kp = _keccak_plan(gpu, msgs)
    try:
        ptr, cnt = kp.device_digests()
        assert ptr.value and cnt == m
        got = _fill_download(gpu, kp, DOMAIN, n)
    finally:
        kp.destroy()
    want = ref_vector([keccak256(x) for x in msgs], DOMAIN, n)
    assert got == want


# ---- 2. realistic m: the Hoodi fixture's 1705 nodes ----

def test_fill_hoodi_digests(gpu):
    from ethrex_amd import witness as W
    state, _, _ = W.load_witness_fixture(FIXTURE)
    assert len(state) == 1705
    kp = _keccak_plan(gpu, state)
    try:
        digests = kp.download()
        got = _fill_download(gpu, kp, DOMAIN, 1024)
    finally:
        kp.destroy()
    hs = [digests[32 * i:32 * i + 32] for i in range(len(state))]
    assert got == ref_vector(hs, DOMAIN, 1024)


# ---- 3. buffer state: a fill after a transform lands in the input buffer ----

def test_fill_resets_buffer_after_run(gpu, synth, oracle_mod):
    _, state, st, vec = synth
    n = 1 << LOG2
    kp = _keccak_plan(gpu, state)
    nplan = gpu.NttPlan(n)
    try:
        nplan.upload(gpu.gen_fr(1, n))
        nplan.run(False)          # data now sits in the work buffer
        nplan.fill_from_digests(kp, bytes.fromhex(st["commitment"]))
        assert nplan.download() == vec
        nplan.run(False)
        rc, want = oracle_mod.fr_ntt(vec, n, False)
        assert rc == 0
        assert nplan.download() == want
    finally:
        nplan.destroy()
        kp.destroy()


# ---- 4. end to end ----

def test_prove_witness_binding_matches_oracle(gpu, synth, oracle_mod):
    from ethrex_amd.prover import Mi355Backend
    input_data, _, st, vec = synth
    n = 1 << LOG2
    backend = Mi355Backend(msm_log2=LOG2, binding="witness")
    proof = backend.prove(input_data, None)
    assert proof["statement"] == st
    rc, fwd = oracle_mod.fr_ntt(vec, n, False)
    assert rc == 0
    rc, want_msm = oracle_mod.g1_msm(oracle_mod.gen_points(0, n), fwd, n)
    assert rc == 0
    assert proof["msm"] == want_msm
    assert proof["ntt_digest"] == hashlib.sha256(fwd).digest()
    pb = bytes(backend.to_proof_bytes(proof, None)["Proof"]["proof"])
    assert len(pb) == 128 and pb[96:] == bytes.fromhex(st["commitment"])


# ---- 5. the binding itself ----

def _proof_bytes(backend, input_data):
    proof = backend.prove(input_data, None)
    pb = bytes(backend.to_proof_bytes(proof, None)["Proof"]["proof"])
    return proof["statement"], pb


def test_skipped_node_bytes_change_the_proof_only_when_bound(gpu):
    from ethrex_amd.prover import Mi355Backend
    in1, _ = _synthetic_input(extra=b"\x01")
    in2, _ = _synthetic_input(extra=b"\x02")
    seed = Mi355Backend(msm_log2=LOG2)
    st1, seed1 = _proof_bytes(seed, in1)
    st2, seed2 = _proof_bytes(seed, in2)
    # the statement (commitment included) does not see the skipped node
    assert st1 == st2 and st1["n_skipped"] == 1
    # ... so the seed binding gives byte-identical proofs (the gap)
    assert seed1 == seed2
    bound = Mi355Backend(msm_log2=LOG2, binding="witness")
    st1w, wit1 = _proof_bytes(bound, in1)
    st2w, wit2 = _proof_bytes(bound, in2)
    assert st1w == st1 and st2w == st1
    assert wit1 != wit2
    assert wit1[:64] != wit2[:64] and wit1[64:96] != wit2[64:96]
    assert wit1[96:] == wit2[96:]
    # a linked leaf's byte changes the proof too
    in3, _ = _synthetic_input(extra=b"\x01", leaf_balance=8)
    _, wit3 = _proof_bytes(bound, in3)
    assert wit3 != wit1 and wit3[:64] != wit1[:64]


def test_witness_less_input_keeps_seed_path(gpu):
    from ethrex_amd.prover import Mi355Backend
    input_data = {"batch": 0, "blocks": [1, 2, 3]}
    a = Mi355Backend(msm_log2=LOG2).prove(input_data, None)
    b = Mi355Backend(msm_log2=LOG2, binding="witness").prove(input_data, None)
    assert a == b and "statement" not in a


# ---- 6. errors ----

def test_errors(gpu):
    from ethrex_amd import lib
    from ethrex_amd.prover import BackendError, Mi355Backend
    kp = gpu.KeccakPlan(64, 2)
    nplan = gpu.NttPlan(4)
    try:
        with pytest.raises(lib.HipCoreError) as ei:
            kp.device_digests()
        assert ei.value.rc == lib.EM_ERR_INPUT
        kp.upload(b"ab", [0, 1, 2])
        with pytest.raises(lib.HipCoreError) as ei:
            kp.device_digests()       # uploaded but not run
        assert ei.value.rc == lib.EM_ERR_INPUT
        with pytest.raises(lib.HipCoreError) as ei:
            nplan.fill_from_digests(kp, DOMAIN)
        assert ei.value.rc == lib.EM_ERR_INPUT
        kp.run()
        ptr, cnt = kp.device_digests()
        assert cnt == 2
        dom = (ctypes.c_uint8 * 32)(*DOMAIN)
        fill = lib._lib.ethrex_mi355_ntt_fill_from_digests
        assert fill(nplan._p, ptr, ctypes.c_size_t(0), dom) == lib.EM_ERR_INPUT
        assert fill(nplan._p, None, ctypes.c_size_t(2), dom) == \
            lib.EM_ERR_INPUT
        assert fill(nplan._p, ptr, ctypes.c_size_t(2), None) == \
            lib.EM_ERR_INPUT
        with pytest.raises(lib.HipCoreError):
            nplan.fill_from_digests(kp, DOMAIN[:31])
    finally:
        nplan.destroy()
        kp.destroy()
    with pytest.raises(BackendError):
        Mi355Backend(binding="node-bytes")


# ---- 7. default unchanged ----

def test_default_binding_is_seed(gpu, synth, oracle_mod):
    from ethrex_amd.prover import Mi355Backend
    input_data, _, st, _ = synth
    n = 1 << LOG2
    proof = Mi355Backend(msm_log2=LOG2).prove(input_data, None)
    assert proof["statement"] == st
    seed = int.from_bytes(bytes.fromhex(st["commitment"])[:8], "little")
    rc, fwd = oracle_mod.fr_ntt(oracle_mod.gen_fr(seed, n), n, False)
    assert rc == 0
    rc, want_msm = oracle_mod.g1_msm(oracle_mod.gen_points(0, n), fwd, n)
    assert rc == 0 and proof["msm"] == want_msm
    assert proof["ntt_digest"] == hashlib.sha256(fwd).digest()
