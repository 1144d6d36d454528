"""CPU-side checks of the C-ABI library: it loads, exports every symbol
include/ethrex_mi355.h declares, and fails LOUDLY (EM_ERR_HIP) on compute
calls when no GPU is present — no CPU fallback (tier rule ③).

Also parity-checks the host-side deterministic input generator against the
oracle's independent restatement (both implement BASELINE.md's scheme).
"""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "ethrex_mi355.h")
SO = os.path.join(REPO, "ethrex_amd", "libethrex_mi355.so")


def _header_symbols():
    syms = []
    with open(HEADER) as f:
        text = f.read()
    for m in re.finditer(r"\b(ethrex_mi355_\w+)\s*\(", text):
        syms.append(m.group(1))
    return sorted(set(syms))


def test_library_exists_and_loads():
    assert os.path.exists(SO), "run __graft_entry__.build() first"
    ctypes.CDLL(SO)


def test_all_header_symbols_exported():
    lib = ctypes.CDLL(SO)
    syms = _header_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(lib, s), f"missing export: {s}"


@pytest.mark.parametrize("cls,prefix,aff,jac", [
    ("MsmPlan", "msm", 64, 96),
    ("BlsMsmPlan", "bls_msm", 96, 144),
    ("BlsG2MsmPlan", "bls_g2_msm", 192, 288),
    ("Bn254G2MsmPlan", "bn254_g2_msm", 128, 192),
])
def test_msm_plan_classes_call_declared_exports(cls, prefix, aff, jac):
    """every ethrex_mi355_<prefix>_<op> a plan class can call is in the
    header (and so, by the test above, exported); an op outside the
    class's list is refused before any lookup"""
    import ethrex_amd.lib as lib
    plan = getattr(lib, cls)
    assert (plan._PREFIX, plan._AFF, plan._JAC) == (prefix, aff, jac)
    syms = set(_header_symbols())
    assert len(plan._OPS) >= 11 and len(set(plan._OPS)) == len(plan._OPS)
    for op in plan._OPS:
        name = f"ethrex_mi355_{prefix}_{op}"
        assert name in syms, f"{cls}: {name} not in the header"
        assert plan._fn(op) is not None
    with pytest.raises(AttributeError):
        plan._fn("no_such_op")


def test_version():
    import ethrex_amd
    assert "gfx950" in ethrex_amd.version()


def test_gen_fr_parity_with_oracle(oracle_mod):
    import ethrex_amd
    for seed, n in [(42, 257), (43, 64), (50, 1)]:
        assert ethrex_amd.gen_fr(seed, n) == oracle_mod.gen_fr(seed, n)


def test_compute_fails_loudly_without_gpu():
    import ethrex_amd
    if ethrex_amd.device_count() > 0:
        pytest.skip("GPU present; the no-fallback check is for CPU-only hosts")
    g = (1).to_bytes(32, "big") + (2).to_bytes(32, "big")
    rc, _ = ethrex_amd.g1_add(g, g)
    assert rc == ethrex_amd.EM_ERR_HIP
    rc, _ = ethrex_amd.g1_msm(g, b"\x01" * 32, 1)
    assert rc == ethrex_amd.EM_ERR_HIP
    rc, _ = ethrex_amd.fr_ntt(b"\x00" * 32, 1, False)
    assert rc == ethrex_amd.EM_ERR_HIP
    with pytest.raises(Exception):
        ethrex_amd.MsmPlan(16)


def test_bls_gen_fr_parity_with_oracle(oracle_mod):
    import ethrex_amd
    for seed, n in [(42, 200), (45, 17)]:
        assert ethrex_amd.bls_gen_fr(seed, n) == oracle_mod.bls_gen_fr(seed, n)
