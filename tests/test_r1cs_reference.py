"""CPU checks of the R1CS pieces that need no GPU: product-chain circuit v1
(ethrex_amd/r1cs.py) is satisfied, its vectors give an exact quotient, its
bytes are stable, and the R1CS entry points refuse loudly without a device.
"""
import ctypes
import hashlib
import random

import pytest

import quotient_reference as Q
import r1cs_reference as S
from r1cs_reference import R

from ethrex_amd import r1cs as C

K = 4
FAN_IN = 3


def _abc(n_cons, seed, n=None):
    mats, witness = C.chain_circuit(n_cons, K, FAN_IN, seed)
    rng = random.Random(1000 + seed)
    z = witness([rng.randrange(R) for _ in range(K)])
    assert len(z) == 1 + K + n_cons and z[0] == 1
    return [S.spmv(*m, z, n) for m in mats], mats, z


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("n_cons", [1, 5, 64])
def test_chain_circuit_is_satisfied(n_cons, seed):
    (a, b, c), mats, z = _abc(n_cons, seed)
    assert len(a) == len(b) == len(c) == n_cons
    assert [x * y % R for x, y in zip(a, b)] == c
    assert c == z[1 + K:]
    # shape: fan_in entries per A/B row, reaching only earlier wires
    for offs, cols, coeffs in mats[:2]:
        assert offs == list(range(0, FAN_IN * n_cons + 1, FAN_IN))
        for i in range(n_cons):
            assert all(cl < 1 + K + i for cl in cols[offs[i]:offs[i + 1]])
        assert all(0 <= co < R for co in coeffs)
    assert mats[2] == (list(range(n_cons + 1)),
                       [1 + K + i for i in range(n_cons)], [1] * n_cons)


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("n_cons", [1, 5, 64])
def test_chain_circuit_quotient_is_exact(n_cons, seed):
    n = 1
    while n < n_cons:
        n *= 2
    (a, b, c), _, _ = _abc(n_cons, seed, n)
    assert len(a) == n
    h = Q.quotient(a, b, c)
    assert h[n - 1] == 0
    rng = random.Random(77 + seed)
    for _ in range(2):
        assert Q.identity_holds(a, b, c, h, rng.randrange(R))


def test_chain_circuit_bytes_are_stable():
    (a, b, c), witness = C.chain_circuit(64, 4, 3, 7)
    h = hashlib.sha256()
    for offs, cols, coeffs in (a, b, c):
        h.update(b"".join(x.to_bytes(8, "little") for x in offs))
        h.update(b"".join(x.to_bytes(4, "little") for x in cols))
        h.update(C.fr_bytes(coeffs))
    h.update(C.fr_bytes(witness([11, 22, 33, 44])))
    assert h.hexdigest() == \
        "7fd303cb05fc2a63b847c2587dce787162079f412301db4f2fe4a4511d5fde65"
    # the stated coefficient mix is present
    kinds = {1: 0, R - 1: 0, "small": 0, "wide": 0}
    for co in a[2] + b[2]:
        key = co if co in (1, R - 1) else "small" if co < 17 else "wide"
        kinds[key] += 1
    assert all(v > 0 for v in kinds.values())
    assert kinds[1] > kinds[R - 1] > kinds["wide"]


def test_spmv_reference_on_a_hand_example():
    offs, cols, coeffs = S.csr_from_rows(
        [[(0, 2), (1, 3)], [], [(1, R - 1), (1, 1)], [(2, 5), (2, 5)]])
    z = [7, 11, R - 1]
    assert S.spmv(offs, cols, coeffs, z, 8) == \
        [47, 0, 0, R - 10, 0, 0, 0, 0]


def test_r1cs_entry_points_without_a_device():
    import ethrex_amd
    from ethrex_amd import lib
    p = ctypes.c_void_p()
    create = lib._lib.ethrex_mi355_r1cs_plan_create
    sz = ctypes.c_size_t
    # argument checks come before the device check
    assert create(sz(0), sz(4), ctypes.byref(p)) == lib.EM_ERR_INPUT
    assert create(sz(12), sz(4), ctypes.byref(p)) == lib.EM_ERR_INPUT
    assert create(sz(16), sz(0), ctypes.byref(p)) == lib.EM_ERR_INPUT
    assert create(sz(16), sz(1 << 32), ctypes.byref(p)) == lib.EM_ERR_INPUT
    assert create(sz(16), sz(4), None) == lib.EM_ERR_INPUT
    if ethrex_amd.device_count() == 0:
        with pytest.raises(lib.HipCoreError) as ei:
            ethrex_amd.R1csPlan(16, 4)
        assert ei.value.rc == lib.EM_ERR_HIP
    else:
        ethrex_amd.R1csPlan(16, 4).destroy()
