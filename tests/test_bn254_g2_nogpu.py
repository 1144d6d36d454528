"""BN254 G2 entry points fail loudly (EM_ERR_HIP) when no GPU is present:
no CPU fallback."""
import pytest

import bn254_g2_reference as g2


def test_bn254_g2_fails_loudly_without_gpu():
    import ethrex_amd
    if ethrex_amd.device_count() > 0:
        pytest.skip("GPU present; the no-fallback check is for CPU-only hosts")
    g = g2.encode(g2.G2)
    rc, _ = ethrex_amd.bn254_g2_add(g, g)
    assert rc == ethrex_amd.EM_ERR_HIP
    rc, _ = ethrex_amd.bn254_g2_mul(g, (5).to_bytes(32, "big"))
    assert rc == ethrex_amd.EM_ERR_HIP
    rc, _ = ethrex_amd.bn254_g2_msm(g, b"\x01" * 32, 1)
    assert rc == ethrex_amd.EM_ERR_HIP
    with pytest.raises(ethrex_amd.lib.HipCoreError) as ei:
        ethrex_amd.Bn254G2MsmPlan(16)
    assert ei.value.rc == ethrex_amd.EM_ERR_HIP
