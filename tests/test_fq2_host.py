"""Host check of the BN254 Fq2 layer and G2 group operations: builds
ethrex_amd/tools/fq2_check.cpp for the host (no GPU needed) and runs it,
once plain and once under UBSan + ASan.  The program compares the fused
fq2_mul / fq2_sqr with the Karatsuba form and a schoolbook as canonical
values, audits the limb/value bound of every multiply input, and runs the
G2 add/double/cancel branches and r*G2 = O on the host.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "ethrex_amd", "tools", "fq2_check.cpp")
INC = os.path.join(REPO, "ethrex_amd", "csrc")

HIPCC = shutil.which("hipcc") or (
    "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not found")


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-O2", "-std=c++17",
           "-DEM_LAZY9_AUDIT", "-I", INC, *extra, SRC, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "all cases agree" in r.stdout
    return r.stdout


def test_fq2_host(tmp_path):
    out = _build_and_run(tmp_path, "fq2_check", [])
    for grp in ("random", "extreme", "chain", "group"):
        assert grp + " ok" in out


def test_fq2_host_sanitized(tmp_path):
    _build_and_run(tmp_path, "fq2_check_san",
                   ["-Xarch_host", "-fsanitize=undefined,address",
                    "-fno-sanitize-recover=undefined", "-g"])
