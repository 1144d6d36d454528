"""Host check of the R1CS matrix packing: builds
ethrex_amd/tools/r1cs_pack_check.cpp for the host (no GPU needed) and runs
it, once plain and once under UBSan + ASan.  For random and edge CSR
matrices and several (threshold, chunk) geometries the packed form must
unpack to exactly the CSR's (row, col, coeff) multiset, put every row in
exactly one bin, keep padding inert, keep ids 0/1 = +1/r-1, and every
malformed input of the ABI must be rejected.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "ethrex_amd", "tools", "r1cs_pack_check.cpp")
INC = os.path.join(REPO, "ethrex_amd", "csrc")

HIPCC = shutil.which("hipcc") or (
    "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc not found")


def _build_and_run(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cmd = [HIPCC, "-x", "hip", "--offload-host-only", "-O2", "-std=c++17",
           "-I", INC, *extra, SRC, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "all cases agree" in r.stdout
    return r.stdout


def test_r1cs_pack_host(tmp_path):
    out = _build_and_run(tmp_path, "r1cs_pack_check", [])
    assert "12 malformed inputs rejected" in out


def test_r1cs_pack_host_sanitized(tmp_path):
    _build_and_run(tmp_path, "r1cs_pack_check_san",
                   ["-Xarch_host", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-g"])
