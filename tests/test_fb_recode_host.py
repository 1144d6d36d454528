"""Host check of the merged fixed-base digit recode: builds
ethrex_amd/tools/fb_recode_check.cpp for the host (no GPU needed) and runs
it, once plain and once under UBSan + ASan.  For c in {20, 22, 24} the
signed digits of 10^5 random scalars below r and of the edge set must
rebuild the scalar exactly, stay within |d| <= 2^(c-1), and never carry
out of the top window.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "ethrex_amd", "tools", "fb_recode_check.cpp")
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


def test_fb_recode_host(tmp_path):
    out = _build_and_run(tmp_path, "fb_recode_check", [])
    for c in (20, 22, 24):
        assert f"c={c} ok" in out


def test_fb_recode_host_sanitized(tmp_path):
    _build_and_run(tmp_path, "fb_recode_check_san",
                   ["-Xarch_host", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-g"])
