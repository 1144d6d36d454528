"""Host check of the merged fixed-base bucket partition: builds
ethrex_amd/tools/fbm_partition_check.cpp for the host (no GPU needed) and
runs it, once plain and once under UBSan + ASan.  It emulates the three
count/scan/scatter passes through csrc/msm_fbm_partition.h for c in
{20, 22, 24}, unit sizes T in {1, 7, 256} and the inputs random, all equal,
all zero, keys < 1024 and the maximum key: every write stays inside its
bin's range, the output is a permutation of the values grouped by key, and
the offsets equal the prefix counts.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "ethrex_amd", "tools", "fbm_partition_check.cpp")
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


def test_fbm_partition_host(tmp_path):
    out = _build_and_run(tmp_path, "fbm_partition_check", [])
    for c in (20, 22, 24):
        assert f"c={c} ok" in out


def test_fbm_partition_host_sanitized(tmp_path):
    _build_and_run(tmp_path, "fbm_partition_check_san",
                   ["-Xarch_host", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-g"])
