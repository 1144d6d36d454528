#!/usr/bin/env python3
"""BN254 G2 MSM benchmark (the flagship bench.py stays the G1 yardstick).

Times the G2 MSM at 2^17, 2^20 and 2^22, synchronous and pipelined, with
whichever libethrex_mi355.so --lib names (default: the in-tree build), and
prints one JSON line per size.  For the fused-vs-Karatsuba A/B build the
variant library once and point --lib at it:

    python ethrex_amd/tools/bench_g2.py --build-variant build/g2_karatsuba
    python ethrex_amd/tools/bench_g2.py --lib build/g2_karatsuba/libethrex_mi355.so

--build-variant compiles only api_msm_bn254_g2.hip with -DEM_FQ2_KARATSUBA
and links it against the in-tree objects of the other translation units.
--g1 adds the G1 time at the same n, for context.

Method: one warm-up run, then --reps timed runs; median and min..max are
reported.  adds/s is computed as for G1: NWIN * n point adds per MSM over
the bucket-walk time (last_times[1]).
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(REPO, "ethrex_amd", "csrc")
OTHER_OBJS = ["api_core.o", "api_msm_bn254.o", "api_msm_bls.o", "api_msm_g2.o",
              "api_ntt.o", "api_keccak.o"]


def build_variant(outdir):
    os.makedirs(outdir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "hipcc")
    obj = os.path.join(outdir, "api_msm_bn254_g2.o")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17",
                    "-fPIC", "-DEM_FQ2_KARATSUBA", "-c",
                    os.path.join(CSRC, "api_msm_bn254_g2.hip"), "-o", obj],
                   check=True, cwd=CSRC)
    subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o",
                    os.path.join(outdir, "libethrex_mi355.so"),
                    *[os.path.join(CSRC, o) for o in OTHER_OBJS], obj],
                   check=True)


class Plan:
    """minimal binding over an explicitly chosen library"""

    def __init__(self, lib, prefix, n, out_bytes):
        self.lib, self.pre, self.n, self.ob = lib, prefix, n, out_bytes
        self.p = ctypes.c_void_p()
        self._call("plan_create", ctypes.c_size_t(n), ctypes.byref(self.p),
                   plan=False)
        self.bufs = []

    def _call(self, name, *args, plan=True):
        f = getattr(self.lib, f"ethrex_mi355_{self.pre}_{name}")
        f.restype = ctypes.c_int
        rc = f(self.p, *args) if plan else f(*args)
        if rc != 0:
            raise RuntimeError(f"{self.pre}_{name}: rc={rc}")

    def gen_points(self):
        self._call("gen_points", ctypes.c_uint64(0))

    def upload_scalars(self, b):
        self._call("upload_scalars", (ctypes.c_uint8 * len(b)).from_buffer_copy(b))

    def run(self):
        out = (ctypes.c_uint8 * self.ob)()
        self._call("run", out)
        return bytes(out)

    def run_async(self):
        out = (ctypes.c_uint8 * self.ob)()
        self.bufs.append(out)
        self._call("run_async", out)

    def sync(self):
        self._call("sync")
        outs, self.bufs = self.bufs, []
        return bytes(outs[-1])

    def times(self):
        t = (ctypes.c_double * 5)()
        self._call("last_times", t)
        return list(t)

    def destroy(self):
        self._call("plan_destroy")


def spread(xs):
    return {"median": round(statistics.median(xs), 4),
            "min": round(min(xs), 4), "max": round(max(xs), 4)}


def bench(lib, prefix, out_bytes, n, reps, pipe_steps, nwin):
    scal = (ctypes.c_uint8 * (32 * n))()
    lib.ethrex_mi355_gen_fr(ctypes.c_uint64(42), ctypes.c_size_t(n), scal)
    plan = Plan(lib, prefix, n, out_bytes)
    plan.gen_points()
    plan.upload_scalars(bytes(scal))
    ref = plan.run()  # warm-up
    total, walk, sort, red = [], [], [], []
    for _ in range(reps):
        assert plan.run() == ref
        t = plan.times()
        sort.append(t[0]), walk.append(t[1]), red.append(t[2]), total.append(t[4])
    for _ in range(2):  # pipelined warm-up (graph capture)
        plan.run_async()
    plan.sync()
    pipe = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(pipe_steps):
            plan.run_async()
        got = plan.sync()
        pipe.append((time.perf_counter() - t0) * 1e3 / pipe_steps)
        assert got == ref
    plan.destroy()
    w = statistics.median(walk)
    return {"curve": prefix, "n": n, "nwin": nwin, "reps": reps,
            "sync_total_ms": spread(total), "digits_sort_ms": spread(sort),
            "bucket_acc_ms": spread(walk), "reduce_ms": spread(red),
            "pipelined_step_ms": spread(pipe),
            "walk_adds_per_s": round(nwin * n / (w * 1e-3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(REPO, "ethrex_amd",
                                                  "libethrex_mi355.so"))
    ap.add_argument("--build-variant", metavar="DIR")
    ap.add_argument("--logn", type=int, nargs="*", default=[17, 20, 22])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--pipe-steps", type=int, default=4)
    ap.add_argument("--g1", action="store_true")
    a = ap.parse_args()
    if a.build_variant:
        build_variant(a.build_variant)
        return 0
    lib = ctypes.CDLL(os.path.abspath(a.lib))
    for ln in a.logn:
        n = 1 << ln
        nwin = 32 if n <= 65536 else 15
        r = bench(lib, "bn254_g2_msm", 128, n, a.reps, a.pipe_steps, nwin)
        r["lib"] = os.path.relpath(os.path.abspath(a.lib), REPO)
        print(json.dumps(r), flush=True)
        if a.g1:
            r = bench(lib, "msm", 64, n, a.reps, a.pipe_steps, nwin)
            print(json.dumps(r), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
