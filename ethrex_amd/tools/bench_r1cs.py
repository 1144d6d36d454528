"""Measurements behind profiles/r1cs.md: eval time of A z, B z, C z
(R1csPlan, HIP events) next to the bytes bound, to the three host uploads
the step replaces and to quot_run; the threshold / chunk sweep; +-1-only
against all-general coefficients.  Not wired into bench.py.

    python ethrex_amd/tools/bench_r1cs.py eval --log2 20 --fan-in 3
    python ethrex_amd/tools/bench_r1cs.py eval --log2 22 --fan-in 8 --skew
    python ethrex_amd/tools/bench_r1cs.py sweep
    python ethrex_amd/tools/bench_r1cs.py classes

Instances.  --gen chain is product-chain circuit v1 (ethrex_amd/r1cs.py,
Python PRNG; slow to generate above 2^20); --gen numpy (the default) draws
the same shape — fan_in columns below wire 1+k+i per A/B row, the 7:4:3:2
coefficient mix, C_i = (1+k+i, 1) — from numpy's PRNG.  The witness values
do not change the work, so z is gen_fr, not the satisfying assignment.
--skew replaces the last 64 rows of A and B by rows of 2^16 entries.
Every line printed is one JSON object.
"""
import argparse
import array
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__)))))

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
HBM_TBS = 6.29   # the project's measured-achievable stream rate, TB/s
K = 64


def _coeff_bytes(rng, nnz, mix):
    """nnz x 32 big-endian bytes; mix = 'chain' | 'pm1' | 'general'"""
    out = np.zeros((nnz, 32), dtype=np.uint8)
    if mix == "chain":
        u = rng.integers(0, 16, nnz)
    elif mix == "pm1":
        u = rng.integers(0, 11, nnz)
    else:
        u = np.full(nnz, 15)
    out[u < 7, 31] = 1
    out[(u >= 7) & (u < 11)] = np.frombuffer((R - 1).to_bytes(32, "big"),
                                              dtype=np.uint8)
    small = (u >= 11) & (u < 14)
    out[small, 31] = rng.integers(2, 17, int(small.sum()))
    wide = u >= 14
    w = rng.integers(0, 256, (int(wide.sum()), 32), dtype=np.uint8)
    w[:, 0] &= 0x1f          # < 2^253 < r
    out[wide] = w
    return out


def _matrix(rng, lengths, avail, mix):
    """CSR with the given row lengths; row i draws columns below avail[i]"""
    offs = np.zeros(len(lengths) + 1, dtype=np.uint64)
    np.cumsum(lengths, out=offs[1:])
    nnz = int(offs[-1])
    hi = np.repeat(avail, lengths).astype(np.float64)
    cols = np.minimum((rng.random(nnz) * hi).astype(np.uint32),
                      (hi - 1).astype(np.uint32))
    a = array.array("I")
    a.frombytes(cols.tobytes())
    o = array.array("Q")
    o.frombytes(offs.tobytes())
    return o, a, _coeff_bytes(rng, nnz, mix).tobytes()


def numpy_instance(n, fan_in, skew, mix="chain", seed=1):
    rng = np.random.default_rng(seed)
    avail = 1 + K + np.arange(n, dtype=np.int64)
    lengths = np.full(n, fan_in, dtype=np.int64)
    if skew:
        lengths[-64:] = 1 << 16
    mats = [_matrix(rng, lengths, avail, mix) for _ in range(2)]
    o = array.array("Q", range(n + 1))
    c = array.array("I")
    c.frombytes(avail.astype(np.uint32).tobytes())
    one = np.zeros((n, 32), dtype=np.uint8)
    one[:, 31] = 1
    mats.append((o, c, one.tobytes()))
    return mats, 1 + K + n


def chain_instance(n, fan_in):
    from ethrex_amd import r1cs as C
    mats, _ = C.chain_circuit(n, K, fan_in, 1)
    return [(m[0], m[1], C.fr_bytes(m[2])) for m in mats], 1 + K + n


def ramp_instance(rows, max_len, seed=2):
    """row lengths log-uniform in [1, max_len]: rows on both sides of every
    threshold the sweep tries"""
    rng = np.random.default_rng(seed)
    lengths = np.exp(rng.random(rows) * np.log(max_len)).astype(np.int64)
    m = 1 << 20
    return _matrix(rng, lengths, np.full(rows, m, dtype=np.int64), "chain"), m


def _stats(v):
    return {"median": round(statistics.median(v), 4),
            "min": round(min(v), 4), "max": round(max(v), 4)}


def _time_evals(rp, whiches, warmup, reps):
    names = ("a_ms", "b_ms", "c_ms")
    per = {w: [] for w in whiches}
    for it in range(warmup + reps):
        for w in whiches:
            rp.eval(w)
            if it >= warmup:
                per[w].append(rp.last_times()[names[w]])
    return per


def cmd_eval(args):
    import ethrex_amd as ea
    ea.set_device(0)
    n = 1 << args.log2
    t0 = time.perf_counter()
    if args.gen == "chain":
        mats, m = chain_instance(n, args.fan_in)
    else:
        mats, m = numpy_instance(n, args.fan_in, args.skew)
    gen_s = time.perf_counter() - t0
    rp = ea.R1csPlan(n, m)
    qp = ea.QuotPlan(n)
    t0 = time.perf_counter()
    for w, (o, c, k) in enumerate(mats):
        rp.upload_matrix(w, o, c, k)
    upload_s = time.perf_counter() - t0
    rp.upload_witness(ea.gen_fr(5, m))
    per = _time_evals(rp, (0, 1, 2), args.warmup, args.reps)
    total = [sum(per[w][i] for w in range(3)) for i in range(args.reps)]
    nnz = [len(mt[1]) for mt in mats]
    # bytes bound: 8 B per stored entry + a 32-B gather per nonzero + the
    # 32-B result per row.  Stored = nnz + padding; this instance's short
    # rows all have one length, so it has no padding.
    bound_ms = [(8 * z + 32 * z + 32 * n) / (HBM_TBS * 1e9) for z in nnz]
    # what the step replaces: three host vectors through quot_upload
    host = [ea.gen_fr(10 + w, n) for w in range(3)]
    up, run, d2d = [], [], []
    for it in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        for w in range(3):
            qp.upload(w, host[w])
        t1 = time.perf_counter()
        rp.eval_all()
        t2 = time.perf_counter()
        for w in range(3):
            qp.load_from_r1cs(w, rp, w)
        t3 = time.perf_counter()
        qp.run()
        if it >= args.warmup:
            up.append((t1 - t0) * 1e3)
            d2d.append((t3 - t2) * 1e3)
            run.append(qp.last_times()["total_ms"])
    out = {"bench": "r1cs_eval", "log2": args.log2, "fan_in": args.fan_in,
           "skew": bool(args.skew), "gen": args.gen, "nnz": nnz,
           "gen_s": round(gen_s, 2), "upload_matrices_s": round(upload_s, 2),
           "eval_a_ms": _stats(per[0]), "eval_b_ms": _stats(per[1]),
           "eval_c_ms": _stats(per[2]), "eval_abc_ms": _stats(total),
           "bytes_bound_abc_ms": round(sum(bound_ms), 4),
           "fraction_of_bound": round(sum(bound_ms) /
                                      statistics.median(total), 3),
           "quot_upload_x3_wall_ms": _stats(up),
           "load_from_r1cs_x3_wall_ms": _stats(d2d),
           "quot_run_total_ms": _stats(run)}
    print(json.dumps(out), flush=True)
    rp.destroy()
    qp.destroy()


def cmd_sweep_child(args):
    import ethrex_amd as ea
    ea.set_device(0)
    (o, c, k), m = ramp_instance(1 << 15, 2048)
    mats, m2 = numpy_instance(1 << 20, 3, True)
    res = {"bench": "r1cs_sweep", "T": os.environ.get("EM_R1CS_T"),
           "chunk": os.environ.get("EM_R1CS_CHUNK")}
    rp = ea.R1csPlan(1 << 15, m)
    rp.upload_matrix(0, o, c, k)
    rp.upload_witness(ea.gen_fr(5, m))
    res["ramp_nnz"] = len(c)
    res["ramp_ms"] = _stats(_time_evals(rp, (0,), 2, args.reps)[0])
    rp.destroy()
    rp = ea.R1csPlan(1 << 20, m2)
    rp.upload_matrix(0, *mats[0])
    rp.upload_witness(ea.gen_fr(5, m2))
    res["skew_2_20_ms"] = _stats(_time_evals(rp, (0,), 2, args.reps)[0])
    rp.destroy()
    print(json.dumps(res), flush=True)


def cmd_sweep(args):
    geoms = [(t, 1024) for t in (8, 32, 64, 128, 512)] + \
            [(64, c) for c in (256, 4096)] + [(0, 1024), (1 << 30, 1024)]
    for t, c in geoms:
        env = dict(os.environ, EM_R1CS_T=str(t), EM_R1CS_CHUNK=str(c))
        r = subprocess.run([sys.executable, os.path.abspath(__file__),
                            "sweep-child", "--reps", str(args.reps)], env=env,
                           capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            print(json.dumps({"bench": "r1cs_sweep", "T": t, "chunk": c,
                              "error": r.stderr[-500:]}), flush=True)
            return 1
        print(r.stdout.strip(), flush=True)
    return 0


def cmd_classes(args):
    import ethrex_amd as ea
    ea.set_device(0)
    n = 1 << args.log2
    for mix in ("pm1", "general", "chain"):
        mats, m = numpy_instance(n, args.fan_in, False, mix)
        rp = ea.R1csPlan(n, m)
        rp.upload_matrix(0, *mats[0])
        rp.upload_witness(ea.gen_fr(5, m))
        t = _time_evals(rp, (0,), args.warmup, args.reps)[0]
        print(json.dumps({"bench": "r1cs_classes", "mix": mix,
                          "log2": args.log2, "fan_in": args.fan_in,
                          "nnz": len(mats[0][1]), "eval_ms": _stats(t)}),
              flush=True)
        rp.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["eval", "sweep", "sweep-child", "classes"])
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--fan-in", type=int, default=3)
    ap.add_argument("--skew", action="store_true")
    ap.add_argument("--gen", choices=["numpy", "chain"], default="numpy")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    fn = {"eval": cmd_eval, "sweep": cmd_sweep, "sweep-child": cmd_sweep_child,
          "classes": cmd_classes}[args.cmd]
    return fn(args) or 0


if __name__ == "__main__":
    sys.exit(main())
