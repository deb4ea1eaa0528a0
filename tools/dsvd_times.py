#!/usr/bin/env python3
"""Set-up time of the dictionary compression (qmri_dict_compress_dev) per stage and per kernel.

    python3 tools/dsvd_times.py [--K 98304] [--T 200 1000] [--s 10] [--reps 3] [--baseline] [--kernels] [--out profiles/dsvd_times.json]

Per T: F (K x T fp64, the synthetic fingerprints of synth.make_dictionary on a 384 x 256 grid when K = 98304) is put on the device once; then, on
the host clock around calls that return after their kernels have finished (best of --reps):
  gram_ms      G = F^T F alone (qmri_debug_dsvd_gram on device arrays: k_dsvd_gram + k_dsvd_gram_reduce), with its fp64 TFLOP/s counted as 2 K T^2
               (the full square: what the matrix stands for; the kernel computes the upper block triangle, flops_done says how much)
  total_ms     the whole call; rest_ms = total - gram: the subspace iteration (host Rayleigh-Ritz + k_dsvd_gq) and the projection
  iters        subspace iterations taken, max_resid
--kernels runs this script again under `rocprofv3 --kernel-trace --stats` (a run of its own) and adds the mean duration of every k_dsvd_* kernel,
with k_dsvd_project's TB/s over the K T 8 bytes of F.  --baseline adds numpy's eigh(F.T @ F) and F @ V on the host's threads.
Writes one JSON document."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def hip_lib():
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


def fingerprints(K, T):
    from qmri_pnp_recon_poc_amd import synth
    n2 = 256 if K % 256 == 0 else 1
    dic = synth.make_dictionary(T=T, n_t1=K // n2, n_t2=n2, uncompressed=True)
    return dic["D"].astype(np.float64) * dic["normD"].astype(np.float64)[:, None]


def measure(K, T, s, reps, baseline):
    from qmri_pnp_recon_poc_amd import engine
    from qmri_pnp_recon_poc_amd._lib import DsvdInfo, DsvdParams
    F = fingerprints(K, T)
    Fb = np.asfortranarray(F).ravel(order="F")
    eng, hip = engine.Engine(0), hip_lib()
    d_F, d_G, d_V, d_D, d_n = (C.c_void_p() for _ in range(5))
    for d, nb in ((d_F, Fb.nbytes), (d_G, T * T * 8), (d_V, T * 16 * 8), (d_D, K * 16 * 4), (d_n, K * 4)):
        assert hip.hipMalloc(C.byref(d), nb) == 0
    out = {"K": K, "T": T, "s": s}
    try:
        t0 = time.perf_counter()
        assert hip.hipMemcpy(d_F, Fb.ctypes.data, Fb.nbytes, 1) == 0
        out["upload_ms"] = 1e3 * (time.perf_counter() - t0)
        p, info, got, eig = DsvdParams(s, 16, 0.0, 0.0, 0), DsvdInfo(), C.c_int(0), np.empty(16)
        gram, total = [], []
        for _ in range(reps + 1):                                    # (the first pass warms up: code objects, allocator)
            t0 = time.perf_counter()
            eng._check(eng.L.qmri_debug_dsvd_gram(eng.h, K, T, d_F, 1, 1, d_G))
            t1 = time.perf_counter()
            eng._check(eng.L.qmri_dict_compress_dev(eng.h, K, T, d_F, 1, C.byref(p), C.byref(got), d_V, d_D, d_n, eig.ctypes.data_as(C.c_void_p), C.byref(info)))
            t2 = time.perf_counter()
            gram.append(1e3 * (t1 - t0))
            total.append(1e3 * (t2 - t1))
        g, t = min(gram[1:]), min(total[1:])
        nblk = (T + 63) // 64
        out.update(gram_ms=g, total_ms=t, rest_ms=t - g, gram_tflops=2.0 * K * T * T / (g * 1e-3) / 1e12,
                   flops_done=2.0 * K * 64 * 64 * nblk * (nblk + 1) / 2, iters=int(info.iters), converged=int(info.converged), max_resid=float(info.max_resid))
    finally:
        for d in (d_F, d_G, d_V, d_D, d_n):
            hip.hipFree(d)
        eng.close()
    if baseline:
        t0 = time.perf_counter()
        lam, U = np.linalg.eigh(F.T @ F)
        V = U[:, ::-1][:, :s]
        t1 = time.perf_counter()
        Dc = F @ V
        Dc /= np.linalg.norm(Dc, axis=1)[:, None]
        t2 = time.perf_counter()
        out["numpy"] = {"gram_eigh_ms": 1e3 * (t1 - t0), "project_ms": 1e3 * (t2 - t1), "threads": int(os.environ.get("OMP_NUM_THREADS", "0"))}
    return out


def kernel_stats(K, T, s):
    """mean duration (us) per k_dsvd_* kernel from a rocprofv3 --kernel-trace --stats run of this script"""
    with tempfile.TemporaryDirectory() as d:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                        "--K", str(K), "--T", str(T), "--s", str(s), "--reps", "2", "--out", os.path.join(d, "child.json")], check=True, capture_output=True, timeout=900)
        rows = {}
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                if "k_dsvd" in r["Name"]:
                    name = r["Name"][r["Name"].index("k_dsvd"):].split("(")[0].split("<")[0]
                    rows[name] = {"calls": int(r["Calls"]), "mean_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3}
        return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=98304)
    ap.add_argument("--T", type=int, nargs="+", default=[200, 1000])
    ap.add_argument("--s", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dsvd_times.json"))
    a = ap.parse_args()
    runs = []
    for T in a.T:
        r = measure(a.K, T, a.s, a.reps, a.baseline)
        if a.kernels:
            try:
                r["kernels"] = kernel_stats(a.K, T, a.s)
            except (subprocess.SubprocessError, OSError, KeyError, ValueError) as e:
                r["kernels"], r["kernels_error"] = {}, repr(e)[:400]
            pr = r["kernels"].get("k_dsvd_project")
            if pr:
                r["project_tb_per_s"] = a.K * T * 8 / (pr["min_us"] * 1e-6) / 1e12
            gr = r["kernels"].get("k_dsvd_gram")
            if gr:
                r["gram_kernel_tflops"] = 2.0 * a.K * T * T / (gr["min_us"] * 1e-6) / 1e12
        runs.append(r)
        print(json.dumps(r))
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/dsvd_times.py", "device": "MI355X", "runs": runs}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
