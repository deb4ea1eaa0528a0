#!/usr/bin/env python3
"""Time of the slice-profile-aware FISP dictionary simulation (qmri_dict_simulate_sp_dev): the whole call, its kernel, and
the two ways to get the same fingerprints without it.

    python3 tools/epgsp_times.py [--K 98304] [--T 200 1000] [--S 32] [--Q 4 16] [--reps 3] [--kernels] [--out profiles/epgsp_times.json]

This process never opens the GPU.  Per (T, S, Q) it starts one child (this script with --child) under `timeout -k 10`, and with --kernels a second
one under `rocprofv3 --kernel-trace --stats` (a run of its own, the program after `--`), again under its own `timeout -k 10`.  The steps are
chained: the first child that fails, is killed or runs out of time ends the tool with its exit status, and what was measured until then is written.
A child uses at most 16 host threads.

The child puts t1, t2 (a 384 x 256 log-spaced grid when K = 98304) on the device once; then, on the host clock around calls that return after
their kernel has finished (best of --reps after one warm-up call):
  call_ms        qmri_dict_simulate_sp_dev with a per-frame profile of synth.rf_slice_profile, fp64 output left on the device
  plain_call_ms  qmri_dict_simulate_dev at the same K, T, S (k_epg, which this feature leaves untouched); ratio_to_q_plain = call_ms / (Q plain_call_ms)
  today_ms       what a caller could do before: Q plain calls with b1 p_q into a K x T x Q device buffer, then the weighted sum over q through torch
                 (a frame-constant profile: the only kind this route can express); today_buffer_gb is that buffer; skipped when it does not fit
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
THREADS = 16


def atoms(K):
    import numpy as np
    n2 = 256 if K % 256 == 0 else 1
    t1 = np.exp(np.linspace(np.log(0.1), np.log(4.0), K // n2))
    t2 = np.exp(np.linspace(np.log(0.01), np.log(0.6), n2))
    return tuple(np.ascontiguousarray(a.ravel()) for a in np.meshgrid(t1, t2, indexing="ij"))


def sinc_envelope(P=32, tbw=4.0):
    import numpy as np
    x = (np.arange(P) + 0.5) / P - 0.5
    return np.sinc(tbw * x) * (0.54 + 0.46 * np.cos(2 * np.pi * x))


def child(K, T, S, Q, reps, today):
    import numpy as np
    from qmri_pnp_recon_poc_amd import engine, synth
    from qmri_pnp_recon_poc_amd._lib import EpgParams
    t1, t2 = atoms(K)
    alpha, tr, te = synth.flip_angle_train(T), np.full(T, 0.012), np.full(T, 0.002)
    prof, w = synth.rf_slice_profile(alpha, sinc_envelope(), 4.0, Q)
    keep = engine.slice_profile_arguments(prof, w, T)
    eng, hip = engine.Engine(0), engine._hip_runtime()
    d_t1, d_t2, d_F = (C.c_void_p() for _ in range(3))
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    out = {"K": K, "T": T, "S": S, "Q": Q}

    def best_ms(call):
        times = []
        for _ in range(reps + 1):                                    # (the first pass warms up: code objects, allocator)
            t0 = time.perf_counter()
            call()
            times.append(1e3 * (time.perf_counter() - t0))
        return min(times[1:]), times[0]
    try:
        for d, nb in ((d_t1, K * 8), (d_t2, K * 8), (d_F, K * T * 8)):
            assert hip.hipMalloc(C.byref(d), nb) == 0
        assert hip.hipMemcpy(d_t1, t1.ctypes.data, K * 8, 1) == 0 and hip.hipMemcpy(d_t2, t2.ctypes.data, K * 8, 1) == 0
        p = EpgParams(S, 1, 0.0, 1.0, 1)
        head = (eng.h, K, T, vp(alpha), vp(tr), vp(te), d_t1, d_t2)
        sp_ms, first = best_ms(lambda: eng._check(eng.L.qmri_dict_simulate_sp_dev(*head, None, C.byref(p), C.byref(keep[2]), d_F)))
        plain_ms, _ = best_ms(lambda: eng._check(eng.L.qmri_dict_simulate_dev(*head, None, C.byref(p), d_F)))
        out.update(call_ms=sp_ms, first_call_ms=first, plain_call_ms=plain_ms, ratio_to_q_plain=sp_ms / (Q * plain_ms),
                   gflops=24.0 * S * T * K * Q / (sp_ms * 1e-3) / 1e9)
        if today:
            import torch
            torch.set_num_threads(min(THREADS, torch.get_num_threads()))
            gb = K * T * Q * 8 / 1e9
            out["today_buffer_gb"] = gb
            free = torch.cuda.mem_get_info(0)[0] / 1e9
            if gb * 1.25 + 1.0 > free:
                out["today_skipped"] = "the K x T x Q buffer does not fit (%.1f GB free)" % free
            else:
                p0 = prof[0]                                         # frame-constant stand-in: the first frame's profile
                buf = torch.empty((Q, T, K), dtype=torch.float64, device="cuda:0")
                res = torch.empty((T, K), dtype=torch.float64, device="cuda:0")
                b1s = [torch.full((K,), float(p0[q]), dtype=torch.float64, device="cuda:0") for q in range(Q)]
                wt = torch.as_tensor(w, device="cuda:0")
                torch.cuda.synchronize()

                def route():
                    for q in range(Q):
                        eng._check(eng.L.qmri_dict_simulate_dev(*head, C.c_void_p(b1s[q].data_ptr()), C.byref(p), C.c_void_p(buf[q].data_ptr())))
                    torch.matmul(wt.view(1, Q), buf.view(Q, T * K), out=res.view(1, T * K))
                    torch.cuda.synchronize()
                out["today_ms"], _ = best_ms(route)
                out["today_over_call"] = out["today_ms"] / sp_ms
                del buf, res, b1s
    finally:
        for d in (d_t1, d_t2, d_F):
            hip.hipFree(d)
        eng.close()
    return out


def run_step(cmd, limit):
    """One GPU step under its own time limit; returns the exit status (124 / 137: the limit)."""
    env = dict(os.environ)
    for k in ("OMP_NUM_THREADS", "MKL_NUM_THREADS", "OPENBLAS_NUM_THREADS"):
        env[k] = str(min(THREADS, int(env.get(k, THREADS) or THREADS)))
    return subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=env).returncode


def kernel_stats(me, args, limit):
    """(exit status, {kernel: calls / mean / least duration in us}) from a rocprofv3 --kernel-trace --stats run of the child"""
    with tempfile.TemporaryDirectory() as d:
        rc = run_step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, me, "--child", "--no-today",
                       "--reps", "2", "--out", os.path.join(d, "child.json")] + args, limit)
        rows = {}
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                name = "k_epg_sp" if "k_epg_sp" in r["Name"] else "k_epg" if "k_epg" in r["Name"] and "shift" not in r["Name"] else None
                if name:
                    rows[name] = {"calls": int(r["Calls"]), "mean_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3}
        return rc, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=98304)
    ap.add_argument("--T", type=int, nargs="+", default=[200, 1000])
    ap.add_argument("--S", type=int, nargs="+", default=[32])
    ap.add_argument("--Q", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--child", action="store_true", help="measure one (T, S, Q) in this process")
    ap.add_argument("--no-today", action="store_true")
    ap.add_argument("--step-limit", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epgsp_times.json"))
    a = ap.parse_args()
    if a.child:
        r = child(a.K, a.T[0], a.S[0], a.Q[0], a.reps, not a.no_today)
        with open(a.out, "w") as f:
            json.dump(r, f)
        return 0
    me, runs, rc = os.path.abspath(__file__), [], 0
    for T in a.T:
        for S in a.S:
            for Q in a.Q:
                if rc:
                    break
                args = ["--K", str(a.K), "--T", str(T), "--S", str(S), "--Q", str(Q)]
                with tempfile.TemporaryDirectory() as d:
                    rc = run_step([sys.executable, me, "--child", "--reps", str(a.reps), "--out", os.path.join(d, "r.json")] + args, a.step_limit)
                    if rc:
                        print("step failed with status %d: T=%d S=%d Q=%d" % (rc, T, S, Q), flush=True)
                        break
                    r = json.load(open(os.path.join(d, "r.json")))
                if a.kernels:
                    rc, r["kernels"] = kernel_stats(me, args, a.step_limit)
                    k, k0 = r["kernels"].get("k_epg_sp"), r["kernels"].get("k_epg")
                    if k and k0:
                        r["kernel_ratio_to_q_plain"] = k["min_us"] / (Q * k0["min_us"])
                        r["kernel_gflops"] = 24.0 * S * T * a.K * Q / (k["min_us"] * 1e-6) / 1e9
                runs.append(r)
                print(json.dumps(r), flush=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/epgsp_times.py", "device": "MI355X", "runs": runs}, f, indent=1)
        f.write("\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
