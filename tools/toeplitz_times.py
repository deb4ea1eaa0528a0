"""The Toeplitz normal operator and the solver "toeplitz"  against the NUFFT pair and the LSQR route, on one MI355X.

Workload: 224^2, s = 10, T = 200, the exact spiral (771 points per frame, m = 154 200), kernel width 12.  Prints one JSON line and writes it to
profiles/toeplitz_times.json:
  setup_ms                   qmri_nufft_prepare_normal (K^ built once per trajectory)
  normal_ms / pair_ms        qmri_normal_dev against qmri_adjoint_dev(qmri_forward_dev), one slice on device arrays, best of 20 (each call synchronised)
  admm_ms_per_iter[_mc8]     qmri_pnp_admm (one unit coil) / qmri_pnp_admm_mc (8 coils) wall time per iteration with solver "toeplitz" and "lsqr" in
                             the same build, with the solver iteration counts
Every step (set-up and apply, the ADMM loops with "toeplitz", the ADMM loops with "lsqr") runs as a child process of its own under
`timeout -k 10 <seconds>`; the first step that fails or runs out of time ends the run, and nothing more is started on the GPU.
`--apply-only` (one process: run it under a timeout of your own, as below) also applies a batch of two, so that a kernel trace holds both
k_toep_mul<1> and k_toep_mul<2>.  Trace mode (CPU) reads a `rocprofv3 --kernel-trace` of `--apply-only` and prints per kernel calls and
mean / max microseconds.

    python tools/toeplitz_times.py [--iters 3]
    timeout -k 10 240 \
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/toeplitz_times.py --apply-only
    python tools/toeplitz_times.py --trace OUT/.../kernel_trace.csv
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
N, T, S_INT, s = 224, 200, 771, 10


def parse_trace(path):
    import csv
    import re
    per = {}
    for r in csv.DictReader(open(path)):
        mm = re.search(r"(k_toep_mul<\d>|k_toep_[a-z_]+|k_nu_[a-z_]+|k_fwd_[hw]|k_adj_[hw])", r.get("Kernel_Name", ""))
        if mm:
            per.setdefault(mm.group(1), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    return {k: {"calls": len(v), "mean_us": round(float(np.mean(v)), 2), "max_us": round(float(np.max(v)), 2)} for k, v in sorted(per.items())}


STEP_LIMIT_S = {"apply": 120, "toeplitz": 240, "lsqr": 300}


def step(name, iters):
    """One step in this process: returns its part of the result."""
    import torch
    from nufft_times import best_ms
    from qmri_pnp_recon_poc_amd import engine as E, synth
    dic = synth.make_dictionary(T=T, n_t1=24, n_t2=16, s=s)
    X0 = synth.synthesize_tsmi(synth.make_phantom_qmaps(N, seed=0), dic)
    fpt, om = E.build_spiral_traj(N, S_INT, T)
    e = E.Engine(0)
    L = e.L
    out = {}
    if name in ("apply", "apply-only"):
        e.set_trajectory(N, N, dic["V"], fpt, om, max_batch=2, width=12)
        out.update({"N": N, "s": s, "T": T, "m": int(fpt[-1]), "width": 12})
        t0 = time.perf_counter()
        e.prepare_normal()
        e.synchronize()
        out["setup_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        x1 = torch.from_numpy(np.asfortranarray(X0).ravel(order="F").astype(np.complex128)).cuda()
        x = torch.cat([x1, x1.flip(0)])
        y = torch.zeros(2 * e.m, dtype=torch.complex128, device="cuda")
        xa, xn = torch.zeros_like(x), torch.zeros_like(x)
        torch.cuda.synchronize()
        vp = lambda t: C.c_void_p(t.data_ptr())

        def normal(B):
            e._check(L.qmri_normal_dev(e.h, vp(x), vp(xn), B)); e.synchronize()

        def pair(B):
            e._check(L.qmri_forward_dev(e.h, vp(x), vp(y), B)); e._check(L.qmri_adjoint_dev(e.h, vp(y), vp(xa), B)); e.synchronize()
        reps = 5 if name == "apply-only" else 20
        for B, tag in ((2, "_batch2"), (1, "")):
            normal(B); pair(B)
            out["normal_ms" + tag] = round(best_ms(lambda: normal(B), reps), 4)
            out["pair_ms" + tag] = round(best_ms(lambda: pair(B), reps), 4)
        n = x1.numel()
        out["normal_vs_pair_rel_err"] = float((torch.linalg.norm(xn[:n] - xa[:n]) / torch.linalg.norm(xa[:n])).item())
    else:
        e.set_trajectory(N, N, dic["V"], fpt, om, width=12)
        w = synth.structured_weights(in_nc=s, out_nc=s, seed=3, eps=0.05)
        e.set_denoiser(w, N, N)
        yv = e.forward(X0)
        hh, ww = np.meshgrid(np.linspace(-1, 1, N), np.linspace(-1, 1, N), indexing="ij")
        maps = np.stack([np.exp(-((hh - np.cos(t)) ** 2 + (ww - np.sin(t)) ** 2)) for t in np.linspace(0, 2 * np.pi, 8, endpoint=False)], axis=2)
        maps = maps / np.sqrt(np.sum(maps ** 2, axis=2, keepdims=True))
        e.pnp_admm(yv, iters=1, solver=name)
        t0 = time.perf_counter()
        _, _, li = e.pnp_admm(yv, iters=iters, solver=name)
        r = {"admm_ms_per_iter": round((time.perf_counter() - t0) * 1e3 / iters, 2), "solver_iters": [int(v) for v in li]}
        e.set_coils(maps)
        ymc = e.forward_mc(X0)
        e.pnp_admm_mc(ymc, iters=1, solver=name)
        t0 = time.perf_counter()
        _, li = e.pnp_admm_mc(ymc, iters=iters, solver=name)
        r["admm_ms_per_iter_mc8"] = round((time.perf_counter() - t0) * 1e3 / iters, 2)
        r["solver_iters_mc8"] = [int(v) for v in li]
        out[name] = r
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--apply-only", action="store_true")
    ap.add_argument("--step", choices=sorted(STEP_LIMIT_S))
    ap.add_argument("--trace")
    a = ap.parse_args()
    if a.trace:
        print(json.dumps(parse_trace(a.trace)))
        return 0
    if a.apply_only or a.step:
        print(json.dumps(step("apply-only" if a.apply_only else a.step, a.iters)))
        return 0
    out = {}
    for name in ("apply", "toeplitz", "lsqr"):                        # each under its own time limit; nothing is started after a failure
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S[name]), sys.executable, os.path.abspath(__file__), "--step", name, "--iters", str(a.iters)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(json.dumps({"failed_step": name, "returncode": r.returncode, **out}))
            return 1
        out.update(json.loads(r.stdout.strip().splitlines()[-1]))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    json.dump(out, open(os.path.join(ROOT, "profiles", "toeplitz_times.json"), "w"), indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
