"""The trajectory operator (qmri_set_operator_nufft) against the gridded one, on one MI355X.

Workload: 224^2, s = 10, T = 200, the exact spiral (771 points per frame, m = 154 200) and its gridded mask (m = 123 604).
Run mode (GPU) prints one JSON line:
  fwd_ms / adj_ms            qmri_forward_dev / qmri_adjoint_dev on device arrays, one slice, best of 20 (each call synchronised)
  admm_ms_per_iter           qmri_pnp_admm wall time / iterations, one slice, single coil (the exact spiral runs the image-domain LSQR with one unit
                             coil, the gridded mask the k-space LSQR), with the LSQR counts
  admm_ms_per_iter_mc8       qmri_pnp_admm_mc with 8 coils on the exact spiral
Trace mode (CPU) reads a `rocprofv3 --kernel-trace` of `--transforms-only` and prints per kernel calls and mean / max microseconds.

    python tools/nufft_times.py [--iters 3]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/nufft_times.py --transforms-only [--seg 256]
    python tools/nufft_times.py --trace OUT/.../kernel_trace.csv
"""
import argparse
import csv
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, T, S_INT, s = 224, 200, 771, 10


def parse_trace(path):
    per = {}
    for r in csv.DictReader(open(path)):
        name = r.get("Kernel_Name", "")
        mm = re.search(r"(k_nu_[a-z_]+|k_fwd_[hw]|k_adj_[hw])", name)
        if not mm:
            continue
        per.setdefault(mm.group(1), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    return {k: {"calls": len(v), "mean_us": round(float(np.mean(v)), 2), "max_us": round(float(np.max(v)), 2)} for k, v in sorted(per.items())}


def best_ms(fn, reps):
    best = 1e30
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--transforms-only", action="store_true")
    ap.add_argument("--trace")
    ap.add_argument("--seg", type=int, default=0, help="samples per spreading segment (knob nufft_seg; 0: the default)")
    a = ap.parse_args()
    if a.trace:
        print(json.dumps(parse_trace(a.trace)))
        return
    import torch
    from qmri_pnp_recon_poc_amd import engine as E, synth
    dic = synth.make_dictionary(T=T, n_t1=24, n_t2=16, s=s)
    X0 = synth.synthesize_tsmi(synth.make_phantom_qmaps(N, seed=0), dic)
    fpt, om = E.build_spiral_traj(N, S_INT, T)
    fpg, kg = E.build_spiral(N, S_INT, T)
    e = E.Engine(0)
    L = e.L
    if a.seg:
        e._check(L.qmri_debug_knob(b"nufft_seg", a.seg))
    out = {"N": N, "s": s, "T": T, "m_exact": int(fpt[-1]), "m_gridded": int(fpg[-1]), "nufft_seg": a.seg or 512}
    x = torch.from_numpy(np.asfortranarray(X0).ravel(order="F").astype(np.complex128)).cuda()
    for name, setup in (("exact", lambda: e.set_trajectory(N, N, dic["V"], fpt, om)), ("gridded", lambda: e.set_operator(N, N, dic["V"], fpg, kg))):
        setup()
        y = torch.zeros(e.m, dtype=torch.complex128, device="cuda")
        xa = torch.zeros_like(x)
        torch.cuda.synchronize()

        def fwd():
            e._check(L.qmri_forward_dev(e.h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), 1)); e.synchronize()

        def adj():
            e._check(L.qmri_adjoint_dev(e.h, C.c_void_p(y.data_ptr()), C.c_void_p(xa.data_ptr()), 1)); e.synchronize()
        fwd(); adj()
        reps = 5 if a.transforms_only else 20
        out[name] = {"fwd_ms": round(best_ms(fwd, reps), 4), "adj_ms": round(best_ms(adj, reps), 4)}
    if a.transforms_only:
        print(json.dumps(out))
        return
    w = synth.structured_weights(in_nc=s, out_nc=s, seed=3, eps=0.05)
    for name in ("exact", "gridded"):
        if name == "exact":
            e.set_trajectory(N, N, dic["V"], fpt, om)
        else:
            e.set_operator(N, N, dic["V"], fpg, kg)
        e.set_denoiser(w, N, N)
        y = e.forward(X0)
        e.pnp_admm(y, iters=1)
        t0 = time.perf_counter()
        _, _, li = e.pnp_admm(y, iters=a.iters)
        out[name]["admm_ms_per_iter"] = round((time.perf_counter() - t0) * 1e3 / a.iters, 2)
        out[name]["lsqr_iters"] = [int(v) for v in li]
    e.set_trajectory(N, N, dic["V"], fpt, om)
    e.set_denoiser(w, N, N)
    hh, ww = np.meshgrid(np.linspace(-1, 1, N), np.linspace(-1, 1, N), indexing="ij")
    maps = np.stack([np.exp(-((hh - np.cos(t)) ** 2 + (ww - np.sin(t)) ** 2)) for t in np.linspace(0, 2 * np.pi, 8, endpoint=False)], axis=2)
    maps = maps / np.sqrt(np.sum(maps ** 2, axis=2, keepdims=True))
    e.set_coils(maps)
    ymc = e.forward_mc(X0)
    e.pnp_admm_mc(ymc, iters=1)
    t0 = time.perf_counter()
    _, li = e.pnp_admm_mc(ymc, iters=a.iters)
    out["exact"]["admm_ms_per_iter_mc8"] = round((time.perf_counter() - t0) * 1e3 / a.iters, 2)
    out["exact"]["lsqr_iters_mc8"] = [int(v) for v in li]
    e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
