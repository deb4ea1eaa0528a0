"""Off-resonance correction on one MI355X: what forward and adjoint cost with a field map of L segments beside the plain ones.

Workload: 224^2, s = 10, the exact spiral with S = 800 points per frame, T = 200 frames (m = 160 000), kernel width 12, a 5 ms readout and the field
100 (sin 2 pi a cos pi b + 0.6 b + 0.2) Hz.  Prints one JSON line and writes it to profiles/offres_times.json; per configuration (no map, L = 1, 4, 8):
  attach_ms                qmri_set_field_map (host histogram and factorisation, the coefficient and phase-map kernels), one call, wall clock
  forward_ms / adjoint_ms  qmri_forward_dev / qmri_adjoint_dev, one slice on device arrays
forward_ms / adjoint_ms are the median of 20 calls after 3 warm-ups, timed by a pair of events on the stream the library launches on.  Every
configuration runs as a child process of its own under `timeout -k 10 <seconds>`; the first one that fails or runs out of time ends the run, and
nothing more is started on the GPU.  L = 1 is a constant map (the only map one segment serves).

    python tools/offres_times.py

`--normal` measures the field-aware Toeplitz normal operator at the same shape with the map at L = 6, beside the plain one,
and writes profiles/offres_normal_times.json.  Three child processes, each under its own time limit as above:
  apply     setup_ms of qmri_nufft_prepare_normal_fm (auto L', wall clock), then normal_ms (qmri_normal_dev) against pair_ms (qmri_forward_dev +
            qmri_adjoint_dev), one slice, with the map, each the median wall clock of 20 calls ended by qmri_synchronize; and the same two plus qmri_nufft_prepare_normal's setup_ms without a map
  toeplitz  one PnP-ADMM iteration (qmri_pnp_admm, one unit coil, wall clock per iteration over 3) with the field-aware CG x-update
  lsqr      the same with the LSQR x-update

    python tools/offres_times.py --normal
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
N, S_INT, T, s, WIDTH, READOUT_S = 224, 800, 200, 10, 12, 5e-3
SEGMENTS = (0, 1, 4, 8)          # 0: no map
WARMUP, REPS = 3, 20
STEP_LIMIT_S = 240


def median_ms(fn):
    import torch
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return round(float(np.median(times)), 4)


def step(L):
    import torch
    from qmri_pnp_recon_poc_amd import engine as E
    V = np.linalg.qr(np.random.default_rng(0).standard_normal((T, s)))[0]
    fp, om = E.build_spiral_traj(N, S_INT, T)
    e = E.Engine(0)
    e.set_trajectory(N, N, V, fp, om, width=WIDTH)
    out = {"m": int(fp[-1])}
    if L:
        a, b = np.meshgrid((np.arange(N) - N / 2) / N, (np.arange(N) - N / 2) / N, indexing="ij")
        f = np.full((N, N), 80.0) if L == 1 else 100.0 * (np.sin(2 * np.pi * a) * np.cos(np.pi * b) + 0.6 * b + 0.2)
        t0 = time.perf_counter()
        info = e.set_field_map(f, E.spiral_readout_times(S_INT, T, READOUT_S), nseg=L)
        out.update({"attach_ms": round(1e3 * (time.perf_counter() - t0), 3), "nseg": info["nseg"], "fit_max": info["fit_max"]})
    e.set_stream(torch.cuda.current_stream().cuda_stream)             # the events below bracket the library's launches
    rng = np.random.default_rng(1)
    x = torch.from_numpy(rng.standard_normal(N * N * s) + 1j * rng.standard_normal(N * N * s)).cuda()
    y = torch.zeros(e.m, dtype=torch.complex128, device="cuda")
    torch.cuda.synchronize()
    vp = lambda t: C.c_void_p(t.data_ptr())
    out["forward_ms"] = median_ms(lambda: e._check(e.L.qmri_forward_dev(e.h, vp(x), vp(y), 1)))
    out["adjoint_ms"] = median_ms(lambda: e._check(e.L.qmri_adjoint_dev(e.h, vp(y), vp(x), 1)))
    e.set_stream(None)
    e.close()
    return out


NORMAL_MAP_L, NORMAL_STEPS, ADMM_ITERS = 6, ("apply", "toeplitz", "lsqr"), 3


def wall_median_ms(fn, sync):
    """median wall clock of fn() followed by sync() (the library's own stream), REPS calls after WARMUP"""
    for _ in range(WARMUP):
        fn()
    sync()
    times = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        sync()
        times.append(1e3 * (time.perf_counter() - t0))
    return round(float(np.median(times)), 4)


def normal_step(name):
    import torch
    from qmri_pnp_recon_poc_amd import engine as E, synth
    dic = synth.make_dictionary(T=T, n_t1=24, n_t2=16, s=s)
    X0 = synth.synthesize_tsmi(synth.make_phantom_qmaps(N, seed=0), dic)
    fp, om = E.build_spiral_traj(N, S_INT, T)
    a, b = np.meshgrid((np.arange(N) - N / 2) / N, (np.arange(N) - N / 2) / N, indexing="ij")
    f = 100.0 * (np.sin(2 * np.pi * a) * np.cos(np.pi * b) + 0.6 * b + 0.2)
    e = E.Engine(0)
    e.set_trajectory(N, N, dic["V"], fp, om, width=WIDTH)
    out = {}
    if name == "apply":
        x = torch.from_numpy(np.asfortranarray(X0).ravel(order="F").astype(np.complex128)).cuda()
        y = torch.zeros(e.m, dtype=torch.complex128, device="cuda")
        xn, xa = torch.zeros_like(x), torch.zeros_like(x)
        vp = lambda t: C.c_void_p(t.data_ptr())

        def normal():
            e._check(e.L.qmri_normal_dev(e.h, vp(x), vp(xn), 1))

        def pair():
            e._check(e.L.qmri_forward_dev(e.h, vp(x), vp(y), 1)); e._check(e.L.qmri_adjoint_dev(e.h, vp(y), vp(xa), 1))
        for tag in ("plain", "field"):
            r = {}
            t0 = time.perf_counter()
            if tag == "field":
                e.set_field_map(f, E.spiral_readout_times(S_INT, T, READOUT_S), nseg=NORMAL_MAP_L)
                t0 = time.perf_counter()
                info = e.prepare_normal_field()
                r.update({"map_nseg": NORMAL_MAP_L, "nseg": info["nseg"], "fit_max": info["fit_max"], "khat_bytes": info["khat_bytes"]})
            else:
                e.prepare_normal()
            e.synchronize()
            r["setup_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
            r["normal_ms"], r["pair_ms"] = wall_median_ms(normal, e.synchronize), wall_median_ms(pair, e.synchronize)
            r["normal_vs_pair_rel_err"] = float((torch.linalg.norm(xn - xa) / torch.linalg.norm(xa)).item())
            out[tag] = r
    else:
        e.set_field_map(f, E.spiral_readout_times(S_INT, T, READOUT_S), nseg=NORMAL_MAP_L)
        if name == "toeplitz":
            out["nseg"] = e.prepare_normal_field()["nseg"]
        e.set_denoiser(synth.structured_weights(in_nc=s, out_nc=s, seed=3, eps=0.05), N, N)
        yv = e.forward(X0)
        e.pnp_admm(yv, iters=1, solver=name)
        t0 = time.perf_counter()
        _, _, li = e.pnp_admm(yv, iters=ADMM_ITERS, solver=name)
        out.update({"admm_ms_per_iter": round(1e3 * (time.perf_counter() - t0) / ADMM_ITERS, 2), "solver_iters": [int(v) for v in li]})
    e.close()
    return out


def normal_main():
    out = {"N": N, "s": s, "S": S_INT, "T": T, "width": WIDTH, "readout_s": READOUT_S, "warmup": WARMUP, "reps": REPS}
    for name in NORMAL_STEPS:                                          # each under its own time limit; nothing is started after a failure
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--normal-step", name]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(json.dumps({"failed_step": name, "returncode": r.returncode, **out}))
            return 1
        out[name] = json.loads(r.stdout.strip().splitlines()[-1])
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    json.dump(out, open(os.path.join(ROOT, "profiles", "offres_normal_times.json"), "w"), indent=1)
    print(json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, choices=SEGMENTS)
    ap.add_argument("--normal", action="store_true")
    ap.add_argument("--normal-step", choices=NORMAL_STEPS)
    a = ap.parse_args()
    if a.normal_step is not None:
        print(json.dumps(normal_step(a.normal_step)))
        return 0
    if a.normal:
        return normal_main()
    if a.segments is not None:
        print(json.dumps(step(a.segments)))
        return 0
    out = {"N": N, "s": s, "S": S_INT, "T": T, "width": WIDTH, "readout_s": READOUT_S, "warmup": WARMUP, "reps": REPS}
    for L in SEGMENTS:                                                 # each under its own time limit; nothing is started after a failure
        cmd = ["timeout", "-k", "10", str(STEP_LIMIT_S), sys.executable, os.path.abspath(__file__), "--segments", str(L)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(json.dumps({"failed_step": f"L={L}", "returncode": r.returncode, **out}))
            return 1
        out["no_map" if L == 0 else f"L{L}"] = json.loads(r.stdout.strip().splitlines()[-1])
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    json.dump(out, open(os.path.join(ROOT, "profiles", "offres_times.json"), "w"), indent=1)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
