"""ADMM iterations / s with real and complex TSMIs: 224 x 224, s = 10, the full-size UNetRes (64, 128, 256, 512; nb = 4)
of random structured weights (10 -> 10 in real mode, 20 -> 20 in complex mode), one slice and slice batches of 15 / 30 (qmri_pnp_admm_dev).

    python tools/complex_times.py [--iters 20] [--reps 3] [--out profiles/complex_times.json]

Each row also records the health of the path that ran (denoiser scheme, resident-tile launch armed) and, from a separate profiled run (profile
level 2, not timed), the convolution launch units per ADMM iteration: a resident-tile launch counts once with every layer riding in it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from qmri_pnp_recon_poc_amd import engine as E, synth  # noqa: E402


def run(batch, domain, iters, reps, dic, fp, k, ys):
    s = 10
    P = 2 * s if domain == "complex" else s
    w = synth.structured_weights(in_nc=P, out_nc=P, seed=2, eps=0.02)
    e = E.Engine(0)
    e.set_operator(224, 224, dic["V"], fp, k, max_batch=batch)
    e.set_denoiser(w, 224, 224, in_nc=P, out_nc=P, max_batch=batch)
    Y = np.stack([ys[b % len(ys)] for b in range(batch)])
    e.pnp_admm_batch(Y, slices_per_launch=batch, iters=2, tsmi_domain=domain)                   # warm-up (set-up, scheme probe)
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        e.pnp_admm_batch(Y, slices_per_launch=batch, iters=iters, tsmi_domain=domain)
        best = min(best, time.perf_counter() - t0)
    h = e.health()
    e.profile_enable(2)
    e.profile_get(reset=True)
    e.pnp_admm_batch(Y, slices_per_launch=batch, iters=3, tsmi_domain=domain)
    p = e.profile_get(reset=True)
    e.profile_enable(0)
    e.close()
    return {"batch": batch, "domain": domain, "iters": iters, "best_s": best, "admm_it_per_s": iters / best,
            "slice_it_per_s": batch * iters / best, "denoiser_scheme": h["denoiser_scheme"],
            "resident_tile_launch_armed": h["resident_tile_launch_armed"],
            "conv_launch_units_per_iter": (p["n_conv3x3"] + p["n_conv2x2"]) / max(p["admm_iters"], 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="1,15,30")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dic = synth.make_dictionary(T=200, n_t1=32, n_t2=16, s=10)
    fp, k = E.build_spiral(224, 771, 200)
    e = E.Engine(0)
    e.set_operator(224, 224, dic["V"], fp, k)
    hh, ww = np.meshgrid(np.linspace(-1, 1, 224), np.linspace(-1, 1, 224), indexing="ij")
    ys = []
    for sd in range(3):
        X0 = synth.synthesize_tsmi(synth.make_phantom_qmaps(224, seed=sd), dic) * np.exp(1j * (1.2 * hh + 0.8 * ww * ww))[:, :, None]
        ys.append(synth.awgn_measured(e.forward(X0), 30.0, seed=sd))
    e.close()
    rows = []
    for b in [int(v) for v in a.batches.split(",")]:
        r = {d: run(b, d, a.iters, a.reps, dic, fp, k, ys) for d in ("real", "complex")}
        ratio = r["complex"]["admm_it_per_s"] / r["real"]["admm_it_per_s"]
        rows += [r["real"], r["complex"]]
        print(f"batch {b:3d}: real {r['real']['admm_it_per_s']:8.2f} it/s, complex {r['complex']['admm_it_per_s']:8.2f} it/s, "
              f"complex/real {ratio:.3f}; conv launch units per iteration real {r['real']['conv_launch_units_per_iter']:g}, "
              f"complex {r['complex']['conv_launch_units_per_iter']:g}", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
