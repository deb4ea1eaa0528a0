"""numpy restatement of the density compensation of a trajectory operator (qmri_nufft_dcf) for the tests, fp64.

    w_i = 1;  g[k] = sum_j w_j psi(u_j1 - k1) psi(u_j2 - k2);  d_i = sum_k g[k] psi(u_i1 - k1) psi(u_i2 - k2);  w_i <- w_i / d_i;  dev = max |d_i - 1|

on the periodic 2N x 2M grid, all samples one set; then w <- kappa w, kappa = (T / 4) I_1^2 I_2^2, I_a = sum_k psi(k) over the window at zero offset.
psi is the operator's kernel exp(beta (sqrt(1 - (d / (w/2))^2) - 1)) on the window [k0, k0 + w), k0 = ceil(u - w/2) (nu_phi / nu_k0 of
csrc/nufft_device.h).  beta is the plan's: the library keeps it in one place, nu_beta() of csrc/nufft_plan.h, and plan_beta() reads it from
there -- it is not restated here."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plan_beta(width):
    """beta of the plan for a kernel of `width` points: the expression nu_beta() of nufft_plan.h returns (a multiple of the width)."""
    src = open(os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "csrc", "nufft_plan.h")).read()
    m = re.search(r"double\s+nu_beta\s*\(\s*int\s+w\s*\)\s*\{\s*return\s+([0-9.eE+-]+)\s*\*\s*w\s*;\s*\}", src)
    assert m, "nu_beta(int w) { return <factor> * w; } not found in nufft_plan.h"
    return float(m.group(1)) * width


def plan_width(width=0):
    """the width a plan uses for qmri_nufft_params.width (0: the default NU_WDEF of nufft_plan.h)."""
    if width:
        return int(width)
    src = open(os.path.join(ROOT, "qmri_pnp_recon_poc_amd", "csrc", "nufft_plan.h")).read()
    m = re.search(r"constexpr\s+int\s+NU_WDEF\s*=\s*(\d+)\s*;", src)
    assert m, "NU_WDEF not found in nufft_plan.h"
    return int(m.group(1))


def phi(d, hw, beta):
    t = 1.0 - (d / hw) ** 2
    return np.where(t >= 0.0, np.exp(beta * (np.sqrt(np.maximum(t, 0.0)) - 1.0)), 0.0)


def kernel_sum(width, beta):
    hw = 0.5 * width
    k0 = int(np.ceil(0.0 - hw))
    return float(np.sum(phi(0.0 - (k0 + np.arange(width)), hw, beta)))


def kappa(T, width, beta):
    I1, I2 = kernel_sum(width, beta), kernel_sum(width, beta)
    return 0.25 * T * I1 ** 2 * I2 ** 2


class Plan:
    """windows and kernel values of every sample: idx [m, w*w] flat indices into the 2N x 2M grid, val [m, w*w] psi1 psi2."""

    def __init__(self, N, M, omega, width=0):
        self.width = plan_width(width)
        self.beta = plan_beta(self.width)
        w, hw = self.width, 0.5 * self.width
        om = np.asarray(omega, np.float64)
        u1, u2 = om[:, 0] * N / np.pi, om[:, 1] * M / np.pi
        k1 = np.ceil(u1 - hw).astype(np.int64)[:, None] + np.arange(w)[None, :]          # m x w
        k2 = np.ceil(u2 - hw).astype(np.int64)[:, None] + np.arange(w)[None, :]
        p1, p2 = phi(u1[:, None] - k1, hw, self.beta), phi(u2[:, None] - k2, hw, self.beta)
        self.idx = ((k1 % (2 * N))[:, :, None] * (2 * M) + (k2 % (2 * M))[:, None, :]).reshape(om.shape[0], w * w)
        self.val = (p1[:, :, None] * p2[:, None, :]).reshape(om.shape[0], w * w)
        self.G = 4 * N * M


def iterate(plan, niter=20, tol=0.0):
    """-> (unscaled weights, iterations run, dev of the last one, dev of every iteration run)."""
    w = np.ones(plan.idx.shape[0])
    devs = []
    for _ in range(niter):
        g = np.bincount(plan.idx.ravel(), weights=(w[:, None] * plan.val).ravel(), minlength=plan.G)
        d = np.sum(g[plan.idx] * plan.val, axis=1)
        w = w / d
        devs.append(float(np.max(np.abs(d - 1.0))))
        if tol > 0.0 and devs[-1] <= tol:
            break
    return w, len(devs), devs[-1], devs


def weights(N, M, T, omega, width=0, niter=20, tol=0.0):
    """-> (w [m] as qmri_nufft_dcf returns them, info dict(iters, dev))."""
    plan = Plan(N, M, omega, width)
    w, it, dev, _ = iterate(plan, niter or 20, tol)
    return kappa(T, plan.width, plan.beta) * w, {"iters": it, "dev": dev}


def phantom(N, M=None):
    """a smooth phantom with a box in it, real, N x M."""
    M = M or N
    a, b = np.meshgrid((np.arange(N) - N / 2) / N, (np.arange(M) - M / 2) / M, indexing="ij")
    x = np.exp(-(a ** 2 + b ** 2) / (2 * 0.18 ** 2))
    x[(np.abs(a - 0.05) < 0.12) & (np.abs(b + 0.08) < 0.09)] += 0.7
    return x


def best_fit(a, x):
    """alpha minimising ||alpha a - x||, and the relative error at it."""
    al = np.vdot(a, x) / np.vdot(a, a)
    return al, float(np.linalg.norm(al * a - x) / np.linalg.norm(x))
