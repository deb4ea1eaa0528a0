"""numpy restatement of the EPG fingerprint derivatives and their Cramer-Rao bound (include/qmri.h qmri_dict_simulate_grad):
what the GPU tests compare against -- never the device's own output.  Forward-mode differentiation of tests/epg_ref.py's recursion: next to
F+, F-, Z every parameter (T1, T2 and, with nparams = 3, b1) carries a tangent of the same shape, real and zero at the start.  The primal lines are
those of epg_ref.epg_fisp, operation for operation, so F has its bits."""
import numpy as np

import epg_ref as R

SINGULAR, BAD_ATOM = 1, 2
PIVOT_MIN = 1e-10


def epg_fisp_grad(alpha, tr, te, t1, t2, b1=None, nstates=32, inversion=True, ti=0.0, inv_eff=1.0, nparams=2, dtype=np.float64, exp=None):
    """(F [K, T], dF [P, K, T]) in `dtype` (np.float64 or np.longdouble); dF[0] = dF/dT1, dF[1] = dF/dT2, dF[2] = dF/db1 (nparams = 3).  The other
    arguments are epg_ref.epg_fisp's; exp replaces np.exp everywhere (the derivative of an exponential is formed from the replaced value)."""
    ex = np.exp if exp is None else exp
    P = int(nparams)
    alpha = np.asarray(alpha, dtype=dtype).ravel()
    T, S = alpha.size, int(nstates)
    tr = np.broadcast_to(np.asarray(tr, dtype=dtype), (T,))
    te = np.broadcast_to(np.asarray(te, dtype=dtype), (T,))
    t1, t2 = np.asarray(t1, dtype=dtype).ravel(), np.asarray(t2, dtype=dtype).ravel()
    K = t1.size
    b1 = np.ones(K, dtype=dtype) if b1 is None else np.asarray(b1, dtype=dtype).ravel()
    one, half = dtype(1), dtype(0.5)
    fp, fm, z = np.zeros((K, S), dtype), np.zeros((K, S), dtype), np.zeros((K, S), dtype)
    dfp, dfm, dz = (np.zeros((P, K, S), dtype) for _ in range(3))
    z[:, 0] = one
    if inversion:
        e = ex(-dtype(ti) / t1)
        de = e * (dtype(ti) / (t1 * t1))
        z[:, 0] = (-dtype(inv_eff) * z[:, 0]) * e + (one - e)
        dz[0, :, 0] = (-dtype(inv_eff)) * de - de
    F, dF = np.empty((K, T), dtype), np.empty((P, K, T), dtype)
    for t in range(T):
        a = alpha[t] * b1
        c, s = np.cos(a)[:, None], np.sin(a)[:, None]
        c2, s2 = (one + c) * half, (one - c) * half
        p, m, zz = fp, fm, z
        fp, fm, z = c2 * p - s2 * m + s * zz, -s2 * p + c2 * m + s * zz, -half * s * (p + m) + c * zz
        dfp, dfm, dz = c2 * dfp - s2 * dfm + s * dz, -s2 * dfp + c2 * dfm + s * dz, -half * s * (dfp + dfm) + c * dz
        if P == 3:
            xy = alpha[t] * (-(half * s) * (p + m) + c * zz)
            dfp[2] += xy
            dfm[2] += xy
            dz[2] += alpha[t] * (-(half * c) * (p + m) - s * zz)
        for step, dt in enumerate((te[t], tr[t] - te[t])):
            e1, e2 = ex(-dt / t1), ex(-dt / t2)
            de1, de2 = e1 * (dt / (t1 * t1)), e2 * (dt / (t2 * t2))
            dfp, dfm, dz = dfp * e2[:, None], dfm * e2[:, None], dz * e1[:, None]
            dfp[1] += de2[:, None] * fp
            dfm[1] += de2[:, None] * fm
            dz[0] += de1[:, None] * z
            dz[0, :, 0] -= de1
            fp, fm, z = fp * e2[:, None], fm * e2[:, None], z * e1[:, None]
            z[:, 0] += one - e1
            if step == 0:
                F[:, t] = fp[:, 0]
                dF[:, :, t] = dfp[:, :, 0]
        fp, fm = R.shift(fp, fm)
        dfp, dfm = R.shift(dfp, dfm)
    return F, dF


def jacobian(F, dF):
    """J [K, T, 1 + P]: the fingerprint, then its derivatives."""
    return np.concatenate([F[None], dF], axis=0).transpose(1, 2, 0)


def crb(J, V=None, dtype=np.float64):
    """(crb [K, 1 + P], flags [K] int32, pivots [K, 1 + P]) of J [K, T, 1 + P], projected on the real subspace V [T, s] when one is given.  Every
    sum runs in ascending row order from 0.  G = J^T J, d = sqrt(diag G), Gn = G / (d d^T), Cholesky of Gn; an atom whose G has a diagonal entry
    that is non-finite or <= 0, or a pivot (the number under the square root) that is not > 1e-10, is SINGULAR: flag 1, every bound +inf.
    Otherwise crb[k, q] = [Gn^-1]_qq / d_q^2, entry 0 the proton density's.  pivots: as far as they were computed (NaN afterwards)."""
    J = np.asarray(J, dtype=dtype)
    K, n = J.shape[0], J.shape[2]
    if V is not None:
        V = np.asarray(V, dtype=dtype)
        Pj = np.zeros((K, V.shape[1], n), dtype)
        for t in range(J.shape[1]):
            Pj = Pj + V[t][None, :, None] * J[:, t][:, None, :]
        J = Pj
    G = np.zeros((K, n, n), dtype)
    for t in range(J.shape[1]):
        G = G + J[:, t][:, :, None] * J[:, t][:, None, :]
    diag = np.stack([G[:, a, a] for a in range(n)], axis=1)
    sing = ~np.all(np.isfinite(diag) & (diag > 0), axis=1)
    with np.errstate(all="ignore"):
        d = np.sqrt(diag)
        Gn = G / (d[:, :, None] * d[:, None, :])
        L = np.zeros((K, n, n), dtype)
        piv = np.full((K, n), np.nan, dtype)
        for j in range(n):
            pj = Gn[:, j, j].copy()
            for k in range(j):
                pj = pj - L[:, j, k] * L[:, j, k]
            piv[:, j] = np.where(sing, np.nan, pj)
            sing = sing | ~(pj > dtype(PIVOT_MIN)) | ~np.isfinite(pj)
            L[:, j, j] = np.sqrt(pj)
            for i in range(j + 1, n):
                v = Gn[:, i, j].copy()
                for k in range(j):
                    v = v - L[:, i, k] * L[:, j, k]
                L[:, i, j] = v / L[:, j, j]
        Li = np.zeros((K, n, n), dtype)                       # L^-1 by forward substitution, column by column
        for q in range(n):
            Li[:, q, q] = dtype(1) / L[:, q, q]
            for i in range(q + 1, n):
                v = np.zeros(K, dtype)
                for k in range(q, i):
                    v = v - L[:, i, k] * Li[:, k, q]
                Li[:, i, q] = v / L[:, i, i]
        out = np.empty((K, n), dtype)
        for q in range(n):
            v = np.zeros(K, dtype)
            for i in range(q, n):
                v = v + Li[:, i, q] * Li[:, i, q]
            out[:, q] = v / (d[:, q] * d[:, q])
    out[sing] = np.inf
    return out, np.where(sing, SINGULAR, 0).astype(np.int32), piv


def uncertainty_gather(crb_k, flags, dm, pd, sigma):
    """(std [N, M, P], std_pd [N, M]): std = sigma sqrt(crb[dm - 1, 1:]) / |pd|, std_pd = sigma sqrt(crb[dm - 1, 0]); NaN where dm = 0, pd = 0 or
    the atom is flagged."""
    dm, pd = np.asarray(dm), np.asarray(pd)
    k = np.maximum(dm.astype(np.int64) - 1, 0)
    ok = (dm > 0) & (pd != 0) & (np.asarray(flags)[k] == 0)
    c = np.asarray(crb_k, np.float64)[k]
    with np.errstate(all="ignore"):
        std = float(sigma) * np.sqrt(c[..., 1:]) / np.abs(pd)[..., None]
        std_pd = float(sigma) * np.sqrt(c[..., 0])
    return np.where(ok[..., None], std, np.nan), np.where(ok, std_pd, np.nan)


# The GPU fixtures (names of epg_ref.CASES; each runs with nparams = 2 and 3) and the subspace cases (fixture, s).
GPU_CASES = ["s1", "s2", "s16", "s17", "s32", "s33", "s64", "s65", "s128", "s129", "s256", "k1", "timing", "noinv", "inveff", "b1", "t1024"]
V_CASES = [("s32", 5), ("s32", 10), ("s32", 16), ("b1", 5), ("b1", 10)]
T_CASES = ["s32@15", "s32@16", "s32@17"]                     # one frame short of a frame block of the kernel, a whole one, one more

# (name, P) -> (fp64 against longdouble, every exponential one ulp away), of max_kt |dF[q] - dF'[q]| / max_kt |dF[q]|, the largest over q: the
# figures tests/test_epg_grad_host.py measures on the restatement, rounded up with a factor 2 of room and asserted there.
SENS_D = {
    ('s1', 2): (4e-15, 1.4e-14), ('s1', 3): (5.9e-15, 2e-14), ('s2', 2): (4.7e-15, 2.1e-14), ('s2', 3): (6.4e-15, 2.3e-14),
    ('s16', 2): (5e-15, 2.2e-14), ('s16', 3): (5e-15, 2.4e-14), ('s17', 2): (5e-15, 2.2e-14), ('s17', 3): (5.2e-15, 2.5e-14),
    ('s32', 2): (5e-15, 2.2e-14), ('s32', 3): (5e-15, 2.5e-14), ('s33', 2): (5e-15, 2.2e-14), ('s33', 3): (5e-15, 2.5e-14),
    ('s64', 2): (5e-15, 2.2e-14), ('s64', 3): (5e-15, 2.5e-14), ('s65', 2): (5e-15, 2.2e-14), ('s65', 3): (5e-15, 2.5e-14),
    ('s128', 2): (5e-15, 2.2e-14), ('s128', 3): (5e-15, 2.5e-14), ('s129', 2): (5e-15, 2.2e-14), ('s129', 3): (5e-15, 2.5e-14),
    ('s256', 2): (5e-15, 2.2e-14), ('s256', 3): (5e-15, 2.5e-14), ('k1', 2): (3.6e-17, 1.4e-15), ('k1', 3): (1.4e-16, 1.4e-15),
    ('timing', 2): (1.9e-15, 1.8e-14), ('timing', 3): (2.8e-15, 2.6e-14), ('noinv', 2): (2.1e-15, 5.5e-15), ('noinv', 3): (5.1e-15, 1.7e-14),
    ('inveff', 2): (5.6e-15, 2.1e-14), ('inveff', 3): (5.6e-15, 2.4e-14), ('b1', 2): (5.9e-15, 2.1e-14), ('b1', 3): (5.9e-15, 2.4e-14),
    ('t1024', 2): (7.1e-15, 2.7e-14), ('t1024', 3): (9.3e-15, 4.7e-14),
    ('s32@15', 2): (3.9e-15, 1.5e-14), ('s32@15', 3): (3.9e-15, 1.5e-14), ('s32@16', 2): (3.9e-15, 1.5e-14), ('s32@16', 3): (3.9e-15, 1.5e-14),
    ('s32@17', 2): (3.9e-15, 1.5e-14), ('s32@17', 3): (3.9e-15, 1.5e-14),
}
# (name, P, s) -> the same two figures of max |crb - crb'| / crb over the regular atoms and all 1 + P entries (s = 0: uncompressed).  Fixtures whose
# atoms are all SINGULAR (s1, k1) have no entry.
SENS_CRB = {
    ('s2', 2, 0): (4.3e-14, 1.3e-13), ('s2', 3, 0): (5e-14, 3.1e-13), ('s16', 2, 0): (2.8e-14, 7e-14), ('s16', 3, 0): (1.5e-13, 2.3e-13),
    ('s17', 2, 0): (4.3e-14, 7.3e-14), ('s17', 3, 0): (9.1e-14, 2.2e-13), ('s32', 2, 0): (3e-14, 8.3e-14), ('s32', 2, 5): (2.2e-14, 7.1e-14),
    ('s32', 2, 10): (2.6e-14, 7.2e-14), ('s32', 2, 16): (2.6e-14, 7.2e-14), ('s32', 3, 0): (1.2e-13, 2.6e-13), ('s32', 3, 5): (8.8e-14, 2.4e-13),
    ('s32', 3, 10): (1.1e-13, 1.9e-13), ('s32', 3, 16): (1.4e-13, 2e-13), ('s33', 2, 0): (3e-14, 8.3e-14), ('s33', 3, 0): (1.2e-13, 2.6e-13),
    ('s64', 2, 0): (3e-14, 8.3e-14), ('s64', 3, 0): (1.2e-13, 2.6e-13), ('s65', 2, 0): (3e-14, 8.3e-14), ('s65', 3, 0): (1.2e-13, 2.6e-13),
    ('s128', 2, 0): (3e-14, 8.3e-14), ('s128', 3, 0): (1.2e-13, 2.6e-13), ('s129', 2, 0): (3e-14, 8.3e-14), ('s129', 3, 0): (1.2e-13, 2.6e-13),
    ('s256', 2, 0): (3e-14, 8.3e-14), ('s256', 3, 0): (1.2e-13, 2.6e-13), ('timing', 2, 0): (4.1e-14, 7.8e-14), ('timing', 3, 0): (7.7e-14, 3.5e-13),
    ('noinv', 2, 0): (9.9e-14, 1.1e-13), ('noinv', 3, 0): (5.3e-13, 3.8e-12), ('inveff', 2, 0): (3e-14, 7.7e-14),
    ('inveff', 3, 0): (1.7e-13, 2.8e-13), ('b1', 2, 0): (2.6e-14, 7.3e-14), ('b1', 2, 5): (2.7e-14, 7e-14), ('b1', 2, 10): (2.2e-14, 6.7e-14),
    ('b1', 3, 0): (1.1e-13, 2.8e-13), ('b1', 3, 5): (3.6e-12, 4.2e-12), ('b1', 3, 10): (3.8e-14, 1.5e-13), ('t1024', 2, 0): (8.4e-14, 3.5e-13),
    ('t1024', 3, 0): (5.4e-13, 3.5e-13),
    ('s32@15', 2, 0): (3.8e-12, 5.4e-12), ('s32@15', 3, 0): (1.7e-11, 1.9e-11), ('s32@16', 2, 0): (3.7e-12, 3.2e-12), ('s32@16', 3, 0): (2.8e-11, 3.5e-11),
    ('s32@17', 2, 0): (1.2e-12, 1.7e-12), ('s32@17', 3, 0): (2e-11, 1.7e-11),
}


def rtol_d(name, P):
    """Tolerance of the GPU tests on dF[q], relative to max |dF[q]| of the fixture: 16 x the larger sensitivity figure (epg_ref.atol's rationale:
    room for a 2-ulp device exp / sincos and for fused multiply-adds, which numpy does not form)."""
    return 16.0 * max(SENS_D[(name, P)])


def rtol_crb(name, P, s=0):
    """Relative tolerance of the GPU tests on every finite crb entry."""
    return 16.0 * max(SENS_CRB[(name, P, s)])


_refs = {}


def case_inputs(name):
    """epg_ref.case_inputs, and "fixture@T": the first T frames of that fixture (the frame-block boundary cases)."""
    if "@" not in name:
        return R.case_inputs(name)
    base, T = name.split("@")
    inp = R.case_inputs(base)
    return dict(inp, alpha=inp["alpha"][:int(T)], tr=inp["tr"][:int(T)], te=inp["te"][:int(T)])


def case_ref(name, P):
    """dict(F, dF, J) in float64 of a fixture, computed once and left unchanged."""
    if (name, P) not in _refs:
        F, dF = epg_fisp_grad(**case_inputs(name), nparams=P)
        r = {"F": F, "dF": dF, "J": jacobian(F, dF)}
        for v in r.values():
            v.setflags(write=False)
        _refs[(name, P)] = r
    return _refs[(name, P)]


def case_V(name, s):
    """V [T, s] of dict_svd_ref.dict_compress_ref on the fixture's own fingerprints, computed once."""
    import dict_svd_ref as DR
    if ("V", name, s) not in _refs:
        V = np.ascontiguousarray(DR.dict_compress_ref(R.case_ref(name), s=s)["V"])
        V.setflags(write=False)
        _refs[("V", name, s)] = V
    return _refs[("V", name, s)]


def case_crb(name, P, s=0):
    """(crb, flags, pivots) in float64 of a fixture, computed once."""
    if ("crb", name, P, s) not in _refs:
        _refs[("crb", name, P, s)] = crb(case_ref(name, P)["J"], case_V(name, s) if s else None)
    return _refs[("crb", name, P, s)]
