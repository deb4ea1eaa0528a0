"""TEST INFRASTRUCTURE: the grouped dictionary match (include/qmri.h qmri_dict_match_grouped) restated on the CPU oracle.

The contract is stated in terms of the ungrouped match, so the reference is the ungrouped oracle: apply the assignment rule in numpy, call
oracle.dict_match once per group on that group's pixels with the group's rows of D / normD / lut, shift dm by the group's offset, scatter, and
write zeros for unmatched pixels.  Every comparison against it is np.array_equal."""
import numpy as np


def assign(group_val, sel):
    """1-based group of each value: the lowest g minimising |sel - group_val[g]| in float64 (np.argmin keeps the first minimum); 0 for a
    non-finite value."""
    gv = np.asarray(group_val, dtype=np.float64).ravel()
    b = np.asarray(sel, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(b.reshape(-1, 1) - gv[None, :])
    g = np.argmin(np.where(np.isnan(d), np.inf, d), axis=1).astype(np.int32) + 1
    g[~np.isfinite(b.ravel())] = 0
    return g.reshape(b.shape)


def match_grouped(O, X, sel, D, normD, lut, group_ptr, group_val, want_xfit=False):
    """O: the oracle module.  X [..., s] complex, sel [...].  Returns dict(qmap, pd, mt, dm, grp[, Xfit]) in the shapes Engine.dict_match gives."""
    X = np.asarray(X, dtype=np.complex128)
    lead, s = X.shape[:-1], X.shape[-1]
    Xf = X.reshape(-1, s)
    D, normD, lut = np.asarray(D, np.float32), np.asarray(normD, np.float32), np.asarray(lut, np.float32)
    gp = np.asarray(group_ptr, dtype=np.int64)
    grp = assign(group_val, np.asarray(sel, dtype=np.float64).reshape(-1))
    n, Q = Xf.shape[0], lut.shape[1]
    out = {"qmap": np.zeros((n, Q), np.float32), "pd": np.zeros(n, np.complex64), "mt": np.zeros(n, np.float32), "dm": np.zeros(n, np.int32), "grp": grp}
    if want_xfit:
        out["Xfit"] = np.zeros((n, s), np.complex64)
    for g in range(len(gp) - 1):
        idx = np.nonzero(grp == g + 1)[0]
        if idx.size == 0:
            continue
        a, b = int(gp[g]), int(gp[g + 1])
        r = O.dict_match(Xf[idx], D[a:b], normD[a:b], lut[a:b], want_xfit=want_xfit)
        out["qmap"][idx], out["pd"][idx], out["mt"][idx], out["dm"][idx] = r["qmap"], r["pd"], r["mt"], r["dm"] + a
        if want_xfit:
            out["Xfit"][idx] = r["Xfit"]
    return {k: v.reshape(lead + v.shape[1:]) for k, v in out.items()}


KEYS = ("dm", "grp", "mt", "pd", "qmap")


def same(a, b, keys=KEYS):
    """bit-for-bit on every named output; returns the names that differ (empty: equal)"""
    return [k for k in keys if not np.array_equal(np.asarray(a[k]), np.asarray(b[k]))]


def random_dictionary(K, s, seed, Q=2):
    """unit-norm random atoms, normD in [0.5, 1.5), lut = (index, random)"""
    rng = np.random.default_rng(seed)
    D = rng.standard_normal((K, s)).astype(np.float32)
    D /= np.linalg.norm(D, axis=1, keepdims=True).astype(np.float32)
    nd = (0.5 + rng.random(K)).astype(np.float32)
    lut = np.stack([np.arange(K, dtype=np.float32)] + [rng.random(K).astype(np.float32) for _ in range(Q - 1)], axis=1)
    return D, nd, lut
