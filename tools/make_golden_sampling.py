"""Write tests/golden/ref_sampling.npz: joint posterior draws (SamplePointsFromGP, gpp_math.cpp:1800-1848) composed from the
unmodified reference behind oracle/ref.py -- its GaussianProcess' mean and variance (the function-value rows when derivatives are
observed), its ComputeCholeskyFactorL (partial factor and return code when a pivot fails) -- then y = mu + tril(L) z and the
reference's argmin rule (best = y[0], index -1, strict <).

    python tools/make_golden_sampling.py      # needs oracle/_ref (make -C oracle ref)

Case keys: c<i>_<field>.  Fields: X, y, noise, hyper, derivs, cov_type, pts, normals, values, argmin, rc; the singular cases
(alpha = 1e-6, an exact duplicate candidate) also store var, the C x C posterior covariance they factor.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ref_sampling.npz")


def ref_argmin(y):
    best, idx = y[0], -1
    for i in range(len(y)):
        if y[i] < best:
            best, idx = y[i], i
    return idx


def compose(gp, g, pts, normals):
    C = pts.shape[0]
    mu = gp.mean(pts)
    m = C * (1 + g)
    var = gp.var(pts).reshape(m, m).T  # [row, col]
    rows = np.arange(C) * (1 + g)
    var = var[np.ix_(rows, rows)].copy()
    rc, fac = ref.cholesky(var)
    L = np.tril(fac)
    values = np.array([mu + L @ z for z in normals])
    return var, rc, values, np.array([ref_argmin(v) for v in values], dtype=np.int32)


def main():
    rng = np.random.default_rng(20261016)
    out = {}
    i = 0
    d = 3
    draws = (1, 3, 64)
    for g in (0, 2):
        for cov_type in (0, 1):
            for ci, C in enumerate((1, 7, 64, 65, 200)):
                D = draws[(ci + g + cov_type) % 3]
                if C == 200 and D == 64:
                    D = 3
                n = 30
                X = rng.uniform(0, 1, size=(n, d))
                derivs = list(range(g))
                y = rng.normal(size=(n, 1 + g))
                noise = np.full(1 + g, 1e-2)
                hyper = np.array([1.3, 0.15, 0.2, 0.12])
                gp = ref.RefGP(cov_type, hyper[0], hyper[1:], X, y.ravel(), noise, derivs)
                pts = rng.uniform(0, 1, size=(C, d))
                normals = rng.normal(size=(D, C))
                var, rc, values, argmin = compose(gp, g, pts, normals)
                assert rc == 0, (g, cov_type, C, rc)
                out.update({"c%d_%s" % (i, k): v for k, v in dict(
                    X=X, y=y, noise=noise, hyper=hyper, derivs=np.array(derivs, dtype=np.int32), cov_type=np.int32(cov_type),
                    pts=pts, normals=normals, values=values, argmin=argmin, rc=np.int32(rc)).items()})
                i += 1
    num_regular = i
    # singular: alpha = 1e-6, candidate `dup` repeats candidate `src` exactly (pivot residue ~1e-22, genuine pivots ~1e-8 and up)
    for C, src, dup in ((40, 5, 20), (100, 10, 80)):
        n = 25
        X = rng.uniform(0, 1, size=(n, d))
        y = rng.normal(size=(n, 1)) * 1e-3
        noise = np.array([1e-8])
        hyper = np.array([1e-6, 0.15, 0.2, 0.12])
        gp = ref.RefGP(1, hyper[0], hyper[1:], X, y.ravel(), noise, [])
        pts = rng.uniform(0, 1, size=(C, d))
        pts[dup] = pts[src]
        normals = rng.normal(size=(3, C))
        var, rc, values, argmin = compose(gp, 0, pts, normals)
        assert rc == dup + 1, rc
        out.update({"c%d_%s" % (i, k): v for k, v in dict(
            X=X, y=y, noise=noise, hyper=hyper, derivs=np.zeros(0, dtype=np.int32), cov_type=np.int32(1), pts=pts,
            normals=normals, values=values, argmin=argmin, rc=np.int32(rc), var=var).items()})
        i += 1
    out["num_regular"] = np.int32(num_regular)
    out["num_cases"] = np.int32(i)
    np.savez_compressed(OUT, **out)
    print("wrote %s: %d cases (%d singular), %d bytes" % (OUT, i, i - num_regular, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
