"""tests/sampling_reference.py (the extended-precision checker of the device's posterior draws) against what the unmodified
reference recorded in tests/golden/ref_sampling.npz.  No GPU: this is what makes tests/test_gpu_sampling_edges.py trustworthy."""
import os

import numpy as np

import sampling_reference as sr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_sampling.npz")


def _cases():
    f = np.load(GOLDEN)
    out = []
    for i in range(int(f["num_cases"])):
        c = {k[len("c%d_" % i):]: f[k] for k in f.files if k.startswith("c%d_" % i)}
        c["index"], c["regular"] = i, i < int(f["num_regular"])
        out.append(c)
    return out


def _close(got, want, tol):
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    assert err.max() <= tol, err.max()
    return float(err.max())


def test_extended_arithmetic_is_extended():
    assert np.finfo(sr.LD).eps < 1e-18
    assert sr.LD(1) + sr.LD(2) ** -60 != sr.LD(1)


def test_reference_module_reproduces_the_regular_fixture_cases():
    """values to 1e-12 max(1, |want|) (the fixture is the reference's double arithmetic), argmin and rc exactly, for every case
    without derivative observations; both covariance types and every fixture shape must be among them."""
    seen, worst = set(), 0.0
    for c in _cases():
        if not c["regular"] or len(c["derivs"]):
            continue
        values, argmin, rc = sr.sample(int(c["cov_type"]), c["hyper"], c["X"], c["y"], c["noise"], c["pts"], c["normals"])
        assert rc == int(c["rc"]) == 0
        worst = max(worst, _close(values, c["values"], 1e-12))
        np.testing.assert_array_equal(argmin, c["argmin"])
        seen.add((int(c["cov_type"]), c["pts"].shape[0]))
    print("extended reference vs fixture, regular cases: worst %.2e" % worst)
    assert seen == {(t, n) for t in (0, 1) for n in (1, 7, 64, 65, 200)}


def test_reference_module_reproduces_the_singular_fixture_cases():
    """The duplicate-candidate cases: the failing pivot is found where the reference found it, the early stop leaves what the
    reference multiplied with; from the posterior the module forms itself and from the covariance the fixture recorded."""
    n = 0
    for c in _cases():
        if c["regular"]:
            continue
        assert len(c["derivs"]) == 0
        values, argmin, rc = sr.sample(int(c["cov_type"]), c["hyper"], c["X"], c["y"], c["noise"], c["pts"], c["normals"])
        assert rc == int(c["rc"]) > 0
        _close(values, c["values"], 1e-12)
        np.testing.assert_array_equal(argmin, c["argmin"])
        mu = sr.Posterior(int(c["cov_type"]), c["hyper"], c["X"], c["y"], c["noise"]).mu_var(c["pts"])[0]
        v2, a2, rc2, _ = sr.draws_from(mu, c["var"], c["normals"])
        assert rc2 == rc
        _close(v2, c["values"], 1e-12)
        # the other failure mode: the failing column zeroed, the factor still reproduces the covariance it was given
        rc3, F = sr.outer_product_cholesky(c["var"].astype(sr.LD), stop_at_failure=False)
        assert rc3 == rc and not F[:, rc - 1].any()
        assert np.abs((F @ F.T).astype(np.float64) - c["var"]).max() <= 1e-16 + 1e-12 * np.abs(c["var"]).max()
        n += 1
    assert n == 2


def test_outer_product_cholesky_in_double_is_the_plain_algorithm():
    rng = np.random.default_rng(0)
    a = rng.normal(size=(40, 40))
    a = a @ a.T + 40 * np.eye(40)
    rc, F = sr.outer_product_cholesky(a)
    assert rc == 0 and F.dtype == np.float64
    assert np.abs(F - np.linalg.cholesky(a)).max() <= 1e-13
    assert np.abs(sr.cholesky_spd(a).astype(np.float64) - np.linalg.cholesky(a)).max() <= 1e-13
    b = rng.normal(size=(40, 3))
    assert np.abs(sr.forward_solve(F.astype(sr.LD), b).astype(np.float64) - np.linalg.solve(F, b)).max() <= 1e-13


def test_reference_argmin_rule():
    assert sr.reference_argmin([1.0, 2.0, 3.0]) == -1
    assert sr.reference_argmin([1.0, 0.5, 0.5]) == 1
    assert sr.reference_argmin([0.5, 0.5, 0.5]) == -1
    assert sr.reference_argmin([2.0, 3.0, 1.0, 1.0]) == 2
    assert sr.reference_argmin([7.0]) == -1


def test_fixture_has_no_near_ties():
    """tests/test_gpu_sampling.py::test_sample_points_match_reference exempts a draw from the argmin check when its two smallest
    reference values are within 1e-8 sqrt(alpha): the committed fixture has no such draw, so that test may demand all of them."""
    exempt = total = 0
    for c in _cases():
        if not c["regular"]:
            continue
        for v in c["values"]:
            two = np.sort(v)[:2]
            total += 1
            exempt += int(len(two) == 2 and two[1] - two[0] <= 1e-8 * np.sqrt(float(c["hyper"][0])))
    assert total > 0 and exempt == 0
