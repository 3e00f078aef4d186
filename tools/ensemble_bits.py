"""The bits of the eight entry points of the ensemble one-point acquisitions (csrc/kg1_opt.hip, csrc/ei1.hip through
csrc/kg1_ascent.hip): moe_kg_discrete_mcmc, _multistart, _pending, _multistart_pending, _suggest and moe_ei_analytic_mcmc,
_multistart, _suggest.  One line per call: a label and the SHA-256 over the raw bytes of every array the call returned.  Two
builds compute the same thing exactly when their outputs are the same line for line:
   python tools/ensemble_bits.py > a.txt;  MOE_LIB_PATH=other/libmoe_hip.so python tools/ensemble_bits.py > b.txt;  diff a.txt b.txt

The cases are the test suite's smallest that reach every branch of the staging: tests/kg1_opt_cases.py (E = 1; E = 3; E = 3 with a
fidelity coordinate and members of unequal N and A), tests/ei1_reference.py's ensemble (g = 0) and tests/ei1_deriv_reference.py's
(g = 2) and the first member of each alone, each with p = 0 and p = 2 pending points, value only and with gradient, the ascent with
and without its path and without the ascent, a greedy batch of q = 3, ensemble-wide launches on and off.  Two refusals close the
list with code, message and payload: a pending point listed twice in a noise-free member, and a member listed twice.

The EI cases are built from tests/ei1_reference.py and tests/ei1_deriv_reference.py (make_ensemble()), the modules that
tests/test_gpu_ei1.py and tests/test_gpu_ei1_deriv.py take theirs from, with the starts and outer parameters of those tests'
_ascent_problem(): the helpers inside the test modules sit behind `import pytest` and the suite's conftest, which a tool does not
load, and tests/ei_cases.py holds the shapes of the Monte-Carlo q,p-EI (csrc/ei.hip), which these entry points do not run."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ei1_deriv_reference as dr  # noqa: E402
import ei1_reference as er  # noqa: E402
import kg1_opt_cases as kc  # noqa: E402
from cornell_moe_amd import _lib, api  # noqa: E402

Q = 3
RUN_KEYS = ("point", "value", "found", "start_values", "kept_index", "end_points", "end_values", "steps_taken", "path")


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def say(label, arrays):
    print("%-78s %s" % (label, digest(arrays)))
    sys.stdout.flush()


def run_arrays(res):
    return [np.asarray(res[k]) if res.get(k) is not None else None for k in RUN_KEYS]


def refusal(label, call):
    try:
        call()
        print("%-78s no refusal" % label)
    except api.OptimalLearningException as e:
        payload = [getattr(e, k) for k in ("num_rows", "leading_minor_index", "value", "truth", "tolerance", "min", "max") if hasattr(e, k)]
        print("%-78s %s %s | %s" % (label, type(e).__name__, payload, e))
    sys.stdout.flush()


def all_calls(tag, evaluate, multistart, suggest, pending_all):
    """evaluate(want_grad, pending), multistart(ascent, want_path, pending), suggest(ascent, pending): the three shapes of entry point"""
    for on in (1, 0):
        _lib.load().moe_set_ensemble_launches(on)
        for p in (0, 2):
            pending = pending_all[:p] if p else None
            head = "%s p=%d launches=%d" % (tag, p, on)
            say(head + " evaluate value", [evaluate(False, pending)])
            say(head + " evaluate value+grad", list(evaluate(True, pending)))
            say(head + " multistart no-ascent", run_arrays(multistart(False, False, pending)))
            say(head + " multistart", run_arrays(multistart(True, False, pending)))
            say(head + " multistart path", run_arrays(multistart(True, True, pending)))
            res = suggest(True, pending)
            say(head + " suggest q=%d" % Q, [res["points"], res["values"], res["found"]])
            res = suggest(False, pending)
            say(head + " suggest q=%d no-ascent" % Q, [res["points"], res["values"], res["found"]])
    _lib.load().moe_set_ensemble_launches(-1)


def kg_case(name):
    case = [c for c in kc.CASES if c.name == name][0]
    p = kc.make_problem(case)
    gps = [api.DeviceGP(p.hyper[e], p.X[e], p.y[e], p.noise[e], cov_type=case.cov[e]) for e in range(len(case.n))]
    pending = np.random.default_rng(402).uniform(0.05, 0.95, size=(2, case.d))
    kw = dict(num_fidelity=case.nf)
    all_calls(
        "kg %s" % name,
        lambda g, pend: api.kg_discrete_ensemble(gps, p.discrete, p.starts, p.best, want_grad=g, points_being_sampled=pend, **kw),
        lambda a, path, pend: api.kg_discrete_multistart(gps, p.gd, p.bounds, p.discrete, p.best, p.starts, gradient_ascent=a,
                                                         want_path=path, points_being_sampled=pend, **kw),
        lambda a, pend: api.kg_discrete_suggest(gps, p.gd, p.bounds, p.discrete, p.best, p.starts, Q, gradient_ascent=a,
                                                points_being_sampled=pend, **kw),
        pending)
    for g in gps:
        g.close()


def ei_case(tag, ep, derivs, members):
    gps = [api.DeviceGP(ep.hyper[k], ep.X[k], ep.y[k], ep.noise[k], derivs, cov_type=ep.cov[k]) for k in members]
    best = [ep.best[k] for k in members]
    d = ep.points.shape[1]
    starts = np.random.default_rng(77).uniform(0.02, 0.98, size=(12, d))
    gd = (12, 6, 2, 0, 0.7, 1.0, 0.5, 1e-10)
    bounds = np.array([[0.0, 1.0]] * d)
    all_calls(
        "ei %s E=%d" % (tag, len(members)),
        lambda g, pend: api.ei_analytic_ensemble(gps, ep.points, best, points_being_sampled=pend, want_grad=g),
        lambda a, path, pend: api.ei_analytic_multistart(gps, gd, bounds, best, starts, gradient_ascent=a, want_path=path,
                                                         points_being_sampled=pend),
        lambda a, pend: api.ei_analytic_suggest(gps, gd, bounds, best, starts, Q, gradient_ascent=a, points_being_sampled=pend),
        ep.pending)
    for g in gps:
        g.close()


def refusals():
    # tests/test_gpu_kg1_pending.py's construction: alpha = 1e-3, noise 0 in the second member, a pending point listed twice
    rng = np.random.default_rng(3)
    X, y = rng.uniform(0, 1, size=(6, 2)), 0.03 * rng.normal(size=(6, 1))
    hyper = [1e-3, 0.5, 0.5]
    near = X[2] + np.array([0.03, -0.04])
    pending = np.vstack([rng.uniform(0.1, 0.9, size=(1, 2)), near, rng.uniform(0.1, 0.9, size=(1, 2)), near])
    gps = [api.DeviceGP(hyper, X, y, [1e-5]), api.DeviceGP(hyper, X, y, [0.0])]
    sets = [rng.uniform(0, 1, size=(10, 2)), rng.uniform(0, 1, size=(7, 2))]
    bests = [float(y.min())] * 2
    starts = rng.uniform(0.1, 0.9, size=(5, 2))
    gd = (5, 3, 1, 0, kc.GAMMA, kc.PRE_MULT, kc.MAX_REL, 1e-10)
    box = [[0, 1], [0, 1]]
    refusal("kg singular pending point: evaluate", lambda: api.kg_discrete_ensemble(gps, sets, starts, bests, points_being_sampled=pending))
    refusal("kg singular pending point: multistart",
            lambda: api.kg_discrete_multistart(gps, gd, box, sets, bests, starts, points_being_sampled=pending))
    refusal("ei singular pending point: evaluate", lambda: api.ei_analytic_ensemble(gps, starts, bests, points_being_sampled=pending))
    refusal("ei singular pending point: suggest", lambda: api.ei_analytic_suggest(gps, gd, box, bests, starts, 2, points_being_sampled=pending))
    twice = [gps[0], gps[1], gps[0]]
    refusal("kg member listed twice", lambda: api.kg_discrete_ensemble(twice, sets + sets[:1], starts, bests + bests[:1]))
    refusal("kg member listed twice: suggest", lambda: api.kg_discrete_suggest(twice, gd, box, sets + sets[:1], bests + bests[:1], starts, 2))
    refusal("ei member listed twice", lambda: api.ei_analytic_ensemble(twice, starts, bests + bests[:1]))
    refusal("ei member listed twice: multistart", lambda: api.ei_analytic_multistart(twice, gd, box, bests + bests[:1], starts))
    say("the handles still answer", [api.kg_discrete_ensemble(gps, sets, starts, bests, want_grad=False, points_being_sampled=pending[:3]),
                                     api.ei_analytic_ensemble(gps, starts, bests, want_grad=False, points_being_sampled=pending[:3])])
    for g in gps:
        g.close()


for name in ("e1_n40_d4_A64_se_s8", "e3_n12_d2_A12_s8_tight", "e3_n12_40_d3_fid_s48_loose"):
    kg_case(name)
ei_case("g=0", er.make_ensemble(), (), (0, 1, 2))
ei_case("g=0", er.make_ensemble(), (), (0,))
ei_case("g=2", dr.make_ensemble(), dr.make_ensemble().derivs, (0, 1, 2))
ei_case("g=2", dr.make_ensemble(), dr.make_ensemble().derivs, (0,))
refusals()
