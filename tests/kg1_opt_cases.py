"""TEST INFRASTRUCTURE: the cases of tests/test_gpu_kg1_opt.py (the ensemble-averaged discretised knowledge gradient and its
multistart ascent, csrc/kg1_opt.hip), and their float64 restatement on the CPU -- tests/ms_restatement.py's optimiser over
tests/kg1_reference.py's evaluator averaged over the members -- with a record of what the optimiser did, which
tests/test_kg1_opt_reference.py holds the inputs to: every branch the device code has must be one these inputs take.

Outer parameters: gamma 0.7, pre_mult 1.0, max_relative_change 0.5 (the reference's examples/main.py).  With max_relative_change
<= 1 a step is clipped to at most the distance to the nearer bound, so a point inside the domain never leaves it and the limiter's
two other outcomes (the step halved at a bound; half-way to the bound) cannot occur: the case `wide_limiter` runs the same
optimiser with max_relative_change 3 so that the device's code for them is compared too.
"""
import collections
import math

import numpy as np

import kg1_reference as kr
import ms_restatement as ms

SE, MATERN = kr.SE, kr.MATERN
GAMMA, PRE_MULT, MAX_REL = 0.7, 1.0, 0.5

# n: sampled points per member; A: discrete points per member; cov: covariance per member
Case = collections.namedtuple("Case", "name seed d nf n A cov starts steps restarts tolerance max_rel")
CASES = [
    # equal A, same N: every launch of the members merges
    Case("e3_n12_d2_A12_s8_tight", 1, 2, 0, (12, 12, 12), (12, 12, 12), (MATERN, MATERN, MATERN), 8, 12, 2, 1e-10, MAX_REL),
    # unequal A (the slope and envelope launches fall back to member after member), Matern and SE members, top_k_order drops starts
    Case("e4_n40_d3_A1_12_64_129_s48_loose", 12, 3, 0, (40, 40, 40, 40), (1, 12, 64, 129), (MATERN, SE, MATERN, SE), 48, 8, 2, 6e-2,
         MAX_REL),
    # one member: the single-GP path
    Case("e1_n40_d4_A64_se_s8", 3, 4, 0, (40,), (64,), (SE,), 8, 6, 1, 1e-10, MAX_REL),
    # a fidelity coordinate; members of different N (nothing merges)
    Case("e3_n12_40_d3_fid_s48_loose", 34, 3, 1, (12, 40, 12), (12, 64, 12), (MATERN, MATERN, SE), 48, 6, 2, 6e-2, MAX_REL),
    # max_relative_change 3: the limiter's halved and half-way outcomes
    Case("wide_limiter", 6, 2, 0, (12, 12, 12), (12, 12, 12), (MATERN, SE, MATERN), 8, 6, 1, 1e-10, 3.0),
    # a tolerance so loose that every start stops before the last step of a round: the device goes on with masked steps where the
    # host loop leaves the round
    Case("e4_n40_d3_all_stop_early", 12, 3, 0, (40, 40, 40, 40), (1, 12, 64, 129), (MATERN, SE, MATERN, SE), 48, 8, 2, 0.12, MAX_REL),
    # padded dimensions 24 (with a fidelity coordinate) and 32: the gather, step and round kernels over every coordinate of dp
    Case("e2_n20_d17_fid_s8", 51, 17, 1, (20, 20), (12, 12), (MATERN, SE), 8, 6, 2, 1e-10, MAX_REL),
    Case("e3_n20_d32_s8", 52, 32, 0, (20, 20, 12), (12, 12, 12), (MATERN, SE, MATERN), 8, 4, 1, 1e-10, MAX_REL),
]
LOOSE = ("e4_n40_d3_A1_12_64_129_s48_loose", "e3_n12_40_d3_fid_s48_loose")

Problem = collections.namedtuple("Problem", "case hyper X y noise discrete best bounds starts gd")
FACTORS = (1.0, 1.3, 0.8, 1.15)


def make_problem(case):
    """member e: the first n[e] of the shared sampled points, hyper-parameters and noise scaled by FACTORS[e], its own discrete set"""
    rng = np.random.default_rng(9100 + case.seed)
    E, nmax = len(case.n), max(case.n)
    X = rng.uniform(0, 1, size=(nmax, case.d))
    y = rng.normal(size=(nmax, 1))
    base = np.array([1.3] + [0.1 + 0.25 * math.sqrt(case.d)] * case.d)
    hyper = [base * FACTORS[e] for e in range(E)]
    noise = [[1e-2 * FACTORS[e]] for e in range(E)]
    discrete = [rng.uniform(0, 1, size=(case.A[e], case.d - case.nf)) for e in range(E)]
    best = [float(y[:case.n[e]].min()) + 0.1 * e for e in range(E)]
    bounds = np.array([[0.0, 1.0]] * case.d)
    starts = rng.uniform(0.02, 0.98, size=(case.starts, case.d))
    if case.max_rel > 1.0:  # (close to the faces of the domain: a step of a few hundredths leaves it)
        near = 0.004 * (1 + np.arange(case.starts))
        starts[:, 0] = np.where(np.arange(case.starts) % 2 == 0, near, 1.0 - near)
        starts[:, 1] = np.where(np.arange(case.starts) % 4 < 2, near[::-1], 1.0 - near[::-1])
    gd = (case.starts, case.steps, case.restarts, 0, GAMMA, PRE_MULT, case.max_rel, case.tolerance)
    return Problem(case, hyper, [X[:n] for n in case.n], [y[:n] for n in case.n], noise, discrete, best, bounds, starts, gd)


def discrete_sets(p, T):
    """the members' kg1_reference.DiscreteSet in the arithmetic of T"""
    c = p.case
    return [kr.DiscreteSet(kr.Model(c.cov[e], p.hyper[e], p.X[e], p.y[e], p.noise[e], T), p.discrete[e], c.nf) for e in range(len(c.n))]


def ensemble_value(sets, p, x, T):
    """(sum_e KG_e(x)) / E in the arithmetic of T, members in order; and the members' results"""
    res = [kr.evaluate(s, x, b, want_grad=False) for s, b in zip(sets, p.best)]
    total = T(0)
    for r in res:
        total = total + T(r.value)
    return total / T(len(res)), res


Record = collections.namedtuple("Record", "point value found start_values kept ends end_values limiter rounds")

_RUNS = {}


def float64_run(case, starts=None):
    """ms_restatement.multistart_best over the float64 evaluator, once per process, with its record:
    limiter: how often each outcome of the limiter occurred [clipped, halved at a bound, half-way to the bound];
    rounds: per restart round the list (per step) of the kept starts that took the step.
    starts: other starts than the case's own (not kept for the process)."""
    if starts is None and case.name in _RUNS:
        return _RUNS[case.name]
    p = make_problem(case)
    if starts is not None:
        p = p._replace(starts=np.asarray(starts, dtype=np.float64))
    sets = discrete_sets(p, np.float64)
    E = len(sets)

    def value_fn(x):
        x = np.asarray(x, dtype=np.float64).reshape(-1, case.d)
        return np.array([float(ensemble_value(sets, p, xi, np.float64)[0]) for xi in x])

    def grad_fn(x):
        x = np.asarray(x, dtype=np.float64).reshape(-1, case.d)
        out = np.zeros_like(x)
        for i, xi in enumerate(x):
            g = None
            for s, b in zip(sets, p.best):
                ge = kr.evaluate(s, xi, b).grad.astype(np.float64)
                g = ge if g is None else g + ge
            out[i] = g / E
        return out

    limiter = [0, 0, 0]
    plain = ms.limit_update

    def recording_limit_update(bounds, max_relative_change, x, step):
        b = np.asarray(bounds, dtype=np.float64).reshape(-1, 2)
        lo, hi = b[:, 0], b[:, 1]
        step = np.asarray(step, dtype=np.float64)
        dist = np.minimum(x - lo, hi - x)
        big = np.abs(step) > max_relative_change * dist
        clipped = np.where(big, np.copysign(max_relative_change * dist, step), step)
        out = (x + clipped < lo) | (x + clipped > hi)
        far = np.where(x + clipped < lo, x + 0.5 * clipped < lo, x + 0.5 * clipped > hi)
        limiter[0] += int(np.sum(big))
        limiter[1] += int(np.sum(out & ~far))
        limiter[2] += int(np.sum(out & far))
        return plain(bounds, max_relative_change, x, step)

    rounds = []

    def on_step(i, idx):
        if i == 0:
            rounds.append([])
        rounds[-1].append([int(k) for k in idx])

    vals = value_fn(p.starts)
    order = ms.top_k_order(vals)
    ms.limit_update = recording_limit_update
    try:
        ends = ms.gradient_ascent(grad_fn, p.gd, p.bounds, p.starts[order], on_step=on_step)
    finally:
        ms.limit_update = plain
    end_vals = value_fn(ends)
    best, best_val, found = np.zeros(case.d), -np.inf, False
    for s in range(ends.shape[0]):
        if end_vals[s] > best_val:
            best, best_val, found = ends[s].copy(), float(end_vals[s]), True
    run = (p, Record(best, best_val, found, vals, order, ends, end_vals, tuple(limiter), rounds))
    if starts is None:
        _RUNS[case.name] = run
    return run
