"""Restatement in numpy of what moe_ll_mcmc computes (include/moe_hip.h): the prior table, the log posterior and ONE half-step of
the stretch move.  The likelihood comes from the plain-C oracle (oracle.orc.log_likelihood), which tests/test_oracle.py holds to
the reference's fixture.  TEST INFRASTRUCTURE ONLY.  It follows the header's description and shares no code with the library.
"""
import numpy as np

NONE, TOPHAT, NORMAL, HORSESHOE, LOGNORMAL, FIXED = 0, 1, 2, 3, 4, 5
BOX = 20.0


def default_prior_table(nh, num_noise):
    """default_priors.py:19-35"""
    return [(NORMAL, 0.0, 1.0)] + [(TOPHAT, -2.0, 3.0)] * (nh - 1 - num_noise) + [(HORSESHOE, 0.1, 0.0)] * num_noise


def prior_term(kind, a, b, theta, quirks):
    """log prior of one log-space coordinate"""
    with np.errstate(divide="ignore", over="ignore"):
        if kind == TOPHAT:
            return -np.inf if (theta < a or theta > b) else 0.0
        if kind == NORMAL:  # (mean a, sigma b)
            t = (theta - a) / b
            if quirks:  # base_prior.py:354: the density itself
                return float(np.exp(-0.5 * t * t) / (b * np.sqrt(2.0 * np.pi)))
            return float(-0.5 * t * t - np.log(b) - 0.5 * np.log(2.0 * np.pi))
        if kind == HORSESHOE:  # (scale a)
            if quirks:  # base_prior.py:199-201, on the log-space coordinate
                if theta == 0.0:
                    return np.inf
                return float(np.log(np.log(1 + 3.0 * (a / theta) ** 2)))
            return float(np.log(np.log1p(3.0 * (a / np.exp(theta)) ** 2)))
        if kind == LOGNORMAL:  # (sigma a, mean b): scipy.stats.lognorm.logpdf(theta, a, loc=b)
            y = theta - b
            if not y > 0.0:
                return -np.inf
            return float(-np.log(y) ** 2 / (2.0 * a ** 2) - np.log(a * y * np.sqrt(2.0 * np.pi)))
        return 0.0


def log_prior(table, theta, quirks):
    terms = [prior_term(k, a, b, th, quirks) for (k, a, b), th in zip(table, theta)]
    if any(v == -np.inf or v != v for v in terms):
        return -np.inf
    if any(v == np.inf for v in terms):
        return np.inf
    return float(sum(terms))


def apply_fixed(table, theta):
    theta = np.array(theta, dtype=np.float64)
    for k, (kind, a, _) in enumerate(table):
        if kind == FIXED:
            theta[k] = a
    return theta


def nh_free(table):
    return sum(1 for kind, _, _ in table if kind != FIXED)


class Posterior(object):
    """theta (FIXED applied) -> log posterior of the data (X [n][d], y [n][1 + g], derivs, cov_type) under a prior table"""

    def __init__(self, cov_type, X, y, derivs, table, quirks):
        self.cov_type, self.X, self.derivs = int(cov_type), np.asarray(X, dtype=np.float64), [int(v) for v in derivs]
        self.y = np.asarray(y, dtype=np.float64).reshape(self.X.shape[0], 1 + len(self.derivs))
        self.table, self.quirks = list(table), bool(quirks)

    def __call__(self, theta):
        from oracle import orc
        d = self.X.shape[1]
        if not np.all(np.abs(theta) <= BOX):
            return -np.inf
        lp = log_prior(self.table, theta, self.quirks)
        if lp == -np.inf:
            return -np.inf
        lin = np.exp(theta)
        try:
            ll = orc.log_likelihood(self.cov_type, lin[0], lin[1:1 + d], self.X, self.y.ravel(), lin[1 + d:], self.derivs)
        except orc.SingularMatrix:
            return -np.inf
        return lp + ll


def stretch_z(a, u):
    return ((a - 1.0) * u + 1.0) ** 2 / a


def half_step(walkers, lnp, half, u_stretch, partner, u_accept, table, lnpost, a=2.0):
    """One half-step from the state (walkers [W][nh], lnp [W]): the moving half `half` against the other.
    u_stretch, partner, u_accept: [W/2].  Returns a dict of per-moving-walker arrays: index (walker), proposal [H][nh],
    proposal_lnprob, lnr, lnu, accept; the state itself is not modified."""
    W, nh = walkers.shape
    H = W // 2
    idx = np.arange(H) + half * H
    other = (1 - half) * H
    nf = nh_free(table)
    out = dict(index=idx, proposal=np.zeros((H, nh)), proposal_lnprob=np.zeros(H), lnr=np.zeros(H), lnu=np.zeros(H),
               accept=np.zeros(H, dtype=bool))
    for i in range(H):
        s, c = walkers[idx[i]], walkers[other + int(partner[i])]
        z = stretch_z(a, u_stretch[i])
        prop = apply_fixed(table, c - z * (c - s))
        lp = lnpost(prop)
        with np.errstate(divide="ignore", invalid="ignore"):
            lnr = (nf - 1) * np.log(z) + lp - lnp[idx[i]]
            lnu = np.log(u_accept[i])
        out["proposal"][i], out["proposal_lnprob"][i], out["lnr"][i], out["lnu"][i] = prop, lp, lnr, lnu
        out["accept"][i] = bool(lp == np.inf or lnr > lnu)
    return out


def run_chain(p0, u_stretch, partner, u_accept, table, lnpost, a=2.0):
    """The whole chain on the host: tables [T][2][W/2].  Returns chain [T][W][nh], lnprob [T][W], lnprob0 [W], proposal_lnprob,
    accepted [T][W] and margin [T][W] = |ln u - ln r| / max(1, |ln r|) of every decision."""
    W, nh = p0.shape
    T = u_stretch.shape[0]
    walkers = np.array([apply_fixed(table, w) for w in p0])
    lnp = np.array([lnpost(w) for w in walkers])
    res = dict(chain=np.zeros((T, W, nh)), lnprob=np.zeros((T, W)), lnprob0=lnp.copy(), proposal_lnprob=np.zeros((T, W)),
               accepted=np.zeros((T, W), dtype=np.int32), margin=np.full((T, W), np.inf))
    for t in range(T):
        for h in range(2):
            hs = half_step(walkers, lnp, h, u_stretch[t, h], partner[t, h], u_accept[t, h], table, lnpost, a)
            for i, w in enumerate(hs["index"]):
                if hs["accept"][i]:
                    walkers[w], lnp[w] = hs["proposal"][i], hs["proposal_lnprob"][i]
                res["proposal_lnprob"][t, w], res["accepted"][t, w] = hs["proposal_lnprob"][i], int(hs["accept"][i])
                if np.isfinite(hs["lnr"][i]) and np.isfinite(hs["lnu"][i]):
                    res["margin"][t, w] = abs(hs["lnu"][i] - hs["lnr"][i]) / max(1.0, abs(hs["lnr"][i]))
        res["chain"][t], res["lnprob"][t] = walkers, lnp
    return res


def stretch_tables(rng, T, W):
    """per half-step: W/2 uniforms for z, W/2 partner indices, W/2 uniforms for the accept (the order the header fixes)"""
    H = W // 2
    us, pt, ua = np.zeros((T, 2, H)), np.zeros((T, 2, H), dtype=np.int32), np.zeros((T, 2, H))
    for t in range(T):
        for h in range(2):
            us[t, h] = rng.rand(H)
            pt[t, h] = rng.randint(H, size=H)
            ua[t, h] = rng.rand(H)
    return us, pt, ua


# ---- the problems of tests/test_gpu_hyper_mcmc.py (here so that the CPU suite can check their seeds without a device) ----
def make_problem(n, d, g, seed):
    rng = np.random.RandomState(seed)
    X = rng.uniform(size=(n, d))
    f = np.sin(3.0 * X[:, 0]) + 0.5 * np.cos(2.0 * X.sum(axis=1))
    y = np.zeros((n, 1 + g))
    y[:, 0] = f + 0.05 * rng.standard_normal(n)
    derivs = list(range(g))
    for j, k in enumerate(derivs):
        df = 0.5 * -2.0 * np.sin(2.0 * X.sum(axis=1)) + (3.0 * np.cos(3.0 * X[:, 0]) if k == 0 else 0.0)
        y[:, 1 + j] = df + 0.05 * rng.standard_normal(n)
    return X, y, derivs


def start_walkers(rng, W, d, g, table=None):
    """walkers near plausible hyper-parameters: log alpha ~ 0, log lengths ~ log 0.5, log noises ~ -3, spread 0.3"""
    nh = 1 + d + 1 + g
    centre = np.r_[0.0, np.full(d, np.log(0.5)), np.full(1 + g, -3.0)]
    p0 = centre + 0.3 * rng.standard_normal((W, nh))
    return p0 if table is None else np.array([apply_fixed(table, w) for w in p0])


# (name, cov_type [0 SE, 1 Matern-5/2], n, d, g, prior, quirks, W or None for 2 nh, T, seed)
#   prior: "default" | "fixed_noise" (DefaultPrior + noisy=False) | "wall" (a narrow tophat on the lengths) | "box" (walker 0
#   started with its noise coordinate at 19.9)
CASES = [
    ("matern_12_2_0", 1, 12, 2, 0, "default", True, None, 12, 101),
    ("se_12_2_0_noquirks", 0, 12, 2, 0, "default", False, None, 12, 102),
    ("matern_40_3_0", 1, 40, 3, 0, "default", True, 16, 10, 103),
    ("se_40_3_0", 0, 40, 3, 0, "default", True, None, 10, 104),
    ("matern_25_3_2", 1, 25, 3, 2, "default", True, None, 8, 105),
    ("se_25_3_2_noquirks", 0, 25, 3, 2, "default", False, None, 8, 106),
    ("matern_300_6_0", 1, 300, 6, 0, "default", True, None, 5, 107),
    ("se_300_6_0_noquirks", 0, 300, 6, 0, "default", False, None, 4, 108),
    ("fixed_noise_40_3_0", 1, 40, 3, 0, "fixed_noise", True, None, 10, 109),
    ("tophat_wall_12_2_0", 1, 12, 2, 0, "wall", True, None, 12, 110),
    ("box_12_2_0", 1, 12, 2, 0, "box", True, None, 12, 111),
    # padded dimensions 12, 16, 24 and 32 of the covariance kernel, each with and without derivative observations (W = 2 nh up to 70)
    ("matern_20_12_0", 1, 20, 12, 0, "default", True, None, 4, 201),
    ("se_20_16_0", 0, 20, 16, 0, "default", True, None, 4, 202),
    ("matern_20_17_2", 1, 20, 17, 2, "default", True, None, 3, 203),
    ("se_20_24_0_noquirks", 0, 20, 24, 0, "default", False, None, 3, 204),
    ("matern_12_32_1", 1, 12, 32, 1, "default", True, None, 3, 205),
    ("se_20_25_0", 0, 20, 25, 0, "default", True, None, 3, 208),       # 32 without, 16 and 12 with derivative observations
    ("matern_12_14_1", 1, 12, 14, 1, "default", True, None, 3, 209),
    ("matern_12_10_1", 1, 12, 10, 1, "default", True, None, 3, 210),
    # W / 2 = 66 proposals: a second workgroup of the propose and accept kernels, and two passes (64 + 2 sets) of the likelihood
    ("matern_12_2_0_w132", 1, 12, 2, 0, "default", True, 132, 4, 206),
    # n (1 + g) = 300 rows: a second row block of the covariance kernel with derivative observations
    ("matern_100_3_2_rows300", 1, 100, 3, 2, "default", True, None, 3, 207),
]


def build_case(case):
    """-> dict(cov_type, X, y, derivs, table, quirks, p0, tables=(u_stretch, partner, u_accept))"""
    name, cov_type, n, d, g, prior, quirks, W, T, seed = case
    nh = 1 + d + 1 + g
    W = 2 * nh if W is None else W
    X, y, derivs = make_problem(n, d, g, seed)
    table = default_prior_table(nh, 1 + g)
    if prior == "fixed_noise":
        table = table[:1 + d] + [(FIXED, float(np.log(1.0e-8)), 0.0)] * (1 + g)
    if prior == "wall":
        table = [table[0]] + [(TOPHAT, -1.3, -0.1)] * d + table[1 + d:]
    rng = np.random.RandomState(seed + 1000)
    p0 = start_walkers(rng, W, d, g, table)
    if prior == "wall":
        p0[:, 1:1 + d] = np.clip(p0[:, 1:1 + d], -1.25, -0.15)
    if prior == "box":
        p0[0, 1 + d] = 19.9
    return dict(name=name, cov_type=cov_type, X=X, y=y, derivs=derivs, table=table, quirks=quirks, p0=p0,
                tables=stretch_tables(rng, T, W))
