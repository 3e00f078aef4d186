"""Hyper-parameter training on the device: the priors of the reference's base_prior.py / default_priors.py as data holders that
lower to the prior table of moe_ll_mcmc, and GaussianProcessLogLikelihoodMCMC (python/cpp_wrappers/log_likelihood_mcmc.py),
whose train() runs the ensemble sampler as ONE device call per chain instead of handing a Python log posterior to emcee.

The flow of train() is the reference's (:170-239): burn-in once from a prior sample, then the sampling chain; the last positions
start the next call; n_hypers walkers of the last step, those inside +-20, become the GaussianProcessMCMC ensemble.
All randomness comes from the `rng` (numpy.random.RandomState) given to the constructor: the same seed gives the same result.
"""
import copy

import numpy as np

from . import GPP, _lib, api

BOX = 20.0  # log_likelihood_mcmc.py:286


class _Prior(object):
    """A prior over log-space hyper-parameters: table(nh) lowers it to rows (kind, a, b); sample_from_prior(n) -> [n][columns]."""

    def __init__(self, rng=None):
        self.rng = np.random.RandomState(42) if rng is None else rng  # (base_prior.py:24-27)

    def row(self):
        raise NotImplementedError

    def table(self, nh):
        return [self.row()] * int(nh)


class TophatPrior(_Prior):
    def __init__(self, l_bound, u_bound, rng=None):
        super(TophatPrior, self).__init__(rng)
        self.min, self.max = float(l_bound), float(u_bound)
        if not self.max > self.min:
            raise ValueError("upper bound of a tophat prior must be greater than the lower bound")

    def row(self):
        return (_lib.PRIOR_TOPHAT, self.min, self.max)

    def sample_from_prior(self, n_samples):
        return (self.min + self.rng.rand(n_samples) * (self.max - self.min))[:, np.newaxis]  # base_prior.py:140


class HorseshoePrior(_Prior):
    def __init__(self, scale=0.1, rng=None):
        super(HorseshoePrior, self).__init__(rng)
        self.scale = float(scale)

    def row(self):
        return (_lib.PRIOR_HORSESHOE, self.scale, 0.0)

    def sample_from_prior(self, n_samples):
        lamda = np.abs(self.rng.standard_cauchy(size=n_samples))  # base_prior.py:218-220: ONE normal draw for all samples
        return np.log(np.abs(self.rng.randn() * lamda * self.scale))[:, np.newaxis]


class LognormalPrior(_Prior):
    def __init__(self, sigma, mean=0.0, rng=None):
        super(LognormalPrior, self).__init__(rng)
        self.sigma, self.mean = float(sigma), float(mean)

    def row(self):
        return (_lib.PRIOR_LOGNORMAL, self.sigma, self.mean)

    def sample_from_prior(self, n_samples):
        return self.rng.lognormal(mean=self.mean, sigma=self.sigma, size=n_samples)[:, np.newaxis]  # base_prior.py:298


class NormalPrior(_Prior):
    def __init__(self, sigma, mean=0.0, rng=None):
        super(NormalPrior, self).__init__(rng)
        self.sigma, self.mean = float(sigma), float(mean)

    def row(self):
        return (_lib.PRIOR_NORMAL, self.mean, self.sigma)

    def sample_from_prior(self, n_samples):  # (base_prior.py:371 draws from numpy's global generator; here the prior's own)
        return self.rng.normal(loc=self.mean, scale=self.sigma, size=n_samples)[:, np.newaxis]


class DefaultPrior(_Prior):
    """default_priors.py:19-35: NORMAL(0, 1) on log alpha, TOPHAT(-2, 3) on the log lengths, HORSESHOE(0.1) on the log noises."""

    def __init__(self, n_dims, num_noise, rng=None):
        super(DefaultPrior, self).__init__(rng)
        self.n_dims, self.num_noise = int(n_dims), int(num_noise)
        self.ln_prior = NormalPrior(mean=0.0, sigma=1.0, rng=self.rng)
        self.tophat = TophatPrior(-2, 3, rng=self.rng)
        self.horseshoe = HorseshoePrior(scale=0.1, rng=self.rng)

    def table(self, nh=None):
        if nh is not None and int(nh) != self.n_dims:
            raise ValueError("DefaultPrior was built for %d hyper-parameters, not %d" % (self.n_dims, nh))
        return ([self.ln_prior.row()] + [self.tophat.row()] * (self.n_dims - 1 - self.num_noise)
                + [self.horseshoe.row()] * self.num_noise)

    def sample_from_prior(self, n_samples):
        p0 = np.zeros((n_samples, self.n_dims))
        p0[:, 0] = self.ln_prior.sample_from_prior(n_samples)[:, 0]
        for k in range(1, self.n_dims - self.num_noise):
            p0[:, k] = self.tophat.sample_from_prior(n_samples)[:, 0]
        for k in range(self.n_dims - self.num_noise, self.n_dims):
            p0[:, k] = self.horseshoe.sample_from_prior(n_samples)[:, 0]
        return p0


class GaussianProcessLogLikelihoodMCMC(object):
    """cpp_wrappers.log_likelihood_mcmc.GaussianProcessLogLikelihoodMCMC on the device.  historical_data: an object with dim,
    num_sampled, points_sampled [n][dim], points_sampled_value [n][1 + g] and append_sample_points (data_containers.HistoricalData).
    prior: one of the classes above, or None (flat).  noisy=False pins the noise coordinates at log 1e-8 (FIXED)."""

    def __init__(self, historical_data, derivatives, prior, chain_length, burnin_steps, n_hypers,
                 log_likelihood_type=GPP.LogLikelihoodTypes.log_marginal_likelihood, noisy=True, rng=None,
                 cov_type=_lib.COV_MATERN_NU_2P5, device=0):
        GPP._check_objective(log_likelihood_type)
        self._historical_data = copy.deepcopy(historical_data)
        self._derivatives = [int(v) for v in derivatives]
        self._num_derivatives = len(self._derivatives)
        self.objective_type = log_likelihood_type
        self.prior = prior
        self.chain_length, self.burnin_steps, self.n_hypers = int(chain_length), int(burnin_steps), int(n_hypers)
        self.noisy = bool(noisy)
        self.burned = False
        self.is_trained = False
        self.rng = np.random.RandomState(np.random.randint(0, 10000)) if rng is None else rng
        self.n_chains = max(self.n_hypers, 2 * self.num_hyperparameters)  # log_likelihood_mcmc.py:122
        self.n_chains += self.n_chains % 2  # (the two halves of the ensemble are equal)
        self._cov_type, self._device = cov_type, int(device)
        self._ll = None
        self._models = []
        self._gaussian_process_mcmc = None
        self.p0 = None
        self.hypers = None

    dim = property(lambda self: self._historical_data.dim)
    num_derivatives = property(lambda self: self._num_derivatives)
    derivatives = property(lambda self: self._derivatives)
    models = property(lambda self: self._models)
    num_hyperparameters = property(lambda self: 1 + self.dim + 1 + self._num_derivatives)
    gaussian_process_mcmc = property(lambda self: self._gaussian_process_mcmc)

    def get_historical_data_copy(self):
        return copy.deepcopy(self._historical_data)

    def _data(self):
        hd = self._historical_data
        X = np.asarray(hd.points_sampled, dtype=np.float64).reshape(hd.num_sampled, self.dim)
        y = np.asarray(hd.points_sampled_value, dtype=np.float64).reshape(hd.num_sampled, 1 + self._num_derivatives)
        return X, y

    def _handle(self):
        if self._ll is None:
            X, y = self._data()
            self._ll = api.LogLikelihood(X, y, self._derivatives, cov_type=self._cov_type, device=self._device,
                                         objective=int(self.objective_type))
        return self._ll

    def prior_table(self):
        nh = self.num_hyperparameters
        table = [(_lib.PRIOR_NONE, 0.0, 0.0)] * nh if self.prior is None else list(self.prior.table(nh))
        if not self.noisy:  # log_likelihood_mcmc.py:288-289
            for k in range(self.dim + 1, nh):
                table[k] = (_lib.PRIOR_FIXED, float(np.log(1.0e-8)), 0.0)
        return table

    def _run(self, p0, num_steps):
        W = self.n_chains
        tables = api.stretch_tables(self.rng, num_steps, W)
        return api.ll_mcmc(self._handle(), self.prior_table(), p0, *tables, diagnostics=False)

    def _initial_walkers(self):
        W, nh = self.n_chains, self.num_hyperparameters
        draw = (lambda n: self.rng.rand(n, nh)) if self.prior is None else self.prior.sample_from_prior
        p0 = np.array(draw(W), dtype=np.float64).reshape(W, nh)
        for _ in range(100 * W):  # a prior sample the box or the prior itself rejects is drawn again
            try:
                self._run(p0, 0)
                return p0
            except api.InvalidValueException as e:
                p0[int(e.value)] = np.array(draw(1), dtype=np.float64).reshape(nh)
        raise api.OptimalLearningException("no prior sample with a finite log posterior")

    def train(self, do_optimize=True, **kwargs):
        if do_optimize or self.hypers is None:
            if not self.burned:
                self.p0 = self._initial_walkers()
                if self.burnin_steps > 0:
                    self.p0 = self._run(self.p0, self.burnin_steps)["chain"][-1]
                self.burned = True
            if self.chain_length > 0:
                self.p0 = self._run(self.p0, self.chain_length)["chain"][-1]
            self.hypers = np.array(self.p0[self.rng.choice(self.n_chains, self.n_hypers)])  # (:214, from this object's rng)
        self.is_trained = True
        X, y = self._data()
        n, g = X.shape[0], self._num_derivatives
        hypers_list, noises_list, self._models = [], [], []
        for sample in self.hypers:
            if np.any(np.abs(sample) > BOX):
                continue
            lin = np.exp(sample)
            cov_hyps = lin[:self.dim + 1]
            noise = lin[self.dim + 1:] if self.noisy else np.full(1 + g, 1.0e-8)
            hypers_list.append(cov_hyps)
            noises_list.append(noise)
            self._models.append(GPP.GaussianProcess([cov_hyps[0], list(cov_hyps[1:])], X.ravel(), y.ravel(), list(noise),
                                                    self._derivatives, g, self.dim, n, cov_type=self._cov_type,
                                                    device=self._device))
        self._gaussian_process_mcmc = GPP.GaussianProcessMCMC(np.ravel(hypers_list), np.ravel(noises_list), X.ravel(), y.ravel(),
                                                              self._derivatives, len(hypers_list), g, self.dim, n,
                                                              device=self._device)

    def compute_log_likelihood(self, hyps):
        """The log posterior of ONE log-space hyper-parameter vector (:277-312) as the sampler defines it: the device evaluates
        it as the initial log posterior of an ensemble of copies of `hyps` (a chain of no steps)."""
        nh = self.num_hyperparameters
        hyps = np.array(hyps, dtype=np.float64).reshape(nh)
        try:
            out = api.ll_mcmc(self._handle(), self.prior_table(), np.tile(hyps, (2 * nh, 1)), *api.stretch_tables(self.rng, 0, 2 * nh),
                              diagnostics=False)
        except api.InvalidValueException as e:  # not finite: the payload carries the value
            return float(e.truth) if e.truth == np.inf else -np.inf
        return float(out["lnprob0"][0])

    compute_objective_function = compute_log_likelihood

    def add_sampled_points(self, sampled_points):
        """Append (point, value, noise) samples to the data; the walkers keep their positions for the next train()."""
        self._historical_data.append_sample_points(sampled_points)
        if self._ll is not None:
            self._ll.close()
            self._ll = None
