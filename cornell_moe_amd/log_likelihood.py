"""The two model-selection objectives of python/cpp_wrappers/log_likelihood.py as classes over the device's evaluators.

``GaussianProcessLogMarginalLikelihood`` is log p(y | X, theta).  ``GaussianProcessLeaveOneOutLogLikelihood`` is the leave-one-out
log pseudo-likelihood (Rasmussen & Williams 5.4.2): every scalar observation -- a function value or one observed partial
derivative -- is predicted from all the others, and the log densities of the N predictions are added.  The reference ships the second
class without an evaluator behind it; here both go to the same handle (moe_ll_*), which computes whichever objective it is set to.

Both take the reference's constructor arguments: a covariance object with ``hyperparameters`` ([alpha, lengths...]), a historical
data object with ``dim``, ``num_sampled``, ``points_sampled`` [n][dim] and ``points_sampled_value`` [n][1 + g], the noise variances
[1 + g] and the list of observed partial derivatives.  Hyper-parameters are laid out [alpha, lengths[dim], noise variances[1 + g]].
"""
import copy

import numpy as np

from . import GPP


class _LogLikelihood(object):
    objective_type = GPP.LogLikelihoodTypes.log_marginal_likelihood

    def __init__(self, covariance_function, historical_data, noise_variance, derivatives):
        self._covariance = copy.deepcopy(covariance_function)
        self._historical_data = copy.deepcopy(historical_data)
        self._noise_variance = np.array(noise_variance, dtype=np.float64).ravel()
        self._derivatives = [int(v) for v in derivatives]

    dim = property(lambda self: self._historical_data.dim)
    derivatives = property(lambda self: self._derivatives)
    num_derivatives = property(lambda self: len(self._derivatives))
    noise_variance = property(lambda self: self._noise_variance)
    num_hyperparameters = property(lambda self: 1 + self.dim + self._noise_variance.size)
    problem_size = num_hyperparameters

    def get_hyperparameters(self):
        return np.concatenate([np.ravel(self._covariance.hyperparameters), self._noise_variance])

    def set_hyperparameters(self, hyperparameters):
        hyperparameters = np.asarray(hyperparameters, dtype=np.float64).ravel()
        self._covariance.hyperparameters = hyperparameters[:1 + self.dim]
        self._noise_variance = hyperparameters[1 + self.dim:].copy()

    hyperparameters = property(get_hyperparameters, set_hyperparameters)
    current_point = hyperparameters

    def get_covariance_copy(self):
        return copy.deepcopy(self._covariance)

    def get_historical_data_copy(self):
        return copy.deepcopy(self._historical_data)

    def _data(self):
        hd = self._historical_data
        return (np.asarray(hd.points_sampled, dtype=np.float64).ravel(), np.asarray(hd.points_sampled_value, dtype=np.float64).ravel(),
                self.dim, hd.num_sampled)

    def _boundary_operands(self):
        cov = np.ravel(self._covariance.hyperparameters)
        return self._data() + (self.objective_type, [float(cov[0]), [float(v) for v in cov[1:]]], self._derivatives,
                               self.num_derivatives, list(self._noise_variance))

    def compute_log_likelihood(self):
        """The objective at the current hyper-parameters (-inf where K + noise is singular)."""
        return GPP.compute_log_likelihood(*self._boundary_operands())

    def compute_grad_log_likelihood(self):
        """Its gradient with respect to [alpha, lengths, noise variances]."""
        return np.array(GPP.compute_hyperparameter_grad_log_likelihood(*self._boundary_operands()))

    compute_objective_function, compute_grad_objective_function = compute_log_likelihood, compute_grad_log_likelihood

    def leave_one_out_predictions(self):
        """(mean, variance), each [n][1 + g]: every observation predicted from all the others at the current hyper-parameters --
        the model check to run before trusting the surrogate.  The same for both objectives."""
        handle = GPP._ll_handle(*self._data(), derivatives=self._derivatives, num_derivatives=self.num_derivatives,
                                objective=self.objective_type)
        return handle.loo_predict(self.get_hyperparameters())


class GaussianProcessLogMarginalLikelihood(_LogLikelihood):
    """log p(y | X, theta) = -1/2 yc^T K^-1 yc - 1/2 log det K - N/2 log 2 pi."""

    objective_type = GPP.LogLikelihoodTypes.log_marginal_likelihood


class GaussianProcessLeaveOneOutLogLikelihood(_LogLikelihood):
    """sum_i log N(y_i; mu_i, var_i) over the leave-one-out predictions (mu_i, var_i) of the N scalar observations."""

    objective_type = GPP.LogLikelihoodTypes.leave_one_out_log_likelihood
