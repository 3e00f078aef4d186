"""Batch lower-confidence-bound selection (python/cpp_wrappers/lower_confidence_bound.py) as ONE device call.

The reference picks q of the candidates like this: the minimiser of mean - std first; then, q - 1 times, it appends the last pick
to the caller's GP as a zero-valued observation and takes the candidate with the largest remaining posterior standard deviation
among those whose lower bound does not exceed the smallest upper bound -- one compute_cholesky_variance_of_points call per candidate
and round.  Here the whole selection runs on the device (moe_gp_lcb_select) and the GP is only read.

What the reference leaves behind is reproduced under reference quirks (api.get_reference_quirks(), the default): its loop has
appended results[0 .. q-2] with zero values to the GP it was given, and so does this function, afterwards, in one rank-k append
through the GP's own add_sampled_points.  With quirks off the GP is untouched.  The noise of 0.25 that the reference writes into
its SamplePoint never reaches its C++ object (gaussian_process.py:334-339 passes no noise on); it is written here too, for the
wrapper's historical data, and ignored in the same way.
"""
import numpy as np

from . import api


def lower_confidence_bound_optimization(gaussian_process, candidate_pts, num_to_sample):
    """(results [num_to_sample][dim], 0.0), as the reference's function of the same name.

    gaussian_process: the wrapper-class GP of the reference's Python layer (its C-level object in ``._gaussian_process``) or a
    GPP.GaussianProcess itself.
    """
    candidate_pts = np.ascontiguousarray(candidate_pts, dtype=np.float64)
    num_to_sample = int(num_to_sample)
    inner = getattr(gaussian_process, "_gaussian_process", gaussian_process)
    dim = inner.dim
    flat = inner.lower_confidence_bound_select(candidate_pts.ravel(), candidate_pts.reshape(-1, dim).shape[0], num_to_sample)
    results = np.asarray(flat, dtype=np.float64).reshape(num_to_sample, dim)
    if api.get_reference_quirks() and num_to_sample > 1:
        g1 = 1 + int(getattr(inner, "_g", 0))
        if inner is gaussian_process:
            inner.add_sampled_points(results[:-1].ravel(), np.zeros((num_to_sample - 1) * g1), num_to_sample - 1)
        else:
            gaussian_process.add_sampled_points([(results[i].copy(), np.zeros(g1), 0.25) for i in range(num_to_sample - 1)])
    return results, 0.0
