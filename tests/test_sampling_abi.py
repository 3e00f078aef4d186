"""CPU tests (-m "not gpu") of the joint posterior sampling entry points: bad arguments come back as error codes, and without a
device the Python boundary fails loudly (no CPU fallback)."""
import ctypes as C

import numpy as np

from cornell_moe_amd import _lib, api


def test_sampling_symbols_declared_and_bound():
    L = _lib.load()
    for name in ("moe_gp_sample_points", "moe_gp_sample_global_optima"):
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None


def test_null_handle_is_an_error():
    L = _lib.load()
    err = _lib.MoeError()
    pts = np.zeros(4)
    z = np.zeros(4)
    vals = np.zeros(4)
    am = np.zeros(4, dtype=np.int32)
    fp = C.c_int(0)
    dp, ip = _lib.dp, _lib.ip
    rc = L.moe_gp_sample_points(None, pts.ctypes.data_as(dp), 2, z.ctypes.data_as(dp), 2, vals.ctypes.data_as(dp),
                                am.ctypes.data_as(ip), C.byref(fp), C.byref(err))
    assert rc != _lib.MOE_OK and err.code == rc
    rc = L.moe_gp_sample_global_optima(None, pts.ctypes.data_as(dp), 2, 1, z.ctypes.data_as(dp), vals.ctypes.data_as(dp),
                                       am.ctypes.data_as(ip), am.ctypes.data_as(ip), C.byref(err))
    assert rc != _lib.MOE_OK and err.code == rc
    # non-positive sizes with a NULL handle are still an error code, not a crash
    rc = L.moe_gp_sample_points(None, None, 0, None, 0, None, None, None, None)
    assert rc != _lib.MOE_OK


def test_no_cpu_fallback():
    """Without a device GPP.GaussianProcess (and so sample_global_optima) raises; with one this is covered by -m gpu tests."""
    if _lib.device_count() > 0:
        return
    from cornell_moe_amd import GPP
    X = np.random.default_rng(0).uniform(size=(10, 2))
    try:
        GPP.GaussianProcess([1.0, [0.5, 0.5]], list(X.ravel()), [0.0] * 10, [0.1], [], 0, 2, 10)
    except api.OptimalLearningException as e:
        assert "no CPU fallback" in str(e)
    else:
        raise AssertionError("a GP was created without a device")
