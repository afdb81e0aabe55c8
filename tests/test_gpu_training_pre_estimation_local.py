"""inference(..., pre_estimate={...}) on the MI355X: the model starts from pre_estimation_local's result, and an int
behaves as before.  The kernels and the estimator are checked in tests/test_gpu_pre_estimation_local.py; like
tests/test_gpu_training_pre_estimation.py these tests build models and engines, which open streams of their own, and
are kept in a file that runs after tests/test_gpu_primitives.py."""
import numpy as np
import pytest

from tests import _golden as G

pytestmark = pytest.mark.gpu


TOY_HYPER = {"sigma2_L0_log": 0., "length_scales_L0_log": 2., "sigma2_L1_log": 0., "length_scales_L1_log": 2.,
             "sigma2_tildeell_log": 0., "length_scales_tildeell_log": 0.}


def _toy():
    """The toy fixture with the second output's values placed on the first output's inputs (as it stands it has no
    complete row)."""
    g = G.load("toy_forward")
    xs, ys = G.split_lists(g)
    order = np.argsort(xs[0], kind="stable")
    xu = np.unique(xs[0])
    assert xu.size == xs[0].size
    X_list, Y_list = [xs[0][:, None], xs[0][:, None]], [ys[0][:, None], ys[1][:, None]]
    return g, X_list, Y_list, xu, np.stack([ys[0][order], ys[1][order]], 1)


def _start(model):
    return (model.mu_v.detach().cpu().numpy().reshape(-1), model.mu_U_dense().detach().cpu().numpy(),
            float(model.sigma2_err_log))


def test_inference_seeded_by_the_local_pre_estimation():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import nmgp_dsvi as ND
    g, X_list, Y_list, xu, Yg = _toy()
    want = ND.init_from_pre_estimation(*ND.pre_estimation_local(xu, Yg, g["z"], P=10, cov_rows=40, device="cuda:0"))
    model, losses, _ = ND.inference(X_list, Y_list, g["z"], 200, 2, hyperpars=dict(TOY_HYPER), lr=0.0, itnum=1,
                                    show_ELBO=False, device="cuda:0", pre_estimate={"P": 10, "cov_rows": 40})
    assert len(losses) == 1 and np.isfinite(losses[0])
    mu_v, mu_U, s = _start(model)                                       # lr = 0: the initial state
    assert np.array_equal(mu_U, want["mu_U"]) and np.array_equal(mu_v, want["mu_v"]) and s == want["sigma2_err_log"]
    assert not np.array_equal(mu_U[:, :, 0], mu_U[:, :, -1])            # a factor per inducing point
    # the other keys reach the estimator
    want2 = ND.init_from_pre_estimation(*ND.pre_estimation_local(xu, Yg, g["z"], P=8, cov_rows=30, shrink=0.5,
                                                                 holdout=False, device="cuda:0"))
    model, _, _ = ND.inference(X_list, Y_list, g["z"], 200, 2, hyperpars=dict(TOY_HYPER), lr=0.0, itnum=1,
                               show_ELBO=False, device="cuda:0",
                               pre_estimate={"P": 8, "cov_rows": 30, "shrink": 0.5, "holdout": False})
    assert np.array_equal(_start(model)[1], want2["mu_U"])
    with pytest.raises(ValueError, match="cov_rows"):
        ND.inference(X_list, Y_list, g["z"], 200, 2, hyperpars=dict(TOY_HYPER), itnum=1, show_ELBO=False,
                     device="cuda:0", pre_estimate={"P": 10})


def test_an_int_starts_as_before():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import nmgp_dsvi as ND
    g, X_list, Y_list, xu, Yg = _toy()
    want = ND.init_from_pre_estimation(*ND.pre_estimation(xu, Yg, g["z"], P=10, device="cuda:0"))
    model, _, _ = ND.inference(X_list, Y_list, g["z"], 200, 2, hyperpars=dict(TOY_HYPER), lr=0.0, itnum=1,
                               show_ELBO=False, device="cuda:0", pre_estimate=10)
    mu_v, mu_U, s = _start(model)
    assert np.array_equal(mu_U, want["mu_U"]) and np.array_equal(mu_v, want["mu_v"]) and s == want["sigma2_err_log"]
    for m in range(mu_U.shape[2]):
        assert np.array_equal(mu_U[:, :, m], mu_U[:, :, 0])             # the global factor, copied
