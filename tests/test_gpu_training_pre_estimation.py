"""inference(..., pre_estimate=P) on the MI355X: the model starts from the estimator's result, and the keyword's
default leaves the training loop as it was.  The kernel and the estimator themselves are checked in
tests/test_gpu_pre_estimation.py; these two tests build models and engines, which open streams of their own, and are
kept in a file that runs after tests/test_gpu_primitives.py, whose external-event test depends on how many streams
the process has opened before it."""
import numpy as np
import pytest
import torch

from tests import _golden as G

pytestmark = pytest.mark.gpu


TOY_HYPER = {"sigma2_L0_log": 0., "length_scales_L0_log": 2., "sigma2_L1_log": 0., "length_scales_L1_log": 2.,
             "sigma2_tildeell_log": 0., "length_scales_tildeell_log": 0.}


def _toy_lists():
    g = G.load("toy_forward")
    xs, ys = G.split_lists(g)
    return g, xs, ys


def test_inference_seeded_by_the_pre_estimation():
    """The toy fixture observes its two outputs at disjoint inputs, so it has no complete row: as it stands it is
    refused; with the second output's values placed on the first output's inputs it runs, and the model starts from
    the estimator's result."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import nmgp_dsvi as ND
    from collaborative_nonstationary_multivariate_gaussian_process_amd import pre_nmgp as PN
    g, xs, ys = _toy_lists()
    with pytest.raises(ValueError, match="complete rows"):
        ND.inference([x[:, None] for x in xs], [y[:, None] for y in ys], g["z"], 200, 2, hyperpars=dict(TOY_HYPER),
                     itnum=1, show_ELBO=False, device="cuda:0", pre_estimate=10)
    X_list, Y_list = [xs[0][:, None], xs[0][:, None]], [ys[0][:, None], ys[1][:, None]]
    xu = np.unique(xs[0])
    order = np.argsort(xs[0], kind="stable")
    assert xu.size == xs[0].size
    v, Lt, s = PN.pre_estimation_partial(xu, np.stack([ys[0][order], ys[1][order]], 1), g["z"], P=10, device="cuda:0")
    want = ND.init_from_pre_estimation(v, Lt, s)
    model, losses, _ = ND.inference(X_list, Y_list, g["z"], 200, 2, hyperpars=dict(TOY_HYPER), lr=0.0, itnum=1,
                                    show_ELBO=False, device="cuda:0", pre_estimate=10)
    assert len(losses) == 1 and np.isfinite(losses[0])
    assert np.array_equal(model.mu_v.detach().cpu().numpy().reshape(-1), v)          # lr = 0: the initial state
    assert np.array_equal(model.mu_U_dense().detach().cpu().numpy(), want["mu_U"])
    assert float(model.sigma2_err_log) == want["sigma2_err_log"]
    # hyperpars wins over the estimate; given mu_v the estimator does not run
    hyp = dict(TOY_HYPER, sigma2_err_log=-2.0)
    model, _, _ = ND.inference(X_list, Y_list, g["z"], 200, 2, hyperpars=hyp, lr=0.0, itnum=1, show_ELBO=False,
                               device="cuda:0", pre_estimate=10)
    assert float(model.sigma2_err_log) == -2.0
    model, _, _ = ND.inference(X_list, Y_list, g["z"], 200, 2, hyperpars=hyp, mu_v=np.ones(20), lr=0.0, itnum=1,
                               show_ELBO=False, device="cuda:0", pre_estimate=10)
    assert np.array_equal(model.mu_v.detach().cpu().numpy().reshape(-1), np.ones(20))


def test_inference_without_the_keyword_is_unchanged():
    """The first-step loss of inference() equals the same step made by hand with NMGP + DsviTrainer on the same
    seed: the new keyword's default touches nothing."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import nmgp_dsvi as ND
    g, xs, ys = _toy_lists()
    X_list, Y_list = [x[:, None] for x in xs], [y[:, None] for y in ys]
    hyp = dict(TOY_HYPER, sigma2_err_log=-2.0)
    _, losses, _ = ND.inference(X_list, Y_list, g["z"], 200, 2, hyperpars=dict(hyp), lr=0.005, itnum=1,
                                show_ELBO=False, device="cuda:0")
    Xv, Yv = np.concatenate(X_list), np.concatenate(Y_list)
    Iv = np.concatenate([np.ones_like(Y_list[i]) * i for i in range(2)]).astype(int)
    X, Y, I = (torch.from_numpy(a).type(torch.DoubleTensor) for a in (Xv, Yv, Iv))
    model = ND.NMGP(number_observations=200, dim_outputs=2, Z=np.asarray(g["z"], np.float64), minibatch_size=200,
                    seed=22, device="cuda:0")
    ND._apply_hyperpars(model, dict(hyp), True, False, "model.pt", {})
    tr = ND.DsviTrainer(model, 0.005)
    idx = next(iter(ND._index_loader(200, 200, None)))
    X_bl, Y_bl = ND.vec2list(X[idx], Y[idx], I[idx], dim=2)
    x, y, sizes = model._prepare(X_bl, Y_bl)
    eng = model.engine(sum(sizes))
    nz = model._torch_noise(sum(sizes), 3)
    eng.load_batch(x, y, sizes, noise=nz)
    loss = tr.step(eng, noise=nz)
    torch.cuda.synchronize()
    assert float(loss) == float(losses[0])
