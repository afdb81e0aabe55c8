"""The host references of the fused conditional prediction (tests/_impute_ref.py) pinned to each other and to
closed forms, the host logic of predict.observed_grid and the argument checks of predict.impute_Y and of the C ABI
that need no device."""
import ctypes

import numpy as np
import pytest

from tests import _impute_ref as IR

LD = IR.LD
ERR_YCOND_ARG = -65         # include/nmgp_hip.h NMGP_ERR_YCOND_ARG

PIN = [(D, N, S, k) for (D, N, S) in IR.GPU_SHAPES for k in IR.MASKS]


@pytest.mark.parametrize("D,N,S,kind", PIN + [(33, 9, 4, "first"), (33, 9, 4, "last")])
def test_the_two_longdouble_forms_agree(D, N, S, kind):
    inp, ref = IR.case(D, N, S, kind)
    bound = IR.forms_bound(ref)
    print(f"D={D} N={N} S={S} {kind}: forms {ref['forms']:.3e} (bound {bound:.3e}) e64 {ref['e64']:.3e} "
          f"gate {IR.gate(ref):.3e}")
    assert ref["forms"] <= bound
    E = int(inp["missing"].sum())
    assert ref["Mu"].shape == (S, ref["sel"].size) and np.isfinite(ref["Mu"]).all()
    rows = IR.rows_checked(D, N)
    if rows is None:
        assert np.array_equal(ref["sel"], np.arange(E))
    else:
        assert set(rows % 8) == set(range(8)) and {0, 1, 2} <= set(rows)
        assert np.array_equal(np.argwhere(inp["missing"])[ref["sel"], 0], np.repeat(rows, inp["missing"][rows].sum(1)))
    assert (ref["Var"] > IR.S2).all()


def _tiny(D, N, S, missing, seed=5):
    g = np.random.default_rng(seed)
    Q = D * (D + 1) // 2
    inp = {"pair_mu": 0.5 * g.standard_normal((Q, N)), "pair_sd": g.uniform(0.05, 0.5, (Q, N)),
           "z_p": g.standard_normal((S, Q, N)), "mu_g": g.standard_normal((S, N, D)),
           "var_g": g.uniform(0.01, 1.0, (S, N, D)), "s2": IR.S2, "missing": missing}
    Y = g.standard_normal((N, D))
    inp["Y_obs"] = np.where(missing, np.nan, Y)
    return inp


def test_D1_closed_form():
    """Nothing to condition on: mu = L mu_g, v = L^2 V + s2."""
    N, S = 4, 3
    inp = _tiny(1, N, S, np.ones((N, 1), bool))
    ref = IR.reference(inp)
    L = np.exp(inp["pair_mu"][None, 0] + inp["pair_sd"][None, 0] * inp["z_p"][:, 0])          # (S, N)
    V = inp["var_g"][:, :, 0] + IR.JIT
    np.testing.assert_allclose(ref["Mu"], L * inp["mu_g"][:, :, 0], rtol=1e-14, atol=0)
    np.testing.assert_allclose(ref["Var"], L * L * V + IR.S2, rtol=1e-14, atol=0)


def test_D2_closed_form_with_output_0_observed():
    N, S = 5, 4
    miss = np.zeros((N, 2), bool)
    miss[:, 1] = True
    inp = _tiny(2, N, S, miss)
    ref = IR.reference(inp)
    l = inp["pair_mu"][None] + inp["pair_sd"][None] * inp["z_p"]                               # (S, 3, N)
    a, b, c = np.exp(l[:, 0]), l[:, 1], np.exp(l[:, 2])
    V = inp["var_g"] + IR.JIT
    m = inp["mu_g"]
    c00 = a * a * V[..., 0] + IR.S2
    c10 = a * b * V[..., 0]
    c11 = b * b * V[..., 0] + c * c * V[..., 1] + IR.S2
    y0 = inp["Y_obs"][None, :, 0]
    mu = b * m[..., 0] + c * m[..., 1] + c10 / c00 * (y0 - a * m[..., 0])
    v = c11 - c10 * c10 / c00
    np.testing.assert_allclose(ref["Mu"], mu, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(ref["Var"], v, rtol=1e-12, atol=0)


def test_conditioning_never_raises_the_variance():
    """Per sample: v given the observed outputs <= v given none, and observing more outputs never raises v."""
    D, N, S = 9, 6, 5
    g = np.random.default_rng(3)
    base = np.zeros((N, D), bool)
    base[:, [2, 7]] = True                                               # the entries compared: always missing
    some = base | (g.random((N, D)) < 0.5)
    most = np.ones((N, D), bool)
    inp = _tiny(D, N, S, base)
    v = {}
    for name, miss in (("few missing", base), ("some", some), ("all", most)):
        cur = dict(inp)
        cur["missing"] = miss
        cur["Y_obs"] = np.where(miss, np.nan, np.nan_to_num(inp["Y_obs"], nan=0.3))
        var = IR._latent(cur, LD)[1]
        v[name] = var[:, base]
    tol = 64 * IR.EPS * float(v["all"].max())
    assert (v["few missing"] <= v["some"] + tol).all() and (v["some"] <= v["all"] + tol).all()
    assert (v["few missing"] < v["all"]).any()


@pytest.mark.parametrize("kind", IR.MASKS)
@pytest.mark.parametrize("D,N", [(1, 1), (2, 11), (17, 70), (128, 3)])
def test_every_mask_recipe_contains_the_special_rows(D, N, kind):
    miss = IR.make_mask(D, N, kind, 1)
    assert miss.shape == (N, D) and miss[0].all()
    if N >= 3:
        assert not miss[1].any() and (~miss[2]).sum() == 1
    rest = miss[3:] if N >= 3 else miss[1:]
    if kind == "one_missing":
        assert (rest.sum(1) == 1).all()
    if kind == "one_observed":
        assert ((~rest).sum(1) == 1).all()
    if kind == "random" and rest.size > 100:
        assert 0.2 < rest.mean() < 0.4
    for k, d in (("first", 0), ("last", D - 1)):
        only = IR.make_mask(D, N, k, 1)
        assert (only.sum(1) == 1).all() and only[:, d].all()


def test_observed_grid_on_unsorted_duplicated_and_absent_inputs():
    from collaborative_nonstationary_multivariate_gaussian_process_amd.predict import observed_grid
    x = np.array([0.5, 0.1, 0.9, 0.3])
    X = [np.array([0.9, 0.1, 0.5, 0.1]), np.array([0.3]), np.array([]), np.array([[0.5], [0.3000000001]])]
    Y = [np.array([9.0, 1.0, 5.0, -1.0]), np.array([3.0]), np.array([]), np.array([[50.0], [30.0]])]
    got = observed_grid(X, Y, x)
    nan = np.nan
    want = np.array([[5.0, nan, nan, 50.0], [1.0, nan, nan, nan], [9.0, nan, nan, nan], [nan, 3.0, nan, nan]])
    assert got.shape == (4, 4) and got.dtype == np.float64
    np.testing.assert_array_equal(got, want)                             # the first of the two 0.1 wins
    with pytest.raises(ValueError):
        observed_grid(X, Y[:3], x)
    with pytest.raises(ValueError):
        observed_grid([np.zeros(3)], [np.zeros(2)], x)


def test_impute_Y_checks_its_arguments_before_any_device_work():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict

    class Stub:                                                          # nothing past the checks touches the model
        D = 3

    x = np.linspace(0, 1, 4)
    ok = np.full((4, 3), np.nan)
    for bad in (np.zeros((4, 2)), np.zeros(12), np.zeros((4, 3, 1))):
        with pytest.raises(ValueError, match="Y_obs"):
            predict.impute_Y(Stub(), x, bad)
    with pytest.raises(ValueError, match="n_sample"):
        predict.impute_Y(Stub(), x, ok, n_sample=0)
    with pytest.raises(ValueError, match="quantiles"):
        predict.impute_Y(Stub(), x, ok, quantiles=(0.025, 1.5))
    with pytest.raises(ValueError, match="Y_true"):
        predict.impute_Y(Stub(), x, ok, Y_true=np.zeros((3, 3)))


def _call(lib, **kw):
    a = dict(D=5, N=4, S=3, E=6, ld_pair=4, z_stride=1 << 20, s2=0.01, ld=8, s_off=0, ws_bytes=None)
    ptrs = dict.fromkeys(["pair_mu", "pair_sd", "z_p", "mu_g", "var_g", "Y_obs", "e_off", "mu_sum", "y2_sum", "f2_sum",
                          "y_true", "lse_max", "lse_sum", "Mu", "Var", "ws"], 0x1000)
    for k, v in kw.items():
        (ptrs if k in ptrs else a)[k] = v
    p = lambda k: None if ptrs[k] is None else ctypes.c_void_p(ptrs[k])
    if a["ws_bytes"] is None:
        a["ws_bytes"] = lib.nmgp_ycond_workspace_size(a["D"], a["N"], a["S"])
    return lib.nmgp_ycond_accum_f64(p("pair_mu"), p("pair_sd"), a["ld_pair"], p("z_p"), a["z_stride"], p("mu_g"),
                                    p("var_g"), p("Y_obs"), a["s2"], a["D"], a["N"], a["S"], p("e_off"), a["E"],
                                    p("mu_sum"), p("y2_sum"), p("f2_sum"), p("y_true"), p("lse_max"), p("lse_sum"),
                                    p("Mu"), p("Var"), a["ld"], a["s_off"], p("ws"), a["ws_bytes"], None)


def test_ycond_accum_refuses_bad_arguments_before_launch():
    """Every case of the header's list returns NMGP_ERR_YCOND_ARG, S = 0, N = 0 or E = 0 returns 0; nothing is
    launched in either case (the pointers are not dereferenced on the host)."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import _lib as L
    lib = L.lib()
    for D in (0, 129, -1):
        assert _call(lib, D=D) == ERR_YCOND_ARG
    for k in ("N", "S", "E", "s_off"):
        assert _call(lib, **{k: -1}) == ERR_YCOND_ARG, k
    assert _call(lib, E=21) == ERR_YCOND_ARG                             # more entries than N D
    assert _call(lib, ld_pair=3) == ERR_YCOND_ARG
    assert _call(lib, z_stride=-1) == ERR_YCOND_ARG
    for s2 in (0.0, -1.0, float("nan")):
        assert _call(lib, s2=s2) == ERR_YCOND_ARG
    for k in ("pair_mu", "pair_sd", "z_p", "mu_g", "var_g", "Y_obs", "e_off", "mu_sum", "y2_sum", "f2_sum"):
        assert _call(lib, **{k: None}) == ERR_YCOND_ARG, k
    assert _call(lib, Mu=None) == ERR_YCOND_ARG and _call(lib, Var=None) == ERR_YCOND_ARG
    assert _call(lib, ld=2) == ERR_YCOND_ARG and _call(lib, s_off=6, ld=8) == ERR_YCOND_ARG
    assert _call(lib, lse_max=None) == ERR_YCOND_ARG and _call(lib, lse_sum=None) == ERR_YCOND_ARG
    assert _call(lib, ws=None) == ERR_YCOND_ARG
    assert _call(lib, ws_bytes=lib.nmgp_ycond_workspace_size(5, 4, 3) - 1) == ERR_YCOND_ARG
    assert _call(lib, N=0, E=0) == 0 and _call(lib, S=0) == 0 and _call(lib, E=0) == 0
    assert lib.nmgp_ycond_workspace_size(5, 4, 3) > 0
    assert lib.nmgp_ycond_workspace_size(5, 256, 3) == 0 and lib.nmgp_ycond_workspace_size(5, 4, 1) == 0
    assert lib.nmgp_ycond_workspace_size(0, 4, 3) == 0 and lib.nmgp_ycond_workspace_size(129, 4, 3) == 0


def test_the_oracles_own_moments_keep_the_recorded_run_inside_the_link_bound():
    """The premise of tests/test_gpu_impute.py's link to the recorded run (tests/golden/sample_cases.npz, D = 2):
    with the oracle's sampling core on the recorded tape, mu = L mu_g and v = diag(L V L^T) + s2 per sample, the
    standardised sums sum_s (fy_Ys - mu) / sqrt(sum_s v) of the 2 N entries stay within 5."""
    import torch
    from oracle import nmgp_oracle as O
    from tests import _golden as G
    g = G.load("sample_cases")
    p = {k: torch.as_tensor(np.asarray(g["p_" + k])) for k in O.PARAM_NAMES if "p_" + k in g}
    S = int(g["n_sample"])
    noise = O.TapeNoise(g["noise_f"])
    D, M = p["mu_W"].shape
    inputs = torch.as_tensor(g["xf"]).reshape(-1, 1)
    Z = torch.as_tensor(g["z"]).reshape(-1, 1)
    SW, Sv, SU = O._covs(p)
    h = O._hyper(p)
    N = inputs.shape[0]
    num = den = 0.0
    for s in range(S):
        c = O._sample_core(p, Sv, SU, h, Z, inputs, D, noise, N)
        K12 = O.create_Gibbs(inputs, Z, c["ell_X"], c["ell_Z"])
        K22 = O.create_Gibbs(Z, Z, c["ell_Z"], c["ell_Z"])
        mu_g, s2_g = O.MGP_mu_sigma2(K12, K22, torch.ones(N, dtype=torch.float64), p["mu_W"], SW)
        noise(D * N), noise(N * D)                                       # z_g and z_f of the sample
        Ln = c["L"].permute(2, 0, 1)
        mu = torch.matmul(Ln, mu_g.permute(1, 0).unsqueeze(2))[:, :, 0]
        v = (Ln ** 2 * (s2_g.permute(1, 0) + 1e-4).unsqueeze(1)).sum(2) + h["s2_err"] + 1e-4
        num = num + (torch.as_tensor(g["fy_Ys"][s]) - mu)
        den = den + v
    assert noise.done()
    z = num / den.sqrt()
    print(f"oracle moments on the recorded run: max |z| {float(z.abs().max()):.3f}")
    assert float(z.abs().max()) <= 5.0
