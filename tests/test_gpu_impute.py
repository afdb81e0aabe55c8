"""Conditional prediction of missing outputs on the MI355X: the fused kernel (csrc/ycond.hip) against the host
references (tests/_impute_ref.py), and predict.impute_Y against the reference run on the host from the same pair
marginals, noise, mu_g and var_g.

The gates are measured on the references, never on the kernel (tests/_impute_ref.py): with e64 the float64 vs
longdouble error of either form on the very input, gate = 16 max(e64, (D + 16) 2^-52 max(1, max |ref|)) for a
collected mu or v, the same with D + S + 16 for sum / S, twice it for the second moments, four times for the
variance."""
import numpy as np
import pytest
import torch

from tests import _golden as G
from tests import _impute_ref as IR

pytestmark = pytest.mark.gpu

F64 = torch.float64
SENTINEL = -7.0
LD = np.longdouble


def _dev():
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ kernel
def _run(inp, s0=0, s1=None, out=None, embed=False, collect=False, ld=None, s_off=0, buf=None, y_true=None, lse=None):
    """One nmgp_ycond_accum_f64 call on samples [s0, s1) -> dict of device tensors."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import hip_ops as H
    dev = _dev()
    S_all, Q, N = inp["z_p"].shape
    D = inp["mu_g"].shape[2]
    s1 = S_all if s1 is None else s1
    S = s1 - s0
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if embed:          # noise in a wider block [junk 5][z_p Q N][junk 7]; pair rows N + 3 apart; NaN around
        zc = torch.full((S, 5 + Q * N + 7), float("nan"), dtype=F64, device=dev)
        zc[:, 5:5 + Q * N] = t(inp["z_p"][s0:s1]).reshape(S, Q * N)
        z_p = zc[:, 5:]
        wide = torch.full((2, Q, N + 3), float("nan"), dtype=F64, device=dev)
        wide[0, :, :N], wide[1, :, :N] = t(inp["pair_mu"]), t(inp["pair_sd"])
        pm, ps = wide[0, :, :N], wide[1, :, :N]
    else:
        z_p = t(inp["z_p"][s0:s1]).reshape(S, Q * N)
        pm, ps = t(inp["pair_mu"]), t(inp["pair_sd"])
    Y_obs = t(inp["Y_obs"])
    e_off, missing = H.missing_table(Y_obs)
    E = missing.shape[0]
    assert E == int(inp["missing"].sum())
    assert np.array_equal(missing.cpu().numpy(), np.argwhere(inp["missing"]))
    if out is None:
        out = tuple(torch.zeros(E, dtype=F64, device=dev) for _ in range(3))
    kw = {}
    if collect:
        if buf is None:
            rows = S if ld is None else ld
            buf = (torch.full((rows, E), SENTINEL, dtype=F64, device=dev),
                   torch.full((rows, E), SENTINEL, dtype=F64, device=dev))
        kw.update(Mu=buf[0], Var=buf[1], s_off=s_off)
    if y_true is not None:
        if lse is None:
            lse = (torch.full((E,), float("-inf"), dtype=F64, device=dev), torch.zeros(E, dtype=F64, device=dev))
        kw.update(y_true=t(y_true), lse_max=lse[0], lse_sum=lse[1])
    H.ycond_accum_(pm, ps, z_p, t(inp["mu_g"][s0:s1]), t(inp["var_g"][s0:s1]), Y_obs, inp["s2"], e_off, *out, **kw)
    torch.cuda.synchronize()
    return {"sums": out, "buf": buf, "lse": lse}


def _check_sums(sums_got, ref, what):
    S = ref["S"]
    got = [g.cpu().numpy()[ref["sel"]] for g in sums_got]
    want = IR.sums(ref)
    g = IR.gate(ref, S)
    e_mu = np.abs(got[0] - want[0]).max(initial=0.0) / S
    e_y2 = np.abs(got[1] - want[1]).max(initial=0.0) / S
    e_f2 = np.abs(got[2] - want[2]).max(initial=0.0) / S
    var = lambda a: a[1] / S - (a[0] / S) ** 2
    e_var = np.abs(var(got) - var(want)).max(initial=0.0)
    print(f"{what}: e64 {ref['e64']:.3e} scale {ref['scale']:.3g}; mu_sum {e_mu:.3e} y2 {e_y2:.3e} f2 {e_f2:.3e} "
          f"var {e_var:.3e} (gate {g:.3e})")
    assert all(np.isfinite(g_.cpu().numpy()).all() for g_ in sums_got)
    assert e_mu <= g, (what, e_mu, g)
    assert e_y2 <= 2 * g and e_f2 <= 2 * g, (what, e_y2, e_f2, 2 * g)
    assert e_var <= 4 * g, (what, e_var, 4 * g)


def _check_samples(buf, ref, what):
    mu, v = (b.cpu().numpy() for b in buf)
    g = IR.gate(ref)
    e_mu = np.abs(mu[:, ref["sel"]] - ref["Mu"]).max(initial=0.0)
    e_v = np.abs(v[:, ref["sel"]] - ref["Var"]).max(initial=0.0)
    print(f"{what}: collected mu {e_mu:.3e} v {e_v:.3e} (gate {g:.3e})")
    assert mu[:, ref["sel"]].shape == ref["Mu"].shape and np.isfinite(mu).all() and np.isfinite(v).all()
    assert e_mu <= g and e_v <= g, (what, e_mu, e_v, g)
    assert (v > IR.S2 * (1 - 1e-12)).all()


@pytest.mark.parametrize("kind", IR.MASKS)
@pytest.mark.parametrize("D,N,S", IR.GPU_SHAPES)
def test_kernel_matches_host_reference(D, N, S, kind):
    from collaborative_nonstationary_multivariate_gaussian_process_amd import _lib as L
    inp, ref = IR.case(D, N, S, kind)
    assert ref["forms"] <= IR.forms_bound(ref)                           # the two longdouble forms, on this very input
    assert (L.lib().nmgp_ycond_workspace_size(D, N, S) == 0) == ((D, N, S) in IR.UNSLICED or S == 1)
    got = _run(inp, collect=True)
    what = f"D={D} N={N} S={S} {kind}"
    _check_samples(got["buf"], ref, what)
    _check_sums(got["sums"], ref, what)


@pytest.mark.parametrize("kind", ["first", "last"])
def test_kernel_single_missing_output_in_the_first_and_last_tile(kind):
    D, N, S = 33, 9, 4
    inp, ref = IR.case(D, N, S, kind)
    assert ref["Mu"].shape == (S, N)
    got = _run(inp, collect=True)
    _check_samples(got["buf"], ref, f"D={D} only output {0 if kind == 'first' else D - 1} missing")
    _check_sums(got["sums"], ref, kind)


def test_collection_into_a_wider_buffer_leaves_the_rest_alone():
    D, N, S = 17, 70, 37
    inp, ref = IR.case(D, N, S)
    single = _run(inp, collect=True)["buf"]
    buf = _run(inp, 0, 20, collect=True, ld=S + 6, s_off=2)["buf"]
    for b in buf:
        assert (b[:2] == SENTINEL).all() and (b[22:] == SENTINEL).all()
    buf = _run(inp, 20, S, collect=True, buf=buf, s_off=22)["buf"]
    for b, one in zip(buf, single):
        assert (b[:2] == SENTINEL).all() and (b[2 + S:] == SENTINEL).all()
        assert torch.equal(b[2:2 + S], one)


@pytest.mark.parametrize("D,N,S,cut", [(17, 70, 37, 20), (17, 256, 3, 2)])
def test_two_calls_accumulate_to_the_single_call(D, N, S, cut):
    inp, ref = IR.case(D, N, S)
    single = _run(inp)["sums"]
    part = _run(inp, 0, cut)["sums"]
    part = _run(inp, cut, S, out=part)["sums"]
    _check_sums(part, ref, f"split {cut} + {S - cut}")
    g = IR.gate(ref, S)
    for k, (a, b) in enumerate(zip(part, single)):
        assert float((a - b).abs().max()) / S <= (1 if k == 0 else 2) * g


@pytest.mark.parametrize("D,N,S", [(17, 70, 37), (17, 256, 3), (128, 3, 5)])
def test_kernel_is_deterministic(D, N, S):
    inp, _ = IR.case(D, N, S)
    y = inp["Y_full"][inp["missing"]]
    a, b = _run(inp, collect=True, y_true=y), _run(inp, collect=True, y_true=y)
    for k in ("sums", "buf", "lse"):
        for x, z in zip(a[k], b[k]):
            assert torch.equal(x, z)


def test_kernel_reads_noise_inside_a_wider_block_and_strided_pair_rows():
    D, N, S = 17, 70, 37
    inp, ref = IR.case(D, N, S)
    a, b = _run(inp, collect=True, embed=True), _run(inp, collect=True)
    _check_sums(a["sums"], ref, "embedded")
    for k in ("sums", "buf"):
        for x, z in zip(a[k], b[k]):
            assert torch.equal(x, z)


@pytest.mark.parametrize("mu", [800.0, -800.0])
def test_non_finite_diagonal_makes_only_its_input_nan(mu):
    """exp(+-800) is inf / 0 on one diagonal of L at input 3: every entry of that input is NaN in every sample and
    in the sums, every other input has the bits of the clean run."""
    D, N, S = 17, 70, 37
    inp, ref = IR.case(D, N, S)
    bad = dict(inp)
    bad["pair_mu"] = inp["pair_mu"].copy()
    bad["pair_sd"] = inp["pair_sd"].copy()
    q = 5 * 6 // 2 + 5                                                   # the diagonal pair (5, 5)
    bad["pair_mu"][q, 3] = mu
    bad["pair_sd"][q, 3] = 0.0
    rows = np.argwhere(inp["missing"])[:, 0]
    assert (rows == 3).any()
    clean, got = _run(inp, collect=True), _run(bad, collect=True)
    at = torch.from_numpy(rows == 3).to(_dev())
    for k in ("sums", "buf"):
        for x, z in zip(got[k], clean[k]):
            assert torch.isnan(x[..., at]).all()
            assert torch.equal(x[..., ~at], z[..., ~at])


def test_non_positive_latent_variance_makes_only_its_input_nan():
    D, N, S = 17, 70, 37
    inp, ref = IR.case(D, N, S)
    bad = dict(inp)
    bad["var_g"] = inp["var_g"].copy()
    bad["var_g"][4, 3, 2] = -1.0
    rows = np.argwhere(inp["missing"])[:, 0]
    clean, got = _run(inp, collect=True), _run(bad, collect=True)
    at = torch.from_numpy(rows == 3).to(_dev())
    for x, z in zip(got["buf"], clean["buf"]):
        assert torch.isnan(x[4, at]).all() and torch.equal(x[:4], z[:4]) and torch.equal(x[5:], z[5:])
        assert torch.equal(x[4, ~at], z[4, ~at])
    for x, z in zip(got["sums"], clean["sums"]):
        assert torch.isnan(x[at]).all() and torch.equal(x[~at], z[~at])


@pytest.mark.parametrize("D,N,S", [(17, 70, 37), (17, 256, 3)])
def test_lse_state_matches_the_reference_and_skips_a_nan_truth(D, N, S):
    inp, ref = IR.case(D, N, S)
    y = inp["Y_full"][inp["missing"]].copy()
    y[1] = np.nan
    lse = (torch.full((y.size,), -3.0, dtype=F64, device=_dev()), torch.full((y.size,), 0.25, dtype=F64,
                                                                             device=_dev()))
    got = _run(inp, y_true=y, lse=lse)["lse"]
    m, r = (a.cpu().numpy() for a in got)
    assert m[1] == -3.0 and r[1] == 0.25                                # untouched
    ok = np.isfinite(y)
    ll = IR.log_density(y[None, ok].astype(LD), ref["MuL"][:, ok], ref["VarL"][:, ok])
    want = np.logaddexp(np.log(LD(0.25)) - 3, np.log(np.exp(ll - ll.max(0)).sum(0)) + ll.max(0))
    have = m[ok] + np.log(r[ok])
    g = IR.gate_lpd(y, ref, IR.gate(ref)) + (S + 16) * IR.EPS * max(1.0, float(np.abs(want).max()))
    e = float(np.abs(have - want.astype(np.float64)).max())
    print(f"lse D={D} N={N} S={S}: {e:.3e} (gate {g:.3e})")
    assert e <= g
    # a second chunk on the same state equals the state of both chunks in one call within the same gate
    cut = S // 2
    two = _run(inp, 0, cut, y_true=y)["lse"]
    two = _run(inp, cut, S, y_true=y, lse=two)["lse"]
    one = _run(inp, y_true=y)["lse"]
    a = (two[0] + torch.log(two[1])).cpu().numpy()[ok]
    b = (one[0] + torch.log(one[1])).cpu().numpy()[ok]
    assert np.abs(a - b).max() <= g
    assert two[0][1] == float("-inf") and two[1][1] == 0.0


def test_rows_without_a_missing_entry_do_no_work_and_e_zero_launches_nothing():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import hip_ops as H
    D, N, S = 17, 70, 37
    inp, _ = IR.case(D, N, S)
    full = dict(inp)
    full["missing"] = np.zeros_like(inp["missing"])
    full["Y_obs"] = inp["Y_full"]
    got = _run(full, collect=True)
    assert got["sums"][0].numel() == 0 and got["buf"][0].shape == (S, 0)


# ------------------------------------------------------------------------------------------------ API
def _model_from(g, D, M, N, **kw):
    from collaborative_nonstationary_multivariate_gaussian_process_amd.nmgp_dsvi import NMGP
    from oracle import nmgp_oracle as O
    m = NMGP(N, D, g["z"], **kw)
    with torch.no_grad():
        for k in O.PARAM_NAMES:
            if "p_" + k in g:
                getattr(m, k).data.copy_(torch.from_numpy(np.asarray(g["p_" + k])))
    return m


def _default_model(D, M, N):
    from collaborative_nonstationary_multivariate_gaussian_process_amd.nmgp_dsvi import NMGP
    return NMGP(N, D, np.linspace(0.0, 1.0, M))


def _grid(D, N, seed=13):
    """Y (N, D) ~ N(0, 1), the random mask recipe, and a truth with one NaN at a missing entry."""
    g = np.random.default_rng(seed)
    Y = g.standard_normal((N, D))
    miss = IR.make_mask(D, N, "random", seed)
    Y_true = Y.copy()
    n, d = np.argwhere(miss)[3]
    Y_true[n, d] = np.nan
    return np.where(miss, np.nan, Y), Y_true, miss


BASE_KEYS = {"missing", "mean", "sd", "F_mean", "F_sd", "Y_filled", "tilde_ell_mean"}
SCORE_KEYS = {"lpd", "mean_lpd", "rmse", "rmse_all", "coverage", "n_scored"}


@pytest.mark.parametrize("N", [13, 300])
def test_impute_Y_matches_the_host_reference_same_seed(N):
    """The pair marginals, the noise, mu_g and var_g of the very call, pulled through the helpers that impute_Y
    uses, and the longdouble reference run on them.  Gates: the kernel's for mean (sum / S) and for the variances
    (4 gates, compared as sd^2); for the quantiles a draw mu + sqrt(v) z moves by at most g (1 + |z| / (2 sqrt(s2)))
    under a perturbation g of mu and v (v >= s2), and the interpolated order statistics are 1-Lipschitz in the
    draws; for lpd the gate of _impute_ref.gate_lpd plus the rounding of S exponentials."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    D, M, S = 5, 20, 40
    qs = (0.025, 0.5, 0.975)
    m = _default_model(D, M, N)
    x = torch.linspace(0.0, 1.0, N, dtype=F64)
    Y_obs, Y_true, miss = _grid(D, N)
    torch.manual_seed(7)
    out = predict.impute_Y(m, x, Y_obs, Y_true, n_sample=S, quantiles=qs, keep_samples=True)
    assert set(out) == BASE_KEYS | SCORE_KEYS | {"quantiles", "Mu", "Var", "tilde_ells"}
    torch.manual_seed(7)
    ts = predict.sample_FY(m, x, S)[0]
    assert torch.equal(out["tilde_ells"], ts)                             # same code, same noise

    torch.manual_seed(7)
    st = predict._sampling_setup(m, x.reshape(-1, 1).to(m.device_).contiguous())
    Q = len(st["pairs"])
    per = M + N + Q * N + D * N + N * D
    assert predict._chunk_size(S, N, M) == S
    zc = predict._Draws(m.device_, None).take(S, per)
    T, mu_g, var_g, o_p, o_g, o_f = predict._sample_T_moments(st, zc)
    assert torch.equal(T, ts)
    s2 = st["s2_err"] + 1e-4
    inp = {"pair_mu": st["pair_mu"].cpu().numpy(), "pair_sd": st["pair_sd"].cpu().numpy(),
           "z_p": zc[:, o_p:o_p + Q * N].reshape(S, Q, N).cpu().numpy(), "mu_g": mu_g.cpu().numpy(),
           "var_g": var_g.transpose(1, 2).contiguous().cpu().numpy(), "s2": s2, "missing": miss, "Y_obs": Y_obs}
    ref = IR.reference(inp)
    mu, v = ref["MuL"], ref["VarL"]
    E = mu.shape[1]
    assert np.array_equal(out["missing"].cpu().numpy(), np.argwhere(miss)) and E == int(miss.sum())
    g1, gS = IR.gate(ref), IR.gate(ref, S)
    get = lambda k: out[k].cpu().numpy()
    e = {"Mu": np.abs(get("Mu") - ref["Mu"]).max(), "Var": np.abs(get("Var") - ref["Var"]).max()}
    mean = mu.mean(0)
    e["mean"] = np.abs(get("mean") - mean.astype(np.float64)).max()
    var_y = ((v + mu * mu).mean(0) - mean * mean).astype(np.float64)
    var_f = ((v - LD(s2) + mu * mu).mean(0) - mean * mean).astype(np.float64)
    e["sd^2"] = np.abs(get("sd") ** 2 - var_y).max()
    e["F_sd^2"] = np.abs(get("F_sd") ** 2 - var_f).max()
    z_f = zc[:, o_f:].reshape(S, N, D).cpu().numpy()[:, miss]
    want_q = np.quantile((mu + np.sqrt(v) * z_f).astype(np.float64), qs, axis=0)
    gq = g1 * (1 + np.abs(z_f).max() / (2 * np.sqrt(s2)))
    e["quantiles"] = np.abs(get("quantiles") - want_q).max()
    y = Y_true[miss]
    ok = np.isfinite(y)
    want_lpd = IR.lpd(y[ok].astype(LD), mu[:, ok], v[:, ok]).astype(np.float64)
    glpd = IR.gate_lpd(y, ref, g1) + (S + 16) * IR.EPS * max(1.0, float(np.abs(want_lpd).max()))
    e["lpd"] = np.abs(get("lpd")[ok] - want_lpd).max()
    print(f"N={N} E={E}: e64 {ref['e64']:.3e} " + " ".join(f"{k} {x_:.3e}" for k, x_ in e.items())
          + f" (gates: sample {g1:.3e} mean {gS:.3e} var {4 * gS:.3e} q {gq:.3e} lpd {glpd:.3e})")
    assert e["Mu"] <= g1 and e["Var"] <= g1 and e["mean"] <= gS
    assert e["sd^2"] <= 4 * gS and e["F_sd^2"] <= 4 * gS
    assert e["quantiles"] <= gq and e["lpd"] <= glpd
    assert np.isnan(get("lpd")[~ok]).all() and (~ok).sum() == 1
    assert torch.equal(out["F_mean"], out["mean"])
    # the scores against their definitions, from the returned means and bands
    d_of = np.argwhere(miss)[:, 1]
    gm, gq_ = get("mean"), get("quantiles")
    inside = (y >= gq_[0]) & (y <= gq_[2])
    for d in range(D):
        sel = ok & (d_of == d)
        assert int(out["n_scored"][d]) == sel.sum()
        if sel.any():
            np.testing.assert_allclose(float(out["rmse"][d]), np.sqrt(np.mean((gm[sel] - y[sel]) ** 2)), rtol=1e-13)
            np.testing.assert_allclose(float(out["coverage"][d]), inside[sel].mean(), rtol=1e-13)
    assert int(out["n_scored"].sum()) == ok.sum() >= D
    np.testing.assert_allclose(float(out["rmse_all"]), np.sqrt(np.mean((gm[ok] - y[ok]) ** 2)), rtol=1e-13)
    np.testing.assert_allclose(float(out["mean_lpd"]), get("lpd")[ok].mean(), rtol=1e-13)
    filled = get("Y_filled")
    assert np.array_equal(filled[~miss], Y_obs[~miss]) and np.array_equal(filled[miss], gm)


@pytest.mark.parametrize("tape", [True, False])
def test_impute_Y_does_not_depend_on_the_chunking(tape, monkeypatch):
    """Two chunks of 20 against one of 40.  A sample does not see its chunk: on a tape the samples' mu, v, the
    draws' quantiles and tilde_ell are the same bits; the means are sums of S terms in two orders and differ by at
    most 2 (S + 16) 2^-52 times the largest term, the variances by that of their two moments.  The Philox stream
    of _Draws is keyed by the chunk's position (a take is a stream of its own, include/nmgp_hip.h nmgp_normal_f64),
    so there the second chunk draws other noise than samples 20..39 of a single take, for every sampler of this
    module alike.  With Philox the check is therefore: the first chunk has the bits of the single take's first 20
    samples, tilde_ell has the bits of sample_FY under the same chunking, the quantiles are those of the draws
    rebuilt from the collected samples and the rebuilt noise bit for bit, and the sums over both chunks match the
    collected samples within the same tolerances."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    D, M, N, S = 5, 20, 13, 40
    m = _default_model(D, M, N)
    x = torch.linspace(0.0, 1.0, N, dtype=F64)
    Y_obs, Y_true, miss = _grid(D, N)
    per = M + N + D * (D + 1) // 2 * N + 2 * D * N
    noise = np.random.default_rng(5).standard_normal(S * per) if tape else None

    def run():
        torch.manual_seed(3)
        return predict.impute_Y(m, x, Y_obs, Y_true, n_sample=S, noise_tape=noise, keep_samples=True)

    one = run()
    monkeypatch.setattr(predict, "_chunk_size", lambda n_sample, N, M: 20)
    two = run()
    assert torch.equal(one["missing"], two["missing"])
    if tape:
        for k in ("Mu", "Var", "tilde_ells", "quantiles"):
            assert torch.equal(one[k], two[k]), k
        want = one
    else:
        for k in ("Mu", "Var", "tilde_ells"):
            assert torch.equal(one[k][:20], two[k][:20]), k
        torch.manual_seed(3)
        assert torch.equal(predict.sample_FY(m, x, S)[0], two["tilde_ells"])
        torch.manual_seed(3)
        predict._sampling_setup(m, x.reshape(-1, 1).to(m.device_).contiguous())
        draws = predict._Draws(m.device_, None)
        zc = torch.cat([draws.take(20, per), draws.take(20, per)])
        flat = two["missing"][:, 0] * D + two["missing"][:, 1]
        z_f = zc[:, per - N * D:].index_select(1, flat)
        Yd = two["Mu"] + torch.sqrt(two["Var"]) * z_f
        assert torch.equal(two["quantiles"], predict._quantiles_dim0(Yd, (0.025, 0.975)))
        mu_, v_ = two["Mu"], two["Var"]
        mean = mu_.mean(0)
        s2 = float(torch.exp(m.sigma2_err_log.detach().double())) + 1e-4
        want = {"mean": mean, "sd": torch.sqrt((v_ + mu_ * mu_).mean(0) - mean * mean),
                "F_sd": torch.sqrt(torch.clamp((v_ - s2 + mu_ * mu_).mean(0) - mean * mean, min=0.0))}
        y = torch.from_numpy(Y_true[miss]).to(mu_.device)
        ll = -0.5 * (torch.log(2 * np.pi * v_) + (y[None] - mu_) ** 2 / v_)
        want["lpd"] = torch.logsumexp(ll, 0) - np.log(S)
    mu, v = two["Mu"].cpu().numpy(), two["Var"].cpu().numpy()
    t1 = 2 * (S + 16) * IR.EPS * np.abs(mu).max()
    t2 = 2 * (S + 16) * IR.EPS * (v + mu * mu).max()
    tv = t2 + 2 * np.abs(mu).max() * t1
    d = lambda k, p=1: float((want[k] ** p - two[k] ** p).abs().max())
    print(f"tape={tape}: mean {d('mean'):.3e} (tol {t1:.3e}) sd^2 {d('sd', 2):.3e} F_sd^2 {d('F_sd', 2):.3e} "
          f"(tol {tv:.3e})")
    assert d("mean") <= t1 and d("sd", 2) <= tv and d("F_sd", 2) <= tv
    ok = torch.isfinite(two["lpd"])
    assert int(ok.sum()) == ok.numel() - 1
    tl = (S + 16) * IR.EPS * max(1.0, float(two["lpd"][ok].abs().max()))
    assert float((want["lpd"][ok] - two["lpd"][ok]).abs().max()) <= tl


def test_impute_Y_with_nothing_missing_has_no_entries():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    D, M, N, S = 5, 20, 13, 8
    m = _default_model(D, M, N)
    Y = np.random.default_rng(2).standard_normal((N, D))
    torch.manual_seed(1)
    out = predict.impute_Y(m, torch.linspace(0.0, 1.0, N, dtype=F64), Y, Y, n_sample=S)
    assert set(out) == BASE_KEYS | SCORE_KEYS | {"quantiles"}
    assert out["missing"].shape == (0, 2) and out["quantiles"].shape == (2, 0)
    for k in ("mean", "sd", "F_mean", "F_sd", "lpd"):
        assert out[k].shape == (0,), k
    assert np.array_equal(out["Y_filled"].cpu().numpy(), Y) and out["tilde_ell_mean"].shape == (N,)
    assert out["n_scored"].tolist() == [0] * D and torch.isnan(out["rmse"]).all()


def test_both_wrappers_key_sets_shapes_and_numpy_types():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import nmgp_dsvi as NM
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    D, M, N, S = 5, 20, 13, 16
    m = _default_model(D, M, N)
    x = np.linspace(0.0, 1.0, N)
    Y_obs, Y_true, miss = _grid(D, N)
    E = int(miss.sum())
    shapes = {"missing": (E, 2), "mean": (E,), "sd": (E,), "F_mean": (E,), "F_sd": (E,), "Y_filled": (N, D),
              "tilde_ell_mean": (N,), "quantiles": (3, E)}
    scores = {"lpd": (E,), "mean_lpd": (), "rmse": (D,), "rmse_all": (), "coverage": (D,), "n_scored": (D,)}
    torch.manual_seed(0)
    out = NM.impute_Y(m, x, Y_obs, n_sample=S, quantiles=(0.025, 0.5, 0.975))
    assert set(out) == set(shapes)
    for k, shp in shapes.items():
        assert isinstance(out[k], np.ndarray) and out[k].shape == shp, k
    assert np.isfinite(out["mean"]).all() and (out["sd"] >= out["F_sd"]).all() and (out["F_sd"] >= 0).all()
    assert (out["quantiles"][0] <= out["quantiles"][1]).all() and (out["quantiles"][1] <= out["quantiles"][2]).all()
    torch.manual_seed(0)
    sc = NM.impute_Y(m, x, Y_obs, Y_true, n_sample=S, quantiles=(0.025, 0.5, 0.975))
    assert set(sc) == set(shapes) | set(scores)
    for k, shp in scores.items():
        assert isinstance(sc[k], np.ndarray) and sc[k].shape == shp, k
    assert np.array_equal(sc["mean"], out["mean"])
    torch.manual_seed(0)
    dv = predict.impute_Y(m, torch.from_numpy(x), torch.from_numpy(Y_obs), n_sample=S, quantiles=())
    assert set(dv) == BASE_KEYS and all(torch.is_tensor(t) and t.is_cuda for t in dv.values())
    assert np.array_equal(dv["mean"].cpu().numpy(), out["mean"])
    torch.manual_seed(0)
    one = predict.impute_Y(m, torch.from_numpy(x), Y_obs, Y_true, n_sample=S, quantiles=(0.5,))
    assert set(one) == BASE_KEYS | (SCORE_KEYS - {"coverage"}) | {"quantiles"}


def test_impute_Y_never_holds_a_covariance_per_sample_and_input():
    """A cap, not a measurement: at D = 50, N = 64, S = 256 in one chunk, one missing output per row, the peak
    allocation grows by less than ONE (S, N, D, D) fp64 tensor (328 MB; the noise block is 180 MB)."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    D, M, N, S = 50, 20, 64, 256
    m = _default_model(D, M, N)
    g = np.random.default_rng(4)
    Y_obs = g.standard_normal((N, D))
    Y_obs[np.arange(N), g.integers(0, D, N)] = np.nan
    assert predict._chunk_size(S, N, M) == S
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    torch.manual_seed(3)
    out = predict.impute_Y(m, torch.linspace(0.0, 1.0, N, dtype=F64), Y_obs, n_sample=S)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    cap = S * N * D * D * 8
    print(f"peak allocation grew by {grown / 1e6:.1f} MB (cap {cap / 1e6:.1f} MB)")
    assert grown < cap
    assert out["mean"].shape == (N,) and all(bool(torch.isfinite(v).all()) for k, v in out.items() if k != "Y_filled")
    assert bool(torch.isfinite(out["Y_filled"]).all())


def test_unconditional_predictive_links_to_the_references_recorded_run():
    """All-NaN Y_obs on the reference's recorded noise (D = 2): under the model the recorded
    sum_s (fy_Ys[s, n, d] - Mu[s, e]) is exactly N(0, sum_s Var[s, e]), so the standardised sums of the 2 N entries
    must satisfy max |z| <= 5 (two-sided tail 5.7e-7 per entry).  tests/test_impute_reference.py checks on the
    host that the oracle's own mu and v keep the recorded run inside that bound (max |z| = 2.08)."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    g = G.load("sample_cases")
    S = int(g["n_sample"])
    m = _model_from(g, 2, 20, 200)
    N = g["xf"].shape[0]
    out = predict.impute_Y(m, torch.from_numpy(g["xf"]), np.full((N, 2), np.nan), n_sample=S,
                           noise_tape=g["noise_f"], keep_samples=True)
    assert out["Mu"].shape == (S, 2 * N)
    r = float((out["tilde_ells"].cpu() - torch.from_numpy(g["fy_tilde_ells"])).norm() / np.linalg.norm(g["fy_tilde_ells"]))
    assert r < 1e-7
    Ys = torch.from_numpy(g["fy_Ys"]).reshape(S, 2 * N)
    z = (Ys - out["Mu"].cpu()).sum(0) / out["Var"].cpu().sum(0).sqrt()
    print(f"golden link: max |z| {float(z.abs().max()):.3f}")
    assert float(z.abs().max()) <= 5.0
