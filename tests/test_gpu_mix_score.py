"""Exact mixture scores on the MI355X: the kernels of csrc/mixscore.hip against the host references
(tests/_mix_ref.py) and the stored 40-digit values, and predict.score_mixture / impute_Y / summarize_Y with
mixture=True against the host reference run on the component buffers they return.

The gates are measured on the references, never on the kernel (tests/_mix_ref.py): with e64 the float64-vs-40-digit
error on the fixture entries of the very case, 16 max(e64, (S + 16) 2^-52 max(1, t1 + t2)) for crps and spread (t1
is not an output of its own: crps + spread is held to twice that gate against it), the same with 1 in place of
t1 + t2 for pit.  The fixture entries are compared with the 40-digit values, the others with the float64 host form.
A quantile is not compared in q (between separated components q is ill-conditioned): the CDF residual of the
returned q, evaluated by the host reference, must meet 4 (f(q) spacing(q) + (S + 16) 2^-52)."""
import numpy as np
import pytest
import torch

from tests import _mix_ref as MR

pytestmark = pytest.mark.gpu

F64 = torch.float64
SENTINEL = -7.0


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _score(Mu, Var, y=None, qs=MR.PS, e0=0, e1=None, embed=False, crps=True):
    """One mix_score_ call on the entries [e0, e1) -> dict of numpy arrays.  embed: Mu / Var as column ranges of
    wider NaN-filled buffers and every output inside a wider sentinel-filled one, checked untouched around it."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import hip_ops as H
    S, E_all = Mu.shape
    e1 = E_all if e1 is None else e1
    E = e1 - e0
    het = isinstance(Var, np.ndarray)
    yt = None if y is None else _t(y[e0:e1])
    out = None
    if embed:
        def wide(a):
            w = torch.full((S, E + 9), float("nan"), dtype=F64, device=_dev())
            w[:, 4:4 + E] = _t(a[:, e0:e1])
            return w[:, 4:4 + E]
        mu, var = wide(Mu), (wide(Var) if het else Var)
        assert mu.stride(0) == E + 9
        vec = {k: torch.full((E + 5,), SENTINEL, dtype=F64, device=_dev()) for k in ("pit", "crps", "spread")}
        qw = torch.full((len(qs), E + 6), SENTINEL, dtype=F64, device=_dev())
        out = {k: v[2:2 + E] for k, v in vec.items()}
        out["quantiles"] = qw[:, 3:3 + E]
    else:
        mu, var = _t(Mu[:, e0:e1]), (_t(Var[:, e0:e1]) if het else Var)
    got = H.mix_score_(mu, var, y=yt, qs=qs, crps=crps, out=out)
    torch.cuda.synchronize()
    if embed:
        for k, v in vec.items():
            assert (v[:2] == SENTINEL).all() and (v[2 + E:] == SENTINEL).all(), k
            assert got[k].data_ptr() == out[k].data_ptr()
        assert (qw[:, :3] == SENTINEL).all() and (qw[:, 3 + E:] == SENTINEL).all()
    return {k: v.cpu().numpy() for k, v in got.items()}


def _check_scores(got, c, E, what):
    ref, nf = c["ref"], min(c["nf"], E)
    want = {k: ref[k][:E].copy() for k in ("crps", "t1", "t2", "pit")}
    if c["gold"] is not None:
        for k in want:
            want[k][:nf] = c["gold"][k][:nf]
    g = c["gate"][:E]
    e = {"crps": np.abs(got["crps"] - want["crps"]), "spread": np.abs(got["spread"] - want["t2"]),
         "t1": np.abs(got["crps"] + got["spread"] - want["t1"]), "pit": np.abs(got["pit"] - want["pit"])}
    print(f"{what}: e64 {c['e64']:.2e} pit {c['e64_pit']:.2e}; " +
          " ".join(f"{k} {v.max():.2e}" for k, v in e.items()) +
          f" (gate {g.min():.2e}..{g.max():.2e}, pit {c['gate_pit']:.2e})")
    assert (e["crps"] <= g).all() and (e["spread"] <= g).all(), what
    assert (e["t1"] <= 2 * g).all() and (e["pit"] <= c["gate_pit"]).all(), what


def _check_quantiles(got, Mu, Var, S, qs, what):
    q = got["quantiles"]
    assert int(got["unconverged"][0]) == 0 and np.isfinite(q).all(), what
    worst = 0.0
    for k, p in enumerate(qs):
        res = np.abs(MR.cdf64(q[k][None], Mu, Var) - p)
        bound = MR.quantile_bound(q[k], Mu, Var, S)
        worst = max(worst, float((res / bound).max()))
        assert (res <= bound).all(), (what, p, float(res.max()))
    assert (np.diff(q, axis=0) >= 0.0).all()                             # qs ascend
    print(f"{what}: quantile residual / bound {worst:.2e}")


# ------------------------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize("het", [True, False], ids=["tensor", "scalar"])
@pytest.mark.parametrize("S", MR.S_LIST)
@pytest.mark.parametrize("kind", MR.KINDS)
def test_kernel_matches_the_references(kind, S, het):
    c = MR.case(kind, S, het)
    assert c["gold"] is not None
    for E in MR.E_LIST:
        V = c["Var"][:, :E] if het else c["Var"]
        got = _score(c["Mu"][:, :E], V, c["y"][:E])
        what = f"{kind} S={S} E={E} {'tensor' if het else 'scalar'}"
        _check_scores(got, c, E, what)
        _check_quantiles(got, c["Mu"][:, :E], V, S, MR.PS, what)


@pytest.mark.parametrize("het", [True, False], ids=["tensor", "scalar"])
def test_more_tile_pairs_than_slices(het):
    """S = 1300: 11 tiles, 66 tile pairs in 64 slices, so a slice walks two tile pairs and reloads its s tile.
    No 40-digit values at this size: the float64 host form under the gate's floor."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import _lib as L
    S, E = 1300, 3
    Mu, Var, y = MR.build("plain", S, E)
    V = Var if het else 0.37
    assert L.lib().nmgp_mix_score_workspace_size(S, E) == 64 * E * 8
    ref = MR.scores64(Mu, V, y)
    got = _score(Mu, V, y, qs=(0.5,))
    c = {"ref": ref, "nf": 0, "gold": None, "e64": 0.0, "e64_pit": 0.0,
         "gate": 16.0 * (S + 16) * MR.EPS * np.maximum(1.0, ref["t1"] + ref["t2"]),
         "gate_pit": 16.0 * (S + 16) * MR.EPS}
    _check_scores(got, c, E, f"S={S}")
    _check_quantiles(got, Mu, V, S, (0.5,), f"S={S}")


@pytest.mark.parametrize("het", [True, False], ids=["tensor", "scalar"])
@pytest.mark.parametrize("kind", MR.KINDS)
def test_column_ranges_of_wider_buffers_and_outputs_left_alone_around(kind, het):
    c = MR.case(kind, 129, het)
    a = _score(c["Mu"], c["Var"], c["y"], embed=True)
    b = _score(c["Mu"], c["Var"], c["y"])
    _check_scores(a, c, MR.E_MAX, f"embedded {kind}")
    for k in b:
        assert np.array_equal(a[k], b[k]), k


def test_workspace_size_and_optional_outputs():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import _lib as L
    from collaborative_nonstationary_multivariate_gaussian_process_amd import hip_ops as H
    size = L.lib().nmgp_mix_score_workspace_size
    assert size(1, 70) == 0 and size(2, 70) == 70 * 8 and size(129, 70) == 3 * 70 * 8 and size(257, 5) == 6 * 5 * 8
    assert H.mix_score_workspace(1, 70, _dev()) is None and H.mix_score_workspace(257, 5, _dev()).numel() == 240
    c = MR.case("plain", 65, True)
    full = _score(c["Mu"], c["Var"], c["y"])
    assert set(full) == {"pit", "crps", "spread", "quantiles", "unconverged"}
    no_y = _score(c["Mu"], c["Var"], None)
    assert set(no_y) == {"spread", "quantiles", "unconverged"}
    only = _score(c["Mu"], c["Var"], c["y"], qs=(), crps=False)
    assert set(only) == {"pit"}
    assert np.array_equal(no_y["spread"], full["spread"]) and np.array_equal(no_y["quantiles"], full["quantiles"])
    assert np.array_equal(only["pit"], full["pit"])
    # a caller's workspace is used as it is
    ws = H.mix_score_workspace(65, MR.E_MAX, _dev())
    again = H.mix_score_(_t(c["Mu"]), _t(c["Var"]), y=_t(c["y"]), ws=ws)
    assert np.array_equal(again["crps"].cpu().numpy(), full["crps"])


def test_argument_errors_raise_before_any_device_work():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import hip_ops as H
    Mu, Var, y = (torch.zeros(5, 3, dtype=F64, device=_dev()), torch.ones(5, 3, dtype=F64, device=_dev()),
                  torch.zeros(3, dtype=F64, device=_dev()))
    for args, kw in [((Mu, Var[:4]), {}), ((Mu, -1.0), {}), ((Mu, Var), {"y": y[:2]}), ((Mu, Var), {"qs": (1.0,)}),
                     ((Mu, Var), {"crps": False}), ((Mu, Var.cpu()), {}), ((Mu, Var), {"y": y.cpu()}),
                     ((Mu, Var), {"out": {"spread": torch.zeros(4, dtype=F64, device=_dev())}}),
                     ((Mu.cpu(), 1.0), {})]:
        with pytest.raises(ValueError):
            H.mix_score_(*args, **kw)


# ------------------------------------------------------------------------------------------------ NaN rules
@pytest.mark.parametrize("het", [True, False], ids=["tensor", "scalar"])
def test_a_bad_component_makes_only_its_entry_nan_and_a_nan_truth_only_pit_and_crps(het):
    c = MR.case("plain", 129, het)
    clean = _score(c["Mu"], c["Var"], c["y"])
    Mu, y = c["Mu"].copy(), c["y"].copy()
    Mu[128, 5] = np.nan                                                  # the last component: the second tile
    Mu[3, 17] = np.inf
    y[9] = np.nan
    y[10] = np.inf
    bad_e = [5, 17]
    Var = c["Var"]
    if het:
        Var = c["Var"].copy()
        Var[70, 30] = 0.0
        Var[0, 31] = -1.0
        Var[64, 32] = np.nan
        bad_e += [30, 31, 32]
    got = _score(Mu, Var, y)
    assert int(got["unconverged"][0]) == 0                               # a bad entry is not an unconverged one
    keep = np.ones(MR.E_MAX, bool)
    keep[bad_e] = False
    for k in ("pit", "crps", "spread"):
        assert np.isnan(got[k][bad_e]).all(), k
    assert np.isnan(got["quantiles"][:, bad_e]).all()
    for k in ("pit", "crps"):
        assert np.isnan(got[k][[9, 10]]).all()
        keep_y = keep.copy()
        keep_y[[9, 10]] = False
        assert np.array_equal(got[k][keep_y], clean[k][keep_y]), k
    assert np.array_equal(got["spread"][keep], clean["spread"][keep])
    assert np.array_equal(got["quantiles"][:, keep], clean["quantiles"][:, keep])


def test_no_entries_launch_nothing_and_return_empties():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    got = _score(np.zeros((7, 0)), np.ones((7, 0)), np.zeros(0))
    assert got["pit"].shape == got["crps"].shape == got["spread"].shape == (0,)
    assert got["quantiles"].shape == (len(MR.PS), 0) and int(got["unconverged"][0]) == 0
    out = predict.score_mixture(torch.zeros(7, 0, dtype=F64, device=_dev()), 0.5,
                                y=torch.zeros(0, dtype=F64, device=_dev()), quantiles=(0.5,))
    assert out["crps"].shape == (0,) and bool(torch.isnan(out["mean_crps"]))


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("het", [True, False], ids=["tensor", "scalar"])
@pytest.mark.parametrize("S", [65, 257])
def test_two_runs_and_two_batchings_give_the_same_bits(S, het):
    c = MR.case("plain", S, het)
    a, b = _score(c["Mu"], c["Var"], c["y"]), _score(c["Mu"], c["Var"], c["y"])
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    lo, hi = _score(c["Mu"], c["Var"], c["y"], e0=0, e1=35), _score(c["Mu"], c["Var"], c["y"], e0=35, e1=70)
    for k in ("pit", "crps", "spread", "quantiles"):
        assert np.array_equal(np.concatenate([lo[k], hi[k]], -1), a[k]), k


# ------------------------------------------------------------------------------------------------ API
def _floor_gate(ref, S):
    return 16.0 * (S + 16) * MR.EPS * np.maximum(1.0, ref["t1"] + ref["t2"])


def test_score_mixture_on_the_replicated_case_equals_the_single_gaussian():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    for het in (True, False):
        c = MR.case("replicated", 65, het)
        v = c["Var"][0] if het else c["Var"]
        out = predict.score_mixture(_t(c["Mu"]), _t(c["Var"]) if het else c["Var"], y=_t(c["y"]),
                                    quantiles=(0.025, 0.975))
        assert set(out) == {"pit", "crps", "mean_crps", "crps_spread", "quantiles", "unconverged"}
        want = MR.single_gaussian(c["Mu"][0], v, c["y"])
        g = 16.0 * (65 + 16) * MR.EPS * np.maximum(1.0, np.abs(want["crps"]) + 2 * want["t2"])
        get = lambda k: out[k].cpu().numpy()
        assert (np.abs(get("crps") - want["crps"]) <= g).all() and (np.abs(get("crps_spread") - want["t2"]) <= g).all()
        assert (np.abs(get("pit") - want["pit"]) <= 16.0 * (65 + 16) * MR.EPS).all()
        np.testing.assert_allclose(float(out["mean_crps"]), get("crps").mean(), rtol=1e-13)
        for k, p in enumerate((0.025, 0.975)):
            zp = float(torch.special.ndtri(torch.tensor(p, dtype=F64)))
            scale = np.abs(c["Mu"][0]) + abs(zp) * np.sqrt(v)
            assert (np.abs(get("quantiles")[k] - (c["Mu"][0] + zp * np.sqrt(v))) <= 1.01e-12 * scale).all()
        assert int(out["unconverged"]) == 0


MIX_KEYS = {"mixture_quantiles", "crps_spread", "mixture_unconverged"}


def _same_bits(a, b):
    """torch.equal on the bit patterns, so that a NaN (an unscored entry's lpd) equals itself."""
    if a.dtype == F64 and b.dtype == F64 and a.shape == b.shape:
        return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))
    return torch.equal(a, b)


def test_impute_Y_mixture_matches_the_host_reference_on_the_returned_components():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import nmgp_dsvi as NM
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    from tests.test_gpu_impute import _default_model, _grid
    D, M, N, S = 5, 20, 13, 40
    qs = (0.025, 0.5, 0.975)
    m = _default_model(D, M, N)
    x = torch.linspace(0.0, 1.0, N, dtype=F64)
    Y_obs, Y_true, miss = _grid(D, N)
    torch.manual_seed(7)
    base = predict.impute_Y(m, x, Y_obs, Y_true, n_sample=S, quantiles=qs, keep_samples=True)
    torch.manual_seed(7)
    out = predict.impute_Y(m, x, Y_obs, Y_true, n_sample=S, quantiles=qs, keep_samples=True, mixture=True)
    assert set(out) == set(base) | MIX_KEYS | {"pit", "crps", "mean_crps", "crps_per_output", "mixture_coverage"}
    for k, v in base.items():
        assert _same_bits(v, out[k]), k
    Mu, Var = out["Mu"].cpu().numpy(), out["Var"].cpu().numpy()
    E = Mu.shape[1]
    y = Y_true[miss]
    ok = np.isfinite(y)
    assert (~ok).sum() == 1
    ref = MR.scores64(Mu, Var, np.where(ok, y, 0.0))
    g = _floor_gate(ref, S)
    get = lambda k: out[k].cpu().numpy()
    e = {"crps": np.abs(get("crps") - ref["crps"])[ok], "spread": np.abs(get("crps_spread") - ref["t2"]),
         "pit": np.abs(get("pit") - ref["pit"])[ok]}
    print(f"impute_Y mixture E={E}: " + " ".join(f"{k} {v.max():.2e}" for k, v in e.items()) + f" (gate {g.min():.2e})")
    assert (e["crps"] <= g[ok]).all() and (e["spread"] <= g).all() and (e["pit"] <= 16.0 * (S + 16) * MR.EPS).all()
    assert np.isnan(get("crps")[~ok]).all() and np.isnan(get("pit")[~ok]).all()
    _check_quantiles({"quantiles": get("mixture_quantiles"), "unconverged": get("mixture_unconverged")}, Mu, Var, S, qs,
                     "impute_Y mixture")
    np.testing.assert_allclose(float(out["mean_crps"]), get("crps")[ok].mean(), rtol=1e-13)
    d_of = np.argwhere(miss)[:, 1]
    q64 = np.stack([MR.quantile64(Mu, Var, p)[0] for p in qs])
    inside = (y >= q64[0]) & (y <= q64[2])
    for d in range(D):
        sel = ok & (d_of == d)
        assert sel.any()
        assert abs(float(out["crps_per_output"][d]) - ref["crps"][sel].mean()) <= g[sel].max()
        np.testing.assert_allclose(float(out["mixture_coverage"][d]), inside[sel].mean(), rtol=1e-13)
    # fewer than two quantiles: the coverage is NaN; no truth: no truth-dependent key; numpy through the wrapper
    torch.manual_seed(7)
    one = predict.impute_Y(m, x, Y_obs, Y_true, n_sample=S, quantiles=(0.5,), mixture=True)
    assert bool(torch.isnan(one["mixture_coverage"]).all()) and one["mixture_quantiles"].shape == (1, E)
    torch.manual_seed(7)
    nm = NM.impute_Y(m, x.numpy(), Y_obs, n_sample=S, quantiles=qs, mixture=True)
    assert MIX_KEYS <= set(nm) and not {"pit", "crps", "mean_crps", "crps_per_output", "mixture_coverage"} & set(nm)
    assert all(isinstance(v, np.ndarray) for v in nm.values())
    assert nm["mixture_quantiles"].shape == (3, E) and nm["crps_spread"].shape == (E,)
    assert np.array_equal(nm["mixture_quantiles"], get("mixture_quantiles"))
    assert np.array_equal(nm["crps_spread"], get("crps_spread"))


def test_summarize_Y_mixture_matches_the_host_reference_on_the_returned_components():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import nmgp_dsvi as NM
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    from tests.test_gpu_impute import _default_model
    D, M, S = 5, 20, 40
    sizes, index = [9, 14], [1, 4]
    N = sum(sizes)
    qs = (0.025, 0.5, 0.975)
    m = _default_model(D, M, N)
    X = [torch.linspace(0.0, 1.0, n, dtype=F64) for n in sizes]
    rng = np.random.default_rng(17)
    y = rng.standard_normal(N)
    y[2] = np.nan
    Y = [torch.from_numpy(p.copy()) for p in np.split(y, np.cumsum(sizes)[:-1])]
    torch.manual_seed(5)
    base = predict.summarize_Y(m, X, Y, n_sample=S, index=index, quantiles=qs, keep_samples=True)
    torch.manual_seed(5)
    out = predict.summarize_Y(m, X, Y, n_sample=S, index=index, quantiles=qs, keep_samples=True, mixture=True)
    assert set(out) == set(base) | MIX_KEYS | {"pit", "crps", "mean_crps", "crps_per_entry", "mixture_coverage"}
    for k, v in base.items():
        assert _same_bits(v, out[k]), k
    Fs = out["Fs"].cpu().numpy()
    s2 = float(torch.exp(m.sigma2_err_log.detach().double())) + 1e-4
    ok = np.isfinite(y)
    ref = MR.scores64(Fs, s2, np.where(ok, y, 0.0))
    g = _floor_gate(ref, S)
    get = lambda k: out[k].cpu().numpy()
    e = {"crps": np.abs(get("crps") - ref["crps"])[ok], "spread": np.abs(get("crps_spread") - ref["t2"]),
         "pit": np.abs(get("pit") - ref["pit"])[ok]}
    print(f"summarize_Y mixture N={N}: " + " ".join(f"{k} {v.max():.2e}" for k, v in e.items()) +
          f" (gate {g.min():.2e})")
    assert (e["crps"] <= g[ok]).all() and (e["spread"] <= g).all() and (e["pit"] <= 16.0 * (S + 16) * MR.EPS).all()
    assert np.isnan(get("crps")[2]) and np.isnan(get("pit")[2])
    _check_quantiles({"quantiles": get("mixture_quantiles"), "unconverged": get("mixture_unconverged")}, Fs, s2, S, qs,
                     "summarize_Y mixture")
    q64 = np.stack([MR.quantile64(Fs, s2, p)[0] for p in qs])
    inside = (y >= q64[0]) & (y <= q64[2])
    off = np.concatenate([[0], np.cumsum(sizes)])
    for i in range(len(sizes)):
        sel = ok & (np.arange(N) >= off[i]) & (np.arange(N) < off[i + 1])
        assert abs(float(out["crps_per_entry"][i]) - ref["crps"][sel].mean()) <= g[sel].max()
        np.testing.assert_allclose(float(out["mixture_coverage"][i]), inside[sel].mean(), rtol=1e-13)
    torch.manual_seed(5)
    nm = NM.summarize_Y(m, [a.numpy() for a in X], n_sample=S, index=index, quantiles=qs, mixture=True)
    assert MIX_KEYS <= set(nm) and "crps" not in nm and all(isinstance(v, np.ndarray) for v in nm.values())
    assert np.array_equal(nm["mixture_quantiles"], get("mixture_quantiles"))
