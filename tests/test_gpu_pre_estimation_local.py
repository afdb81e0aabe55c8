"""The local coefficient factors on the MI355X: the factor kernel (csrc/prelocal.hip) and the window-data form of the
search (csrc/preest.hip) against the host reference (tests/_prelocal_ref.py) and the recorded runs of the reference's
objective (tests/golden/prelocal_cases.npz), then the Python surface (pre_nmgp.pre_estimate(cov_rows=...),
pre_estimation_local).  inference(pre_estimate={...}) is in tests/test_gpu_training_pre_estimation_local.py.

Bounds come from the reference side only.  B_m: the kernel sums the Pc products of an entry in some order, scales,
and adds alpha B with at most three more roundings, so |B^ - B*| <= gamma_{Pc+3} (w |Y_w|^T |Y_w| + alpha |B|) against
the long-double B*.  L: the kernel is a plain column Cholesky (every update uses the stored l_ij; no explicitly
inverted diagonal tile), so Higham's Theorem 10.3 applies as it stands: |L^ L^^T - B^| <= gamma_{D+1} |L^| |L^^T|,
products in long double, no condition-number factor.  The search: the gates of tests/test_gpu_pre_estimation.py."""
import os

import numpy as np
import pytest
import torch

from tests import _preest_ref as PR
from tests import _prelocal_ref as PL

pytestmark = pytest.mark.gpu

F64 = torch.float64
LD = np.longdouble
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prelocal_cases.npz")


def _dev():
    return torch.device("cuda:0")


def _H():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import hip_ops as H
    return H


def _PN():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import pre_nmgp as PN
    return PN


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _np(res):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _factor(est, z=None, **kw):
    pre = est["pre"]
    z = est["z"] if z is None else z
    return _np(_H().pre_local_factor_(_t(pre["x"]), _t(pre["Y"]), _t(pre["B"]), _t(z), est["P"], est["Pc"], est["w"],
                                      est["alpha"], est["holdout"], **kw))


def _check_B(got_B, B_ld, size, Pc, what):
    assert np.array_equal(got_B, got_B.T), what                         # symmetric bit for bit
    err = np.abs(np.asarray(got_B, LD) - B_ld)
    bound = LD(PL.gamma(Pc + 3)) * size
    worst = float(np.max(err / np.where(bound > 0, bound, 1)))
    print(f"{what}: worst |B^ - B*| / bound = {worst:.3f}")
    assert np.all(err <= bound), (what, worst)


def _check_L(Lh, Bh, what):
    D = Bh.shape[0]
    assert np.all(np.triu(Lh, 1) == 0.0) and np.all(np.diag(Lh) > 0.0), what
    Ll = np.asarray(Lh, LD)
    res = np.abs(Ll.dot(Ll.T) - np.asarray(Bh, LD))
    bound = LD(PL.gamma(D + 1)) * np.abs(Ll).dot(np.abs(Ll).T)
    worst = float(np.max(res / bound))
    print(f"{what}: worst |L L^T - B^| / (gamma_(D+1) |L||L^T|) = {worst:.3f}")
    assert np.all(res <= bound), (what, worst)


# ------------------------------------------------------------------------------------------- the factor kernel
@pytest.mark.parametrize("fx", PL.FIXTURES, ids=str)
def test_factor_kernel_against_host(fx):
    x, Y, z, est = PL.fixture(fx)
    N, D, M, P, Pc = fx[:5]
    got = _factor(est)
    assert not got["flags"].any()
    assert np.array_equal(got["neighbours"], np.stack(est["neighbours"]))
    assert np.array_equal(got["cov_neighbours"], np.stack(est["cov_neighbours"]))
    if not est["holdout"]:
        assert all(set(est["neighbours"][m]) <= set(est["cov_neighbours"][m]) for m in range(M))
    else:
        assert all(not set(est["neighbours"][m]) & set(est["cov_neighbours"][m]) for m in range(M))
    # the fit window is the window of today's kernel, bit for bit
    assert np.array_equal(got["neighbours"], np.stack([PR.neighbours(est["pre"]["x"], zm, P) for zm in z]))
    for m in range(M):
        idx = est["neighbours"][m]
        assert np.array_equal(got["xs"][m], est["pre"]["x"][idx]) and np.array_equal(got["Yloc"][m], est["pre"]["Y"][idx])
        _check_B(got["B_local"][m], est["B_ld"][m], est["B_size"][m], Pc, f"{fx} window {m}")
        _check_L(got["L"][m], got["B_local"][m], f"{fx} window {m}")


def test_factor_kernel_at_the_largest_windows():
    """P = 32 and Pc = 1024 with hold-out: all 1056 slots of the selection, 32 staging chunks, more rows than one pass
    of the scan (N = 1100 > 4 x 256)."""
    x, Y, z = PL.synth_local(1100, 3, 2, 9)
    est = PL.estimate_local(x, Y, z, 32, PL.MAX_COV_ROWS, holdout=True, search=False)
    got = _factor(est)
    assert not got["flags"].any()
    assert np.array_equal(got["neighbours"], np.stack(est["neighbours"]))
    assert np.array_equal(got["cov_neighbours"], np.stack(est["cov_neighbours"]))
    for m in range(2):
        _check_B(got["B_local"][m], est["B_ld"][m], est["B_size"][m], PL.MAX_COV_ROWS, f"largest window {m}")
        _check_L(got["L"][m], got["B_local"][m], f"largest window {m}")


# ------------------------------------------------------------------------------------------- the search on windows
def _search_windows(est):
    xs, Yr, mu = np.stack(est["xs"]), np.stack(est["Yrot_loc"]), np.stack(est["mu"])
    return _np(_H().pre_estimate_windows_(_t(xs), _t(Yr), _t(mu)))


def _check_search(got, est, what, bfgs_nll=None):
    """The checks of tests/test_gpu_pre_estimation.py::_check_search with every window's own mu."""
    M = len(est["nll"])
    assert np.array_equal(got["flags"], est["flags"].astype(np.int32)), (what, got["flags"], est["flags"])
    for m in range(M):
        xs, Yr, mu = est["xs"][m], est["Yrot_loc"][m], est["mu"][m]
        ls, le = float(est["log_s"][m]), float(est["log_ell"][m])
        gate = PR.eval_gate(xs, Yr, mu, ls, le)
        dn = abs(got["nll"][m] - est["nll"][m])
        box_h, box_g = np.asarray(est["box"][m]), got["box"][m]
        print(f"{what} window {m}: |dnll| {dn:.3e} gate {gate:.3e} d_ell {abs(got['log_ell'][m] - le):.3e} "
              f"d_s {abs(got['log_s'][m] - ls):.3e} flags {got['flags'][m]}")
        assert np.all(np.abs(box_g - box_h) <= 4 * np.spacing(np.abs(box_h))), (what, m, box_g, box_h)
        assert dn <= gate, (what, m, got["nll"][m], est["nll"][m], gate)
        if bfgs_nll is not None:
            assert got["nll"][m] <= bfgs_nll[m] + gate, (what, m, got["nll"][m], bfgs_nll[m])
        fl = int(est["flags"][m])
        if fl == 0:
            h_min = PR.fd_hessian_min_eig(xs, Yr, mu, ls, le)
            assert h_min > 0.0, (what, m, h_min)
            tol = np.sqrt(2 * gate / h_min) + 1e-8
            assert abs(got["log_ell"][m] - le) <= tol and abs(got["log_s"][m] - ls) <= tol, (what, m, tol)
        for bit, key, col in ((PR.FLAG_ELL_LO, "log_ell", 0), (PR.FLAG_ELL_HI, "log_ell", 1),
                              (PR.FLAG_S_LO, "log_s", 2), (PR.FLAG_S_HI, "log_s", 3)):
            if fl & bit:
                assert got[key][m] == box_g[col], (what, m, key)


@pytest.mark.parametrize("fx", PL.FIXTURES, ids=str)
def test_window_search_against_host(fx):
    x, Y, z, est = PL.fixture(fx)
    _check_search(_search_windows(est), est, str(fx))


def _check_loglik(est, pts, what):
    """pre_loglik_windows_ at pts (M, E, 2) against the long-double nll."""
    xs, Yr, mu = np.stack(est["xs"]), np.stack(est["Yrot_loc"]), np.stack(est["mu"])
    r = _np(_H().pre_loglik_windows_(_t(xs), _t(Yr), _t(mu), _t(pts)))
    assert not r["flags"].any()
    for m in range(pts.shape[0]):
        for e in range(pts.shape[1]):
            ls, le = pts[m, e]
            want = float(PR.nll(xs[m], Yr[m], mu[m], ls, le, PR.LD))
            gate = PR.eval_gate(xs[m], Yr[m], mu[m], ls, le)
            print(f"{what} window {m} point {e}: gpu {r['nll'][m, e]:.12f} ref {want:.12f} "
                  f"|d| {abs(r['nll'][m, e] - want):.3e} gate {gate:.3e}")
            assert abs(r["nll"][m, e] - want) <= gate, (what, m, e)


@pytest.mark.parametrize("fx", PL.FIXTURES, ids=str)
def test_window_evaluation_at_the_host_optimum(fx):
    x, Y, z, est = PL.fixture(fx)
    _check_loglik(est, np.stack([est["log_s"], est["log_ell"]], 1)[:, None, :], str(fx))


def _golden(name):
    c = PL.golden_cases(GOLDEN)[name]
    return c, PL.cached_estimate_local(("golden", name), c["x"], c["Y"], c["z"], c["P"], c["Pc"], holdout=True)


@pytest.mark.parametrize("name", ["local_a", "local_b"])
def test_window_evaluation_at_the_recorded_bfgs_points(name):
    c, est = _golden(name)
    pts = np.stack([np.stack([c["bfgs_log_s"], c["bfgs_log_ell"]], 1), np.stack([est["log_s"], est["log_ell"]], 1)], 1)
    _check_loglik(est, pts, name)


@pytest.mark.parametrize("name", ["local_a", "local_b"])
def test_golden_through_the_whole_path(name):
    """nll_gpu <= nll_bfgs + gate through pre_estimate(cov_rows=...), the device GEMM and eigensolver included."""
    c, est = _golden(name)
    full = _PN().pre_estimate(c["x"], c["Y"], c["z"], P=c["P"], cov_rows=c["Pc"], device="cuda:0")
    assert np.array_equal(full["neighbours"], np.stack(est["neighbours"]))
    assert np.array_equal(full["cov_neighbours"], np.stack(est["cov_neighbours"]))
    assert full["shrink"] == est["alpha"] and full["holdout"] is True
    for m in range(len(c["z"])):
        gate = PR.eval_gate(est["xs"][m], est["Yrot_loc"][m], est["mu"][m], est["log_s"][m], est["log_ell"][m])
        print(f"{name} window {m}: gpu {full['nll'][m]:.9f} host {est['nll'][m]:.9f} bfgs {c['bfgs_nll'][m]:.9f} "
              f"gate {gate:.3e}")
        assert full["nll"][m] <= c["bfgs_nll"][m] + gate, (name, m)
        assert abs(full["nll"][m] - est["nll"][m]) <= gate, (name, m)
        assert np.array_equal(full["L_tensor"][:, :, m], np.tril(full["L_tensor"][:, :, m]))
        Lh = est["L"][m]
        assert np.linalg.norm(full["L_tensor"][:, :, m] - Lh) / np.linalg.norm(Lh) < 1e-12


# ------------------------------------------------------------------------------------------- the window rule
def _rule_case(x, z, P, Pc, holdout, seed=0):
    rng = np.random.default_rng(seed)
    x = np.asarray(x, np.float64)
    Y = np.stack([np.sin(3 * x) + 0.1 * rng.standard_normal(x.size), np.cos(2 * x) + 0.1 * rng.standard_normal(x.size)], 1)
    return PL.estimate_local(x, Y, z, P, Pc, holdout=holdout, search=False)


@pytest.mark.parametrize("holdout", [True, False])
def test_windows_at_the_ends_on_a_data_point_and_with_ties(holdout):
    rng = np.random.default_rng(8)
    x = rng.permutation(np.linspace(0.0, 2.0, 41))                      # unsorted rows
    est = _rule_case(x, np.array([-5.0, 9.0, x[7]]), 6, 9, holdout)
    got = _factor(est)
    assert np.array_equal(got["neighbours"], np.stack(est["neighbours"]))
    assert np.array_equal(got["cov_neighbours"], np.stack(est["cov_neighbours"]))
    assert 7 in got["neighbours"][2]
    # rows 2 and 5 repeat the input 1.0; around z = 1 the distances tie in pairs.  P = 5: the last place of the fit
    # window is a tie between rows 1 and 6; Pc = 6 with hold-out (rows 6, 0, 7, 8, 13, then the tie 9 / 10 at distance 2)
    # and Pc = 9 without (the tie 8 / 13 at distance 1.5): the lower row wins each time
    x = np.array([0.25, 0.5, 1.0, 0.75, 1.25, 1.0, 1.5, 1.75, 2.5, 3.0, -1.0, 4.0, 5.0, -0.5])
    est = _rule_case(x, np.array([1.0]), 5, 6 if holdout else 9, holdout)
    assert est["neighbours"][0].tolist() == [1, 2, 3, 4, 5]
    assert est["cov_neighbours"][0].tolist() == ([0, 6, 7, 8, 9, 13] if holdout else [0, 1, 2, 3, 4, 5, 6, 7, 8])
    got = _factor(est)
    assert got["neighbours"][0].tolist() == est["neighbours"][0].tolist()
    assert got["cov_neighbours"][0].tolist() == est["cov_neighbours"][0].tolist()


def test_too_few_finite_inputs_are_degenerate():
    H = _H()
    x, Y, z = PL.synth_local(30, 2, 2, 4)
    x = x.copy()
    x[5:] = np.nan                                                      # five finite inputs, the windows want 3 + 4
    B = Y.T.dot(Y) / 29
    got = _np(H.pre_local_factor_(_t(x), _t(Y), _t(B), _t(z), 3, 4, 0.2, 0.4, True))
    assert (got["flags"] == H.PRE_FLAG_DEGENERATE).all() and (got["neighbours"] == -1).all()
    assert (got["cov_neighbours"] == -1).all() and np.isnan(got["L"]).all() and np.isnan(got["B_local"]).all()
    got = _np(H.pre_local_factor_(_t(x), _t(Y), _t(B), _t(z), 3, 5, 0.2, 0.4, False))
    assert not got["flags"].any() and got["cov_neighbours"].tolist() == [[0, 1, 2, 3, 4]] * 2


# ------------------------------------------------------------------------------------------- invariances
def _sign_case():
    x, Y, z = PL.sign_flip_case()
    return x, Y, z


@pytest.mark.parametrize("how", ["shrink_one", "all_rows"])
def test_global_matrix_is_recovered(how):
    """shrink = 1, and cov_rows = N without hold-out, both make B_m the global B: within the B bound against B itself
    (B on the device is Y^T Y / (N - 1) summed in another order: gamma_{N+2} |Y|^T |Y| / (N - 1) more), and the fit
    agrees with the global run within the gates."""
    PN = _PN()
    x, Y, z = _sign_case()
    N, D = Y.shape
    P = 10
    kw = dict(cov_rows=40, shrink=1.0) if how == "shrink_one" else dict(cov_rows=N, holdout=False)
    loc = PN.pre_estimate(x, Y, z, P=P, device="cuda:0", **kw)
    glob = PN.pre_estimate(x, Y, z, P=P, device="cuda:0")
    Pc = kw["cov_rows"]
    w, alpha = PL.weights(D, Pc, kw.get("shrink"))
    assert loc["shrink"] == alpha
    host = PR.cached_estimate("sign_flip", x, Y, z, P)
    absYY = np.abs(Y).T.dot(np.abs(Y))
    for m in range(len(z)):
        cov = loc["cov_neighbours"][m]
        size = w * np.abs(Y[cov]).T.dot(np.abs(Y[cov])) + alpha * np.abs(glob["B"])
        bound = PL.gamma(Pc + 3) * size + PL.gamma(N + 2) * absYY / (N - 1)
        assert np.all(np.abs(loc["B_local"][m] - glob["B"]) <= bound), (how, m)
        if how == "shrink_one":
            assert np.array_equal(loc["B_local"][m], glob["B"])
        idx = host["neighbours"][m]
        xs, Yr, mu = host["pre"]["x"][idx], host["pre"]["Yrot"][idx], host["pre"]["mu"]
        gate = PR.eval_gate(xs, Yr, mu, host["log_s"][m], host["log_ell"][m])
        print(f"{how} window {m}: local {loc['nll'][m]:.12f} global {glob['nll'][m]:.12f} gate {gate:.3e}")
        assert abs(loc["nll"][m] - glob["nll"][m]) <= gate, (how, m)
        assert loc["flags"][m] == glob["flags"][m] == 0
        tol = np.sqrt(2 * gate / PR.fd_hessian_min_eig(xs, Yr, mu, host["log_s"][m], host["log_ell"][m])) + 1e-8
        assert abs(loc["v_array"][m] - glob["v_array"][m]) <= tol, (how, m)
        assert abs(loc["sigma2_err_log_array"][m] - glob["sigma2_err_log_array"][m]) <= tol, (how, m)
    assert np.array_equal(loc["neighbours"], glob["neighbours"])


def test_cov_rows_none_is_todays_dict():
    PN = _PN()
    x, Y, z = _sign_case()
    a = PN.pre_estimate(x, Y, z, P=10, device="cuda:0")
    b = PN.pre_estimate(x, Y, z, 10, "cuda:0", None, 0.3, False)        # shrink / holdout are not read without cov_rows
    assert set(a) == {"v_array", "L_tensor", "sigma2_err_log_array", "nll", "flags", "neighbours", "B", "box"}
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    host = PR.cached_estimate("sign_flip", x, Y, z, 10)
    assert np.array_equal(a["neighbours"], np.stack(host["neighbours"]))
    for m in range(len(z)):
        assert np.array_equal(a["L_tensor"][:, :, m], a["L_tensor"][:, :, 0])


# ------------------------------------------------------------------------------------------- layout, determinism
def test_strided_inputs_untouched_surroundings_and_the_same_bits():
    H = _H()
    fx = PL.FIXTURES[5]                                                 # D = 17: two tiles a side, the second ragged
    x, Y, z, est = PL.fixture(fx)
    N, D, M, P, Pc = fx[:5]
    pre = est["pre"]
    plain, again = _factor(est), _factor(est)
    for k in plain:
        assert np.array_equal(plain[k], again[k]), k
    nan = float("nan")
    wide = torch.full((N, D + 3), nan, dtype=F64, device=_dev())
    wide[:, :D] = _t(pre["Y"])
    Bw = torch.full((D, D + 2), nan, dtype=F64, device=_dev())
    Bw[:, :D] = _t(pre["B"])
    xw = torch.full((3 * N,), nan, dtype=F64, device=_dev())
    xw[::3] = _t(pre["x"])
    zw = torch.full((2 * M,), nan, dtype=F64, device=_dev())
    zw[::2] = _t(z)
    shapes = {"B_local": (D, D), "L": (D, D), "xs": (P,), "Yloc": (P, D), "neighbours": (P,), "cov_neighbours": (Pc,),
              "flags": ()}
    bufs, out = {}, {}
    for k, sh in shapes.items():
        integer = k in ("neighbours", "cov_neighbours", "flags")
        bufs[k] = torch.full((M + 2,) + sh, -7 if integer else nan, dtype=torch.int32 if integer else F64, device=_dev())
        out[k] = bufs[k][1:M + 1]
    H.pre_local_factor_(xw[::3], wide[:, :D], Bw[:, :D], zw[::2], P, Pc, est["w"], est["alpha"], est["holdout"], out=out)
    torch.cuda.synchronize()
    for k in shapes:
        assert np.array_equal(out[k].cpu().numpy(), plain[k]), k
        for edge in (bufs[k][0], bufs[k][M + 1]):
            assert (edge == -7).all() if edge.dtype == torch.int32 else torch.isnan(edge).all(), k
    assert torch.isnan(wide[:, D:]).all() and torch.isnan(Bw[:, D:]).all() and torch.isnan(xw[1::3]).all()
    assert torch.isnan(zw[1::2]).all()
    # every window alone gives the bits it has in the whole launch
    for m in range(M):
        one = _factor(est, z=z[m:m + 1])
        for k in plain:
            assert np.array_equal(one[k][0], plain[k][m]), (k, m)
    # the search on windows: two launches, single-window launches, canaries
    xs, Yr, mu = _t(np.stack(est["xs"])), _t(np.stack(est["Yrot_loc"])), _t(np.stack(est["mu"]))
    a, b = _np(H.pre_estimate_windows_(xs, Yr, mu)), _np(H.pre_estimate_windows_(xs, Yr, mu))
    sb = {k: torch.full((M + 2,) + tuple(v.shape[1:]), -7 if v.dtype == np.int32 else nan,
                        dtype=torch.int32 if v.dtype == np.int32 else F64, device=_dev()) for k, v in a.items()}
    H.pre_estimate_windows_(xs, Yr, mu, out={k: v[1:M + 1] for k, v in sb.items()})
    torch.cuda.synchronize()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(sb[k][1:M + 1].cpu().numpy(), a[k]), k
        for edge in (sb[k][0], sb[k][M + 1]):
            assert (edge == -7).all() if edge.dtype == torch.int32 else torch.isnan(edge).all(), k
    ones = [H.pre_estimate_windows_(xs[m:m + 1], Yr[m:m + 1], mu[m:m + 1]) for m in range(M)]
    torch.cuda.synchronize()
    for k in a:
        assert np.array_equal(torch.cat([o[k] for o in ones]).cpu().numpy(), a[k]), k
    # the evaluation twin repeats the search's own last evaluation
    pars = _t(np.stack([a["log_s"], a["log_ell"]], 1)[:, None, :])
    r = _np(H.pre_loglik_windows_(xs, Yr, mu, pars))
    assert np.array_equal(r["nll"][:, 0], a["nll"])


# ------------------------------------------------------------------------------------------- the failure path
def _rank_case():
    """D = 6 outputs, Pc = D = 6 rows, shrink 0: the first output is exactly 0 on the left ten rows, so the left
    window's matrix has a zero first pivot; the right window's six rows span."""
    rng = np.random.default_rng(12)
    x = np.linspace(0.0, 1.0, 40)
    Y = rng.standard_normal((40, 6))
    Y[:10, 0] = 0.0
    return x, Y, np.array([0.05, 0.9])


def test_rank_deficient_window_is_flagged_and_the_other_is_finite():
    H, PN = _H(), _PN()
    x, Y, z = _rank_case()
    est = PL.estimate_local(x, Y, z, 3, 6, shrink=0.0, holdout=False, search=False)
    assert est["L"][0] is None and est["L"][1] is not None and np.all(np.diag(est["L"][1]) > 1e-3)
    got = _factor(est)
    assert got["flags"].tolist() == [H.PRE_FLAG_FACTOR, 0]
    assert np.isnan(got["L"][0]).all() and np.isfinite(got["L"][1]).all()
    _check_L(got["L"][1], got["B_local"][1], "spanning window")
    mu, V = H.syevj(_t(got["B_local"]))
    r = _np(H.pre_estimate_windows_(_t(got["xs"]), H.bmm(_t(got["Yloc"]), V), mu, flags=_t(got["flags"])))
    assert r["flags"][0] == H.PRE_FLAG_FACTOR and r["flags"][1] & (H.PRE_FLAG_FACTOR | H.PRE_FLAG_DEGENERATE) == 0
    assert np.isnan([r["log_ell"][0], r["log_s"][0], r["nll"][0]]).all()
    assert np.isfinite([r["log_ell"][1], r["log_s"][1], r["nll"][1]]).all()
    with pytest.raises(np.linalg.LinAlgError, match=r"z index \[0\]$"):
        PN.pre_estimate(x, Y, z, P=3, cov_rows=6, shrink=0.0, holdout=False, device="cuda:0")


def test_argument_errors_are_raised_before_any_launch():
    H, PN = _H(), _PN()
    from collaborative_nonstationary_multivariate_gaussian_process_amd import _lib as L
    x, Y, z = PL.synth_local(40, 2, 2, 4)
    B = Y.T.dot(Y) / 39
    xd, Yd, Bd, zd = _t(x), _t(Y), _t(B), _t(z)
    o = torch.zeros(4096, dtype=F64, device=_dev())
    # (P, Pc, holdout, alpha): Pc < P; Pc > 1024; P + Pc > N under hold-out; alpha outside [0, 1]
    for P, Pc, ho, alpha, word in ((10, 9, False, 0.5, "cov_rows"), (10, 1025, False, 0.5, "cov_rows"),
                                   (10, 31, True, 0.5, "rows"), (10, 20, True, -0.1, "alpha"),
                                   (10, 20, True, 1.5, "alpha"), (10, 20, True, float("nan"), "alpha")):
        with pytest.raises(ValueError, match=word):
            H.pre_local_factor_(xd, Yd, Bd, zd, P, Pc, 0.1, alpha, ho)
        rc = L.lib().nmgp_pre_local_factor_f64(L.ptr(xd), 1, L.ptr(Yd), 2, L.ptr(Bd), 2, L.ptr(zd), 1, 40, 2, 2, P, Pc,
                                               int(ho), 0.1, alpha, L.ptr(o), L.ptr(o), L.ptr(o), L.ptr(o), L.ptr(o),
                                               L.ptr(o), L.ptr(o), L.stream_handle())
        assert rc == -69, (P, Pc, ho, alpha)
    torch.cuda.synchronize()
    assert (o == 0).all()                                               # nothing was launched
    assert H.pre_local_factor_(xd, Yd, Bd, zd, 10, 30, 0.1, 0.5, True)["flags"].shape == (2,)   # P + Pc = N is allowed
    for kw, word in ((dict(cov_rows=9), "cov_rows"), (dict(cov_rows=1025), "cov_rows"), (dict(cov_rows=31), "rows"),
                     (dict(cov_rows=20, shrink=1.5), "shrink"), (dict(cov_rows=20, shrink=-0.1), "shrink")):
        with pytest.raises(ValueError, match=word):
            PN.pre_estimate(x, Y, z, P=10, device="cuda:0", **kw)


# ------------------------------------------------------------------------------------------- the Python surface
def test_pre_estimation_local_surface():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import nmgp_dsvi as ND
    PN = _PN()
    assert ND.pre_estimation_local is PN.pre_estimation_local
    x, Y, z = _sign_case()
    M, D = len(z), Y.shape[1]
    # NaN rows are dropped first, as in pre_estimation_partial
    x2 = np.concatenate([x, [0.31, 0.32]])
    Y2 = np.concatenate([Y, np.full((2, D), np.nan)])
    o = np.argsort(x2, kind="stable")
    v, Lt, s = PN.pre_estimation_local(x2[o], Y2[o], z, P=10, cov_rows=40, device="cuda:0")
    assert v.shape == (M,) and Lt.shape == (D, D, M) and s.shape == (M,)
    assert v.dtype == np.float64 and Lt.dtype == np.float64 and s.dtype == np.float64
    full = PN.pre_estimate(x, Y, z, P=10, cov_rows=40, device="cuda:0")
    assert np.array_equal(full["v_array"], v) and np.array_equal(full["L_tensor"], Lt)
    assert set(full) >= {"B_local", "cov_neighbours", "shrink", "holdout", "L_tensor", "nll", "flags", "neighbours"}
    assert not np.array_equal(Lt[:, :, 0], Lt[:, :, -1])
    corr = [b[0, 1] / np.sqrt(b[0, 0] * b[1, 1]) for b in full["B_local"]]
    assert corr[0] > 0.5 and corr[-1] < -0.5 and abs(full["B"][0, 1] / np.sqrt(full["B"][0, 0] * full["B"][1, 1])) < 0.5
    init = ND.init_from_pre_estimation(v, Lt, s)
    assert init["mu_U"].shape == (D, D, M) and np.isfinite(init["mu_U"]).all()
    assert not np.array_equal(init["mu_U"][:, :, 0], init["mu_U"][:, :, -1])
