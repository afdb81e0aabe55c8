"""The pre-estimation on the MI355X: the two kernel entries (csrc/preest.hip) against the host reference
(tests/_preest_ref.py) and the recorded reference runs (tests/golden/preest_cases.npz), then the Python surface
(pre_nmgp.py, nmgp_dsvi.pre_estimation).  inference(pre_estimate=...) is in
tests/test_gpu_training_pre_estimation.py.

Gates come from the reference side only: the evaluation gate c (P + D) 2^-52 sum_pd(|log G| + E / G) with c from
the float64-vs-long-double error of the host restatement (tests/test_preest_reference.py); for the location of an
interior optimum sqrt(2 gate / h_min) + 1e-8 with h_min the smaller eigenvalue of the host's finite-difference
Hessian (an nll error of `gate` moves the minimum of a quadratic bowl of curvature h_min by at most that); box ends
within 4 ulp of the host's (one log and two roundings each side), the answer on an edge bitwise equal to the
kernel's own box end."""
import os

import numpy as np
import pytest
import torch

from tests import _preest_ref as PR

pytestmark = pytest.mark.gpu

F64 = torch.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "preest_cases.npz")
# (N, D, M, P): two outputs; one output and the smallest window; D odd; the LDS maximum; P = N
SHAPES = [(40, 2, 3, 10), (40, 1, 1, 3), (64, 5, 4, 10), (160, 128, 2, 32), (32, 7, 2, 32)]


def _dev():
    return torch.device("cuda:0")


def _H():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import hip_ops as H
    return H


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _synth(N, D, M, seed):
    """Outputs sharing three latent waves whose frequency grows along [0, 1], plus noise; z inside the range.  The
    noise (sd 0.5) is large enough that a window of 3 points of one output is not interpolated: with less, its
    optimum runs to the lower s edge, where G = lam mu + s is the rounding of lam and the float64 restatement itself
    leaves the evaluation gate (30 to 74 units measured at sd 0.15, against c = 10.1)."""
    rng = np.random.default_rng(seed)
    u = np.sort(rng.uniform(0.0, 1.0, N))
    warp = u + 1.5 * u * u
    lat = np.stack([np.sin(2 * np.pi * (k + 1.5) * warp + rng.uniform(0, 2 * np.pi)) for k in range(3)], axis=1)
    Y = lat.dot(rng.standard_normal((3, D))) + 0.5 * rng.standard_normal((N, D))
    return u, Y, np.linspace(0.1, 0.9, M)


_SHAPE_CACHE = {}


def _shape_case(shape):
    """Data and host estimate of one synthetic shape, computed once."""
    if shape not in _SHAPE_CACHE:
        N, D, M, P = shape
        x, Y, z = _synth(N, D, M, 100 + N + D)
        _SHAPE_CACHE[shape] = (x, Y, z, PR.cached_estimate(("shape",) + shape, x, Y, z, P))
    return _SHAPE_CACHE[shape]


def _search(pre, z, P, **kw):
    r = _H().pre_estimate_(_t(pre["x"]), _t(pre["Yrot"]), _t(pre["mu"]), _t(z), P, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _check_search(got, est, what, bfgs_nll=None):
    pre = est["pre"]
    M = len(est["nll"])
    assert np.array_equal(got["neighbours"], np.stack(est["neighbours"])), what
    assert np.array_equal(got["flags"], est["flags"].astype(np.int32)), (what, got["flags"], est["flags"])
    for m in range(M):
        idx = est["neighbours"][m]
        xs, Yr, mu = pre["x"][idx], pre["Yrot"][idx], pre["mu"]
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


# ------------------------------------------------------------------------------------------- evaluation entry
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_evaluation_entry_against_long_double(shape):
    N, D, M, P = shape
    x, Y, z, est = _shape_case(shape)
    pre = est["pre"]
    # the host optimum and a grid step either side of it: where the search evaluates, and where c was calibrated
    pars = np.zeros((M, 3, 2))
    for m in range(M):
        ls, le = est["log_s"][m], est["log_ell"][m]
        pars[m] = [(ls, le), (ls + 0.5, le + 0.5), (ls - 0.5, le - 0.5)]
    r = _H().pre_loglik_(_t(pre["x"]), _t(pre["Yrot"]), _t(pre["mu"]), _t(z), P, _t(pars))
    torch.cuda.synchronize()
    got, flags = r["nll"].cpu().numpy(), r["flags"].cpu().numpy()
    assert np.array_equal(r["neighbours"].cpu().numpy(), np.stack(est["neighbours"]))
    assert not flags.any()
    for m in range(M):
        idx = est["neighbours"][m]
        xs, Yr = pre["x"][idx], pre["Yrot"][idx]
        for e in range(3):
            ls, le = pars[m, e]
            want = float(PR.nll(xs, Yr, pre["mu"], ls, le, PR.LD))
            gate = PR.eval_gate(xs, Yr, pre["mu"], ls, le)
            print(f"{shape} window {m} point {e}: gpu {got[m, e]:.12f} ref {want:.12f} |d| {abs(got[m, e] - want):.3e} "
                  f"gate {gate:.3e}")
            assert abs(got[m, e] - want) <= gate, (shape, m, e)


def test_window_larger_than_the_limit_is_refused():
    H = _H()
    x, Y, z = _synth(33, 7, 2, 5)
    pre = PR.prepare(x, Y)
    with pytest.raises(ValueError, match="P must lie"):
        H.pre_estimate_(_t(pre["x"]), _t(pre["Yrot"]), _t(pre["mu"]), _t(z), 33)
    from collaborative_nonstationary_multivariate_gaussian_process_amd import _lib as L
    xd, Yd, mud, zd = _t(pre["x"]), _t(pre["Yrot"]), _t(pre["mu"]), _t(z)
    o = torch.zeros(2, 33, dtype=F64, device=_dev())
    rc = L.lib().nmgp_pre_estimate_f64(L.ptr(xd), 1, L.ptr(Yd), 7, L.ptr(mud), L.ptr(zd), 1, 33, 7, 2, 33, L.ptr(o),
                                       L.ptr(o), L.ptr(o), L.ptr(o), None, None, L.stream_handle())
    assert rc == -68


# ------------------------------------------------------------------------------------------- the search
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_search_against_host_reference(shape):
    N, D, M, P = shape
    x, Y, z, est = _shape_case(shape)
    _check_search(_search(est["pre"], z, P), est, str(shape))


@pytest.mark.parametrize("name", ["unit_a", "unit_b", "unit_c", "hour"])
def test_search_on_the_golden_cases(name):
    c = PR.golden_cases(GOLDEN)[name]
    est = PR.cached_estimate(name, c["x"], c["Y"], c["z"], c["P"])
    _check_search(_search(est["pre"], c["z"], c["P"]), est, name, bfgs_nll=c["bfgs_nll"])


# ------------------------------------------------------------------------------------------- neighbours
def _neighbour_case(x, z, P, seed=0):
    rng = np.random.default_rng(seed)
    x = np.asarray(x, np.float64)
    Y = np.stack([np.sin(3 * x) + 0.1 * rng.standard_normal(x.size), np.cos(2 * x) + 0.1 * rng.standard_normal(x.size)], 1)
    pre = PR.prepare(x, Y)
    est = PR.estimate(x, Y, z, P)
    return pre, est


def test_neighbours_at_the_ends_and_on_a_data_point():
    rng = np.random.default_rng(8)
    x = rng.permutation(np.linspace(0.0, 2.0, 41))          # unsorted rows
    z = np.array([-5.0, 9.0, x[7]])
    pre, est = _neighbour_case(x, z, 6)
    got = _search(pre, z, 6)
    assert np.array_equal(got["neighbours"], np.stack(est["neighbours"]))
    assert 7 in got["neighbours"][2]
    assert set(x[got["neighbours"][0]]) == set(np.sort(x)[:6]) and set(x[got["neighbours"][1]]) == set(np.sort(x)[-6:])
    _check_search(got, est, "ends")


def test_duplicate_inputs_and_an_exact_tie_at_the_last_place():
    # rows 2 and 5 repeat the input 1.0; around z = 1 the distances tie in pairs (0.75 / 1.25, 0.5 / 1.5, ...):
    # with P = 5 the last place is a tie between rows 1 (x = 0.5) and 6 (x = 1.5): the lower row wins
    x = np.array([0.25, 0.5, 1.0, 0.75, 1.25, 1.0, 1.5, 1.75, 2.5, 3.0, -1.0, 4.0])
    z = np.array([1.0])
    pre, est = _neighbour_case(x, z, 5)
    assert est["neighbours"][0].tolist() == [1, 2, 3, 4, 5]
    got = _search(pre, z, 5)
    assert got["neighbours"][0].tolist() == [1, 2, 3, 4, 5]
    assert abs(got["box"][0, 0] - np.log(0.25 / 4)) < 1e-14  # delta over the positive gaps only
    _check_search(got, est, "ties")


def test_all_equal_inputs_in_a_window_are_degenerate():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import pre_nmgp as PN
    rng = np.random.default_rng(2)
    x = np.concatenate([np.full(6, 0.5), np.linspace(2.0, 3.0, 20)])
    Y = rng.standard_normal((26, 2))
    pre = PR.prepare(x, Y)
    got = _search(pre, np.array([0.4, 2.5]), 5)
    assert got["flags"][0] == PR.FLAG_DEGENERATE and got["flags"][1] & PR.FLAG_DEGENERATE == 0
    assert np.isnan([got["log_ell"][0], got["log_s"][0], got["nll"][0]]).all() and np.isfinite(got["nll"][1])
    with pytest.raises(ValueError, match=r"degenerate windows.*\[0\]"):
        PN.pre_estimation_partial(x, Y, np.array([0.4, 2.5]), P=5, device="cuda:0")


# ------------------------------------------------------------------------------------------- layout, determinism
def test_strided_inputs_and_untouched_surroundings():
    H = _H()
    shape = (64, 5, 4, 10)
    N, D, M, P = shape
    x, Y, z, est = _shape_case(shape)
    pre = est["pre"]
    plain = _search(pre, z, P)
    nan = float("nan")
    wide = torch.full((N, D + 3), nan, dtype=F64, device=_dev())
    wide[:, :D] = _t(pre["Yrot"])
    xw = torch.full((3 * N,), nan, dtype=F64, device=_dev())
    xw[::3] = _t(pre["x"])
    zw = torch.full((2 * M,), nan, dtype=F64, device=_dev())
    zw[::2] = _t(z)
    bufs = {k: torch.full((M + 4,), nan, dtype=F64, device=_dev()) for k in ("log_ell", "log_s", "nll")}
    fl = torch.full((M + 4,), -7, dtype=torch.int32, device=_dev())
    nb = torch.full((M + 2, P), -7, dtype=torch.int32, device=_dev())
    bx = torch.full((M + 2, 4), nan, dtype=F64, device=_dev())
    out = {k: v[2:M + 2] for k, v in bufs.items()}
    out.update(flags=fl[2:M + 2], neighbours=nb[1:M + 1], box=bx[1:M + 1])
    H.pre_estimate_(xw[::3], wide[:, :D], _t(pre["mu"]), zw[::2], P, out=out)
    torch.cuda.synchronize()
    for k in ("log_ell", "log_s", "nll"):
        assert np.array_equal(out[k].cpu().numpy(), plain[k]), k
        assert torch.isnan(bufs[k][:2]).all() and torch.isnan(bufs[k][M + 2:]).all(), k
    assert np.array_equal(out["flags"].cpu().numpy(), plain["flags"]) and np.array_equal(nb[1:M + 1].cpu().numpy(),
                                                                                         plain["neighbours"])
    assert (fl[:2] == -7).all() and (fl[M + 2:] == -7).all() and (nb[0] == -7).all() and (nb[M + 1] == -7).all()
    assert torch.isnan(bx[0]).all() and torch.isnan(bx[M + 1]).all()
    assert torch.isnan(wide[:, D:]).all() and torch.isnan(xw[1::3]).all() and torch.isnan(zw[1::2]).all()
    # the evaluation entry on the same views
    pars = _t(np.stack([np.stack([plain["log_s"], plain["log_ell"]], 1)], 1))
    nl = torch.full((M + 2, 1), nan, dtype=F64, device=_dev())
    r = H.pre_loglik_(xw[::3], wide[:, :D], _t(pre["mu"]), zw[::2], P, pars, out={"nll": nl[1:M + 1]})
    torch.cuda.synchronize()
    assert np.array_equal(r["nll"].cpu().numpy()[:, 0], plain["nll"])      # the search's own last evaluation
    assert torch.isnan(nl[0]).all() and torch.isnan(nl[M + 1]).all()


def test_two_launches_and_single_window_launches_give_the_same_bits():
    M, P = 70, 5
    x, Y, _ = _synth(50, 3, 2, 77)
    z = np.linspace(-0.1, 1.1, M)
    pre = PR.prepare(x, Y)
    a, b = _search(pre, z, P), _search(pre, z, P)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    H = _H()
    xd, Yd, mud, zd = _t(pre["x"]), _t(pre["Yrot"]), _t(pre["mu"]), _t(z)
    one = [H.pre_estimate_(xd, Yd, mud, zd[m:m + 1], P) for m in range(M)]
    torch.cuda.synchronize()
    for k in a:
        assert np.array_equal(a[k], torch.cat([o[k] for o in one]).cpu().numpy(), equal_nan=True), k


# ------------------------------------------------------------------------------------------- Python surface
def test_pre_estimation_partial_matches_the_reference_shapes_and_the_host():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import nmgp_dsvi as ND
    from collaborative_nonstationary_multivariate_gaussian_process_amd import pre_nmgp as PN
    assert ND.pre_estimation is PN.pre_estimation_partial
    c = PR.golden_cases(GOLDEN)["unit_b"]
    est = PR.cached_estimate("unit_b", c["x"], c["Y"], c["z"], c["P"])
    N, D = c["Y"].shape
    M = c["z"].shape[0]
    # NaN rows are dropped: three extra rows with a missing output change nothing
    x2 = np.concatenate([c["x"], [0.31, 0.32, 0.33]])
    Y2 = np.concatenate([c["Y"], np.full((3, D), 0.5)])
    Y2[N:, 1] = np.nan
    order = np.argsort(x2, kind="stable")
    v, Lt, s = PN.pre_estimation_partial(x2[order], Y2[order], c["z"], device="cuda:0")
    assert v.shape == (M,) and Lt.shape == (D, D, M) and s.shape == (M,)
    assert v.dtype == np.float64 and Lt.dtype == np.float64 and s.dtype == np.float64
    Lref = np.linalg.cholesky(c["Y"].T.dot(c["Y"]) / (N - 1))
    for m in range(M):
        assert np.linalg.norm(Lt[:, :, m] - Lref) / np.linalg.norm(Lref) < 1e-13
    full = PN.pre_estimate(c["x"], c["Y"], c["z"], device="cuda:0")
    assert np.array_equal(full["v_array"], v) and np.array_equal(full["sigma2_err_log_array"], s)
    assert set(full) >= {"v_array", "L_tensor", "sigma2_err_log_array", "nll", "flags", "neighbours", "B"}
    assert np.array_equal(full["neighbours"], np.stack(est["neighbours"]))
    # the device plumbing (GEMM, Jacobi of B) feeds the same optimum as the host's LAPACK did
    for m in range(M):
        idx = est["neighbours"][m]
        gate = PR.eval_gate(est["pre"]["x"][idx], est["pre"]["Yrot"][idx], est["pre"]["mu"], est["log_s"][m],
                            est["log_ell"][m])
        assert abs(full["nll"][m] - est["nll"][m]) <= gate, (m, full["nll"][m], est["nll"][m], gate)
    # compute_loglik_part goes through the evaluation entry: the window's likelihood, the reference's sign
    idx = est["neighbours"][0]
    ll = PN.compute_loglik_part([s[0], v[0]], c["x"][idx], c["Y"][idx], Lref, device="cuda:0")
    gate = PR.eval_gate(est["pre"]["x"][idx], est["pre"]["Yrot"][idx], est["pre"]["mu"], s[0], v[0])
    assert abs(-ll - full["nll"][0]) <= gate
    pars = np.concatenate([[s[0], v[0]], Lref[np.tril_indices(D)]])
    assert PN.compute_loglik(pars, c["x"][idx], c["Y"][idx], device="cuda:0") == ll
