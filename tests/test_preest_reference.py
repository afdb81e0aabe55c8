"""The host reference of the pre-estimation (tests/_preest_ref.py) against what the reference recorded
(tests/golden/preest_cases.npz, written by tests/golden/make_preest_golden.py from the real code/pre_nmgp.py), the
pieces of the Python surface that need no device, and the refusals of the two ABI entries.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

from tests import _preest_ref as PR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "preest_cases.npz")
UNIT = ("unit_a", "unit_b", "unit_c")


def _cases():
    return PR.golden_cases(GOLDEN)


def _windows():
    """(case name, window, xs, Yrot_loc, Y_loc, mu, case, host estimate) over every recorded window."""
    for name, c in _cases().items():
        est = PR.cached_estimate(name, c["x"], c["Y"], c["z"], c["P"])
        pre = est["pre"]
        for m in range(len(c["z"])):
            idx = est["neighbours"][m]
            yield name, m, pre["x"][idx], pre["Yrot"][idx], pre["Y"][idx], pre["mu"], c, est


def test_fixture_shapes_and_basin_condition():
    cs = _cases()
    shapes = {n: (c["Y"].shape[0], c["Y"].shape[1], c["z"].shape[0]) for n, c in cs.items()}
    assert shapes == {"unit_a": (100, 2, 6), "unit_b": (200, 5, 8), "unit_c": (120, 12, 5), "hour": (300, 5, 6)}
    same = np.concatenate([cs[n]["same_basin"] for n in UNIT])
    assert 2 * int(same.sum()) >= same.size
    assert cs["hour"]["x"].max() > 250.0


def test_eval_gate_constant_and_dense_reference():
    """Measured on the fixtures: the float64 restatement differs from the long-double one by at most 1.263 units of
    (P + D) 2^-52 sum_pd(|log G| + E / G) (an hour-scale window); c = 8 x that = 10.1 (PR.GATE_C).  The recorded
    dense nll (scipy's logpdf of the P D x P D Gaussian) is at most 1.96 units from the long-double eigen form."""
    worst, worst_dense = 0.0, 0.0
    for name, m, xs, Yr, Yl, mu, c, est in _windows():
        pts = ((c["bfgs_log_s"][m], c["bfgs_log_ell"][m]), (est["log_s"][m], est["log_ell"][m]))
        for ls, le in pts:
            unit = PR.eval_gate(xs, Yr, mu, ls, le, c=1.0)
            f64, fld = float(PR.nll(xs, Yr, mu, ls, le)), float(PR.nll(xs, Yr, mu, ls, le, PR.LD))
            worst = max(worst, abs(f64 - fld) / unit)
        ls, le = pts[0]
        gate = PR.eval_gate(xs, Yr, mu, ls, le)
        dense = abs(float(PR.nll(xs, Yr, mu, ls, le, PR.LD)) - float(c["bfgs_nll"][m]))
        worst_dense = max(worst_dense, dense / (gate / PR.GATE_C))
        assert dense <= gate, (name, m, dense, gate)
    print(f"float64 vs long double: worst {worst:.4f} units, c = {PR.GATE_C}; dense reference: worst "
          f"{worst_dense:.4f} units")
    assert worst <= PR.GATE_C


def test_dense_restatement_matches_eigen_form():
    """The Kronecker identity itself, on one window per case: the dense P D x P D Gaussian against the eigen form."""
    for name, m, xs, Yr, Yl, mu, c, est in _windows():
        if m != 0:
            continue
        ls, le = est["log_s"][m], est["log_ell"][m]
        d = PR.dense_nll(xs, Yl, est["pre"]["B"], ls, le)
        assert abs(d - float(PR.nll(xs, Yr, mu, ls, le, PR.LD))) <= PR.eval_gate(xs, Yr, mu, ls, le), name


def test_host_optimum_against_bfgs():
    gaps = []
    for name, m, xs, Yr, Yl, mu, c, est in _windows():
        host, bfgs = float(est["nll"][m]), float(c["bfgs_nll"][m])
        gate = PR.eval_gate(xs, Yr, mu, est["log_s"][m], est["log_ell"][m])
        assert host <= bfgs + gate, (name, m, host, bfgs)
        if c["same_basin"][m]:
            assert abs(host - bfgs) <= 1e-6 * max(1.0, abs(bfgs)), (name, m, host, bfgs)
        if name == "hour":
            gaps.append(bfgs - host)
    print("hour-scale gaps:", np.round(gaps, 3))
    assert len(gaps) == 6 and min(gaps) >= 10.0


def test_host_search_is_a_local_minimum_of_the_box():
    """The returned point is no worse than its neighbours a grid step away inside the box."""
    for name, m, xs, Yr, Yl, mu, c, est in _windows():
        le, ls, f = est["log_ell"][m], est["log_s"][m], est["nll"][m]
        lo_e, hi_e, lo_s, hi_s = est["box"][m]
        gate = PR.eval_gate(xs, Yr, mu, ls, le)
        for de, ds in ((1e-3, 0), (-1e-3, 0), (0, 1e-3), (0, -1e-3)):
            e2, s2 = min(max(le + de, lo_e), hi_e), min(max(ls + ds, lo_s), hi_s)
            assert f <= float(PR.nll(xs, Yr, mu, s2, e2)) + gate, (name, m, de, ds)


def test_neighbour_rule_matches_the_reference_rule():
    """code/pre_nmgp.py:9-12 takes np.argsort(|x - z_m|)[:10]; without a tie at the 10th place that is the set of
    the host rule (which orders ties by row index and returns ascending rows)."""
    checked = 0
    for name, c in _cases().items():
        for zm in c["z"]:
            assert PR.no_tie_at(c["x"], zm, 10)
            ref_idx = np.argsort(np.abs(c["x"] - zm))[:10]
            got = PR.neighbours(c["x"], zm, 10)
            assert np.array_equal(np.sort(ref_idx), got) and np.all(np.diff(got) > 0)
            checked += 1
    assert checked == 25
    x = np.array([0.0, 2.0, 1.0, 3.0, -1.0, 1.0])
    assert PR.neighbours(x, 1.0, 3).tolist() == [0, 2, 5]          # |x - 1| = 1 at rows 0 and 1: the lower row


def test_init_from_pre_estimation():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import nmgp_dsvi as ND
    rng = np.random.default_rng(3)
    D, M = 4, 5
    A = rng.standard_normal((D, D))
    Lc = np.linalg.cholesky(A.dot(A.T) + D * np.eye(D))
    Lt = np.stack([Lc] * M, axis=-1)
    v, s = rng.standard_normal(M), rng.standard_normal(M)
    out = ND.init_from_pre_estimation(v, Lt, s)
    assert set(out) == {"mu_v", "mu_U", "sigma2_err_log"}
    assert out["mu_v"].shape == (M,) and out["mu_U"].shape == (D, D, M)
    assert np.array_equal(out["mu_v"], v) and out["sigma2_err_log"] == np.median(s)
    for i in range(D):
        for j in range(D):
            want = Lc[i, j] if j < i else (np.log(Lc[i, i]) if i == j else 0.0)
            assert np.all(out["mu_U"][i, j] == want), (i, j)
    with pytest.raises(ValueError):
        ND.init_from_pre_estimation(v, -Lt, s)


def test_module_surface_without_a_device():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import nmgp_dsvi as ND
    from collaborative_nonstationary_multivariate_gaussian_process_amd import pre_nmgp as PN
    assert ND.pre_estimation is PN.pre_estimation_partial
    with pytest.raises(NotImplementedError):
        PN.pre_estimation_all(np.zeros(3), np.zeros((3, 1)), np.zeros(1))
    Y = np.ones((12, 2))
    Y[3:, 0] = np.nan
    with pytest.raises(ValueError, match="complete rows"):
        PN.pre_estimation_partial(np.arange(12.0), Y, np.zeros(2), P=10)
    with pytest.raises(ValueError, match="P must lie"):
        PN.pre_estimation_partial(np.arange(12.0), np.ones((12, 2)), np.zeros(2), P=2)


@pytest.mark.parametrize("N,D,P", [(40, 5, 2), (40, 5, 33), (40, 129, 10), (9, 5, 10)])
def test_abi_entries_refuse_before_any_launch(N, D, P):
    from collaborative_nonstationary_multivariate_gaussian_process_amd import _lib as L
    lib = L.lib()
    fake = ctypes.c_void_p(0x1000)
    rc = lib.nmgp_pre_estimate_f64(fake, 1, fake, D, fake, fake, 1, N, D, 4, P, fake, fake, fake, fake, fake, fake,
                                   None)
    assert rc == -68
    rc = lib.nmgp_pre_loglik_f64(fake, 1, fake, D, fake, fake, 1, N, D, 4, P, fake, 1, fake, fake, fake, None)
    assert rc == -68


def test_abi_entries_refuse_spans_and_strides():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import _lib as L
    lib = L.lib()
    fake = ctypes.c_void_p(0x1000)
    est = lambda xs, ldy, zs, N=40, M=4: lib.nmgp_pre_estimate_f64(fake, xs, fake, ldy, fake, fake, zs, N, 5, M, 10,
                                                                   fake, fake, fake, fake, fake, fake, None)
    assert est(1, 4, 1) == -68                       # row stride below D
    assert est(0, 5, 1) == -68                       # non-positive strides
    assert est(1, 5, 0) == -68
    assert est(1 << 27, 5, 1) == -68                 # 39 * 2^27 elements of x pass 2^31 - 1
    assert est(1, 1 << 26, 1) == -68                 # 40 rows * 2^26
    assert est(1, 5, 1 << 30, M=4) == -68
    assert est(1, 5, 1, M=0) == 0                    # nothing to do, nothing launched
