"""The host reference of the local coefficient factors (tests/_prelocal_ref.py): its likelihood against the
reference's dense objective, its window rule, the conditions the GPU fixtures must meet, the sign-flip property that
motivates the estimator, the recorded BFGS runs (tests/golden/prelocal_cases.npz), and what the Python surface and the
ABI entries refuse without a device.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

from tests import _preest_ref as PR
from tests import _prelocal_ref as PL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prelocal_cases.npz")


def _ratio(est, m):
    """|nll_f64 - nll_longdouble| in units of the evaluation gate at c = 1, at the host optimum of window m."""
    xs, Yr, mu = est["xs"][m], est["Yrot_loc"][m], est["mu"][m]
    ls, le = est["log_s"][m], est["log_ell"][m]
    unit = PR.eval_gate(xs, Yr, mu, ls, le, c=1.0)
    return abs(float(PR.nll(xs, Yr, mu, ls, le)) - float(PR.nll(xs, Yr, mu, ls, le, PR.LD))) / unit


@pytest.mark.parametrize("fx", PL.FIXTURES, ids=str)
def test_fixtures_are_interior_and_inside_the_gate(fx):
    """A condition on the inputs of the GPU tests, not a tolerance: no window sits on the lower s edge (there the
    float64 restatement itself leaves the gate), and float64 against long double stays under PR.GATE_C."""
    x, Y, z, est = PL.fixture(fx)
    N, D, M, P, Pc, holdout, _ = fx
    assert len(est["nll"]) == M and est["alpha"] == D / (D + Pc - 1.0)
    assert not (est["flags"] & (PR.FLAG_S_LO | PR.FLAG_DEGENERATE | PL.FLAG_FACTOR)).any(), est["flags"]
    worst = max(_ratio(est, m) for m in range(M))
    print(f"{fx}: flags {est['flags']} worst float64-vs-long-double ratio {worst:.3f} (c = {PR.GATE_C})")
    assert worst <= PR.GATE_C
    for m in range(M):
        assert np.array_equal(est["neighbours"][m], PR.neighbours(est["pre"]["x"], z[m], P))
        assert len(est["cov_neighbours"][m]) == Pc and np.all(np.diff(est["cov_neighbours"][m]) > 0)
        assert np.array_equal(est["B_local"][m], est["B_local"][m].T)
        assert np.allclose(est["L"][m].dot(est["L"][m].T), est["B_local"][m], rtol=1e-12, atol=0)


@pytest.mark.parametrize("fx", [f for f in PL.FIXTURES if f[1] * f[3] <= 200], ids=str)
def test_eigen_form_with_the_local_matrix_matches_the_dense_objective(fx):
    """The Kronecker identity with B_m in place of B: the dense P D x P D Gaussian of code/pre_nmgp.py:48-56 against
    the eigen form, at the host optimum (the shapes whose dense matrix is at most 200 x 200)."""
    x, Y, z, est = PL.fixture(fx)
    for m in range(len(z)):
        xs, Yr, mu = est["xs"][m], est["Yrot_loc"][m], est["mu"][m]
        ls, le = est["log_s"][m], est["log_ell"][m]
        Y_loc = est["pre"]["Y"][est["neighbours"][m]]
        d = PR.dense_nll(xs, Y_loc, est["B_local"][m], ls, le)
        assert abs(d - float(PR.nll(xs, Yr, mu, ls, le, PR.LD))) <= PR.eval_gate(xs, Yr, mu, ls, le), (fx, m)


def _brute(x, zm, P, Pc, holdout):
    keys = sorted((abs(xn - zm), n) for n, xn in enumerate(x) if np.isfinite(abs(xn - zm)))
    rows = [n for _, n in keys]
    return sorted(rows[:P]), sorted(rows[P:P + Pc] if holdout else rows[:Pc])


def test_window_rule():
    # duplicates (rows 2 and 5) and exact ties at the last place of both windows: the lower row wins
    x = np.array([0.25, 0.5, 1.0, 0.75, 1.25, 1.0, 1.5, 1.75, 2.5, 3.0, -1.0, 4.0, 5.0, -0.5])
    fit, cov = PL.windows(x, 1.0, 5, 6, True)
    assert fit.tolist() == [1, 2, 3, 4, 5] and cov.tolist() == [0, 6, 7, 8, 9, 13]     # 1 over 6 at 0.5, 9 over 10 at 2
    assert PL.windows(x, 1.0, 5, 5, True)[1].tolist() == [0, 6, 7, 8, 13]
    fit, cov = PL.windows(x, 1.0, 5, 9, False)
    assert fit.tolist() == [1, 2, 3, 4, 5] and cov.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8]
    # both ends of the range, z on a data point, unsorted rows; against a sort of the (distance, row) pairs
    rng = np.random.default_rng(8)
    x = rng.permutation(np.linspace(0.0, 2.0, 41))
    for zm in (-5.0, 9.0, x[7], 1.0):
        for holdout in (True, False):
            fit, cov = PL.windows(x, zm, 6, 9, holdout)
            bf, bc = _brute(x, zm, 6, 9, holdout)
            assert fit.tolist() == bf and cov.tolist() == bc
            assert np.array_equal(fit, PR.neighbours(x, zm, 6))
    assert set(x[PL.windows(x, -5.0, 6, 9, True)[0]]) == set(np.sort(x)[:6])
    assert set(x[PL.windows(x, 9.0, 6, 9, True)[1]]) == set(np.sort(x)[-15:-6])
    assert 7 in PL.windows(x, x[7], 6, 9, True)[0]
    # non-finite inputs are not rows of the order; too few finite ones: no window
    x = np.array([0.0, np.nan, 1.0, np.inf, 2.0, 3.0])
    assert PL.order(x, 0.9).tolist() == [2, 0, 4, 5]
    assert PL.windows(x, 0.9, 3, 3, True) is None and PL.windows(x, 0.9, 3, 4, False)[1].tolist() == [0, 2, 4, 5]


def test_sign_flip_is_seen_locally_and_not_globally():
    """Two outputs that move together on the left and against each other on the right: the local correlation changes
    sign along z, the global one is near zero, and the local matrix fits every window at least as well (windows that
    contain their fit rows)."""
    x, Y, z = PL.sign_flip_case()
    P, Pc = 10, 40
    loc = PL.cached_estimate_local("sign_flip", x, Y, z, P, Pc, holdout=False)
    glob = PR.cached_estimate("sign_flip", x, Y, z, P)
    corr = lambda B: B[0, 1] / np.sqrt(B[0, 0] * B[1, 1])
    c = [corr(b) for b in loc["B_local"]]
    print("local correlations", np.round(c, 3), "global", round(corr(glob["pre"]["B"]), 3))
    print("local nll", np.round(loc["nll"], 3), "global nll", np.round(glob["nll"], 3))
    assert c[0] > 0.5 and c[-1] < -0.5 and abs(corr(glob["pre"]["B"])) < 0.5
    assert np.all(loc["nll"] <= glob["nll"])


def test_golden_fixture_and_host_optimum_against_bfgs():
    cs = PL.golden_cases(GOLDEN)
    assert {n: (c["Y"].shape[0], c["Y"].shape[1], c["z"].shape[0]) for n, c in cs.items()} == \
        {"local_a": (120, 2, 5), "local_b": (150, 5, 6)}
    same = np.concatenate([c["same_basin"] for c in cs.values()])
    assert 2 * int(same.sum()) >= same.size
    for name, c in cs.items():
        assert c["P"] == 10 and c["Pc"] == 40
        est = PL.cached_estimate_local(("golden", name), c["x"], c["Y"], c["z"], c["P"], c["Pc"], holdout=True)
        for m in range(len(c["z"])):
            xs, Yr, mu = est["xs"][m], est["Yrot_loc"][m], est["mu"][m]
            host, bfgs = float(est["nll"][m]), float(c["bfgs_nll"][m])
            gate = PR.eval_gate(xs, Yr, mu, est["log_s"][m], est["log_ell"][m])
            assert host <= bfgs + gate, (name, m, host, bfgs)
            if c["same_basin"][m]:
                assert abs(host - bfgs) <= 1e-6 * max(1.0, abs(bfgs)), (name, m, host, bfgs)
            # the recorded dense logpdf against the long-double eigen form at BFGS's point
            ls, le = c["bfgs_log_s"][m], c["bfgs_log_ell"][m]
            assert abs(float(PR.nll(xs, Yr, mu, ls, le, PR.LD)) - bfgs) <= PR.eval_gate(xs, Yr, mu, ls, le), (name, m)


def test_module_surface_without_a_device():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import hip_ops as H
    from collaborative_nonstationary_multivariate_gaussian_process_amd import nmgp_dsvi as ND
    from collaborative_nonstationary_multivariate_gaussian_process_amd import pre_nmgp as PN
    assert ND.pre_estimation_local is PN.pre_estimation_local and ND.pre_estimation is PN.pre_estimation_partial
    assert H.PRE_MAX_COV_ROWS == PL.MAX_COV_ROWS == 1024 and H.PRE_FLAG_FACTOR == PL.FLAG_FACTOR == 64
    with pytest.raises(NotImplementedError):
        PN.pre_estimation_all(np.zeros(3), np.zeros((3, 1)), np.zeros(1))
    x, Y, z = PL.synth_local(40, 2, 2, 4)
    for kw, word in ((dict(cov_rows=9), "cov_rows"), (dict(cov_rows=1025), "cov_rows"), (dict(cov_rows=31), "rows"),
                     (dict(cov_rows=41, holdout=False), "rows"), (dict(cov_rows=20, shrink=1.5), "shrink"),
                     (dict(cov_rows=20, shrink=-0.1), "shrink"), (dict(cov_rows=20, shrink=float("nan")), "shrink")):
        with pytest.raises(ValueError, match=word):
            PN.pre_estimation_local(x, Y, z, P=10, **kw)
    with pytest.raises(ValueError, match="P must lie"):
        PN.pre_estimation_local(x, Y, z, P=2, cov_rows=20)
    Pc, w, alpha, holdout = PN._local_plan(40, 2, 10, 30, None, True)
    assert (w, alpha) == PL.weights(2, 30) and alpha == 2 / 31.0 and holdout is True


@pytest.mark.parametrize("P,Pc,holdout,alpha,w", [(10, 9, 0, 0.5, 0.1), (10, 1025, 0, 0.5, 0.1), (10, 31, 1, 0.5, 0.1),
                                                  (10, 41, 0, 0.5, 0.1), (10, 20, 1, -0.1, 0.1), (10, 20, 1, 1.5, 0.1),
                                                  (10, 20, 1, float("nan"), 0.1), (10, 20, 1, 0.5, -1.0),
                                                  (10, 20, 2, 0.5, 0.1), (2, 20, 1, 0.5, 0.1), (33, 40, 0, 0.5, 0.1)])
def test_factor_entry_refuses_before_any_launch(P, Pc, holdout, alpha, w):
    from collaborative_nonstationary_multivariate_gaussian_process_amd import _lib as L
    fake = ctypes.c_void_p(0x1000)
    rc = L.lib().nmgp_pre_local_factor_f64(fake, 1, fake, 5, fake, 5, fake, 1, 40, 5, 4, P, Pc, holdout, w, alpha, fake,
                                           fake, fake, fake, fake, fake, fake, None)
    assert rc == -69


def test_abi_entries_refuse_shapes_strides_and_spans():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import _lib as L
    lib = L.lib()
    fake = ctypes.c_void_p(0x1000)
    fac = lambda xs=1, ldy=5, ldb=5, zs=1, N=40, D=5, M=4: lib.nmgp_pre_local_factor_f64(
        fake, xs, fake, ldy, fake, ldb, fake, zs, N, D, M, 10, 20, 1, 0.1, 0.5, fake, fake, fake, fake, fake, fake, fake,
        None)
    assert fac(ldy=4) == -69 and fac(ldb=4) == -69 and fac(xs=0) == -69 and fac(zs=0) == -69
    assert fac(D=129, ldy=129, ldb=129) == -69 and fac(D=0) == -69 and fac(M=-1) == -69
    assert fac(xs=1 << 27) == -69 and fac(ldy=1 << 26) == -69 and fac(zs=1 << 30) == -69
    assert fac(M=0) == 0                                                # nothing to do, nothing launched
    rc = lib.nmgp_pre_local_factor_f64(fake, 1, fake, 5, None, 5, fake, 1, 40, 5, 4, 10, 20, 1, 0.1, 0.5, fake, fake,
                                       fake, fake, fake, fake, fake, None)
    assert rc == -69
    for P, D in ((2, 5), (33, 5), (10, 129), (10, 0)):
        assert lib.nmgp_pre_estimate_windows_f64(fake, fake, fake, 4, D, P, None, fake, fake, fake, fake, fake,
                                                 None) == -68
        assert lib.nmgp_pre_loglik_windows_f64(fake, fake, fake, 4, D, P, None, fake, 1, fake, fake, None) == -68
    assert lib.nmgp_pre_estimate_windows_f64(fake, fake, None, 4, 5, 10, None, fake, fake, fake, fake, fake, None) == -68
    assert lib.nmgp_pre_estimate_windows_f64(fake, fake, fake, 0, 5, 10, None, fake, fake, fake, fake, fake, None) == 0
    assert lib.nmgp_pre_loglik_windows_f64(fake, fake, fake, 4, 5, 10, None, fake, -1, fake, fake, None) == -68
