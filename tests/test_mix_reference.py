"""The host references of the exact mixture scores (tests/_mix_ref.py) against the stored 40-digit values and against
the properties a CRPS, a PIT and a quantile must have; the argument checks of predict.score_mixture that need no
device.  No GPU."""
import numpy as np
import pytest
import torch

from tests import _mix_ref as MR

CASES = [(k, S) for k in MR.KINDS for S in MR.S_LIST]


def test_fixture_holds_every_case_and_stays_small():
    import os
    g = MR._golden()
    assert os.path.getsize(MR.GOLDEN) < 200 * 1024
    for kind, S in CASES:
        assert g[f"{kind}_{S}_mp"].shape == (2, len(MR.QUANTITIES), MR.n_fixture(S))
        assert g[f"{kind}_{S}_in"].shape == (2 * S + 1, MR.n_fixture(S))


@pytest.mark.parametrize("het", [True, False])
@pytest.mark.parametrize("kind,S", CASES)
def test_float64_form_matches_the_stored_40_digit_values(kind, S, het):
    """The float64 closed form loses a few S 2^-52 of the values' size at most: its own error must sit well inside
    the floor of the gate that the kernel is held to."""
    c = MR.case(kind, S, het)
    assert c["gold"] is not None
    floor = (S + 16) * MR.EPS * np.maximum(1.0, c["ref"]["t1"] + c["ref"]["t2"])[:c["nf"]]
    for k in ("crps", "t1", "t2"):
        assert (np.abs(c["ref"][k][:c["nf"]] - c["gold"][k]) <= floor).all(), (k, c["e64"])
    assert c["e64_pit"] <= (S + 16) * MR.EPS
    np.testing.assert_array_equal(c["gold"]["crps"] >= 0.0, True)


@pytest.mark.parametrize("kind,S", [(k, S) for k in MR.KINDS for S in (1, 2, 63)])
def test_mpmath_form_reproduces_the_stored_values(kind, S):
    pytest.importorskip("mpmath")
    c = MR.case(kind, S, True)
    got = MR.scoresmp(c["Mu"][:, :c["nf"]], c["Var"][:, :c["nf"]], c["y"][:c["nf"]])
    for k, a in got.items():
        np.testing.assert_array_equal(a, c["gold"][k])


@pytest.mark.parametrize("het", [True, False])
@pytest.mark.parametrize("S", [1, 2, 65])
def test_replicated_equals_the_single_gaussian_closed_form(S, het):
    c = MR.case("replicated", S, het)
    v = c["Var"][0] if het else c["Var"]
    want = MR.single_gaussian(c["Mu"][0], v, c["y"])
    tol = (S + 16) * MR.EPS * np.maximum(1.0, c["ref"]["t1"] + c["ref"]["t2"])
    assert (np.abs(c["ref"]["crps"] - want["crps"]) <= tol).all()
    assert (np.abs(c["ref"]["t2"] - want["t2"]) <= tol).all()
    assert (np.abs(c["ref"]["pit"] - want["pit"]) <= (S + 16) * MR.EPS).all()
    for p in MR.PS:
        q, _ = MR.quantile64(c["Mu"], c["Var"], p)
        zp = float(torch.special.ndtri(torch.tensor(p, dtype=torch.float64)))
        # the bracket is the root +- 1e-12 of the scale, and the bisection stays inside it
        scale = np.abs(c["Mu"][0]) + abs(zp) * np.sqrt(v)
        assert (np.abs(q - (c["Mu"][0] + zp * np.sqrt(v))) <= 1.01e-12 * scale).all()


@pytest.mark.parametrize("kind,S", [(k, S) for k in MR.KINDS for S in (2, 65)])
def test_crps_is_nonnegative_and_pit_is_monotone_in_y(kind, S):
    c = MR.case(kind, S, True)
    assert (c["ref"]["crps"] >= 0.0).all() and (c["ref"]["t2"] > 0.0).all()
    assert ((c["ref"]["pit"] >= 0.0) & (c["ref"]["pit"] <= 1.0)).all()
    ys = np.sort(np.concatenate([c["y"], c["y"] + 0.3, c["y"] - 2.0]).reshape(3, -1), 0)
    pits = np.stack([MR.cdf64(y[None], c["Mu"], c["Var"]) for y in ys])
    assert (np.diff(pits, axis=0) >= 0.0).all()


@pytest.mark.parametrize("kind,S", [(k, S) for k in MR.KINDS for S in (1, 65)])
def test_quantiles_bracket_monotone_and_residual(kind, S):
    """The bracket holds the root; the bisection ends at adjacent doubles inside it within the step cap; the
    quantiles are monotone in p; the CDF residual of the bisected q meets the bound the kernel is held to."""
    c = MR.case(kind, S, True)
    Mu, Var = c["Mu"][:, :9], c["Var"][:, :9]
    prev = None
    for p in MR.PS:
        lo, hi = MR.bracket64(Mu, Var, p)
        assert (MR.cdf64(lo[None], Mu, Var) <= p).all() and (MR.cdf64(hi[None], Mu, Var) >= p).all()
        q, steps = MR.quantile64(Mu, Var, p)
        assert steps < 200 and ((q >= lo) & (q <= hi)).all()
        res = np.abs(MR.cdf64(q[None], Mu, Var) - p)
        assert (res <= MR.quantile_bound(q, Mu, Var, S)).all(), (p, res.max())
        if prev is not None:
            assert (q >= prev).all()
        prev = q


def test_quantile_residual_against_the_40_digit_cdf():
    mp = pytest.importorskip("mpmath")  # noqa: F841
    c = MR.case("bimodal", 65, True)
    for p in MR.PS:
        q, _ = MR.quantile64(c["Mu"][:, :2], c["Var"][:, :2], p)
        for e in range(2):
            F, f = MR.cdfmp(q[e], c["Mu"][:, e], c["Var"][:, e])
            assert abs(F - p) <= 4.0 * (f * np.spacing(abs(q[e])) + (65 + 16) * MR.EPS)


@pytest.mark.parametrize("kind", MR.KINDS)
def test_scores_do_not_depend_on_the_order_of_the_components(kind):
    c = MR.case(kind, 65, True)
    perm = np.random.default_rng(3).permutation(65)
    a = c["ref"]
    b = MR.scores64(c["Mu"][perm], c["Var"][perm], c["y"])
    tol = (65 + 16) * MR.EPS * np.maximum(1.0, a["t1"] + a["t2"])
    for k in ("crps", "t1", "t2"):
        assert (np.abs(a[k] - b[k]) <= tol).all(), k
    assert (np.abs(a["pit"] - b["pit"]) <= (65 + 16) * MR.EPS).all()
    qa, _ = MR.quantile64(c["Mu"][:, :5], c["Var"][:, :5], 0.975)
    qb, _ = MR.quantile64(c["Mu"][perm][:, :5], c["Var"][perm][:, :5], 0.975)
    # both are roots to within the residual bound, in the CDF of either order
    Fa, Fb = (MR.cdf64(q[None], c["Mu"][:, :5], c["Var"][:, :5]) for q in (qa, qb))
    bound = MR.quantile_bound(qa, c["Mu"][:, :5], c["Var"][:, :5], 65) + MR.quantile_bound(qb, c["Mu"][:, :5],
                                                                                            c["Var"][:, :5], 65)
    assert (np.abs(Fa - Fb) <= bound).all()


def test_score_mixture_argument_checks_raise_before_any_device_work():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    Mu, Var = torch.zeros(5, 3, dtype=torch.float64), torch.ones(5, 3, dtype=torch.float64)
    y = torch.zeros(3, dtype=torch.float64)
    bad = [dict(Mu=Mu.float(), Var=Var), dict(Mu=Mu[0], Var=Var[0]), dict(Mu=Mu, Var=Var[:4]),
           dict(Mu=Mu, Var=Var.float()), dict(Mu=Mu, Var=0.0), dict(Mu=Mu, Var=-1.0), dict(Mu=Mu, Var=float("nan")),
           dict(Mu=Mu, Var=float("inf")), dict(Mu=Mu, Var=Var, y=y[:2]), dict(Mu=Mu, Var=Var, y=y.float()),
           dict(Mu=Mu, Var=Var, quantiles=(0.0,)), dict(Mu=Mu, Var=Var, quantiles=(0.5, 1.0)),
           dict(Mu=Mu, Var=Var, quantiles=(float("nan"),)), dict(Mu=Mu, Var=Var, quantiles=tuple([0.5] * 17)),
           dict(Mu=Mu.t().contiguous().t(), Var=Var), dict(Mu=torch.zeros(0, 3, dtype=torch.float64), Var=1.0),
           dict(Mu=Mu, Var=Var, crps=False), dict(Mu=Mu.numpy(), Var=1.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            predict.score_mixture(**kw)
    with pytest.raises(ValueError, match="device"):                       # every other check passed
        predict.score_mixture(Mu, Var, y=y, quantiles=(0.5,))
