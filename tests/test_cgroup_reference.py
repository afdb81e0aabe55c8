"""The host references of the group-mean kernels (tests/_cgroup_ref.py) pinned to their float64 restatement and to the
oracle's float64 torch expressions, the parsing of corr_groups, groups_from_labels, and the library's refusals before
launch (no GPU)."""
import ctypes

import numpy as np
import pytest
import torch

from collaborative_nonstationary_multivariate_gaussian_process_amd import _lib as L
from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
from tests import _cgroup_ref as GR
from tests import _fy_ref as R
from tests import _pcorr_ref as PR

ERR_CGROUP_ARG = -64        # include/nmgp_hip.h NMGP_ERR_CGROUP_ARG
ERR_PCORR_ARG = -63         # include/nmgp_hip.h NMGP_ERR_PCORR_ARG
SHAPES = [(2, 11, 3), (17, 70, 37), (50, 9, 6), (128, 3, 5)]


@pytest.mark.parametrize("recipe", ["fy", "pcorr"])
@pytest.mark.parametrize("D,N,S", SHAPES)
def test_float64_restatement_is_within_the_gate_of_long_double(D, N, S, recipe):
    """Every i > j in one group, summed naively: the float64 run against the long-double one, for the correlations
    (gate_group) and the partial correlations (gate_pgroup with e64 of that input)."""
    make = R.make_inputs if recipe == "fy" else PR.make_inputs
    inp = make(D, N, S, PR.seed_of(D, N, S))
    a = (inp["pair_mu"], inp["pair_sd"], inp["z_p"])
    groups = [GR.all_pairs(D)]
    g = len(groups[0])
    want = GR.group_ref(*a, groups)
    e = GR.err(GR.group_f64(*a, groups), want)
    gate = GR.gate_group(D, g)
    print(f"{recipe} D={D} N={N} S={S} g={g}: corr groups f64 vs long double {e:.3e} (gate {gate:.3e})")
    assert want.shape == (1, N, S) and np.isfinite(want).all() and e <= gate
    pc_ld = PR._pcorr(*a, GR.LD)[0]
    e64 = PR.e64_of(PR.pcorr_f64(*a), pc_ld.astype(np.float64))
    pe = GR.err(GR.pgroup_f64(*a, groups), GR.group_means(pc_ld, groups))
    pgate = GR.gate_pgroup(D, g, e64)
    print(f"  pcorr groups f64 vs long double {pe:.3e} (e64 {e64:.3e}, gate {pgate:.3e})")
    assert pe <= pgate
    # a missing pair is far outside the gate: the check can see one
    if g > 1:
        miss = GR.err(GR.group_ref(*a, [groups[0][:-1]]), want)
        assert miss > 100 * gate, (miss, gate)


def _torch_literal(inp):
    """Per sample, the float64 expressions of the oracle's sample_FY tail -> corr (S, N, D, D)."""
    S, Q, N = inp["z_p"].shape
    D = int(round((np.sqrt(8 * Q + 1) - 1) / 2))
    Cs = []
    for s in range(S):
        l = torch.from_numpy(inp["pair_mu"] + inp["pair_sd"] * inp["z_p"][s])          # (Q, N)
        Lc = torch.zeros(D, D, N, dtype=torch.float64)
        for q, (i, j) in enumerate(R.pairs(D)):
            Lc[i, j] = torch.exp(l[q]) if i == j else l[q]
        Ln = Lc.permute(2, 0, 1)                                                       # (N, D, D)
        cov = torch.matmul(Ln, Lc.permute(2, 1, 0))
        invstd = torch.sqrt(torch.diag_embed(1. / torch.diagonal(cov, dim1=-2, dim2=-1)))
        Cs.append(torch.matmul(torch.matmul(invstd, cov), invstd))
    return torch.stack(Cs).numpy()


@pytest.mark.parametrize("D,N,S", [(2, 7, 5), (5, 6, 9), (17, 4, 3)])
def test_group_ref_matches_oracle_expressions(D, N, S):
    inp = R.make_inputs(D, N, S, seed=100 + D)
    groups = [GR.all_pairs(D), [(D - 1, 0)], [(0, D - 1), (D - 1, 0), (1, 1)], [(0, 0), (D - 1, D - 1)]]
    got = GR.group_ref(inp["pair_mu"], inp["pair_sd"], inp["z_p"], groups)
    Ct = _torch_literal(inp)
    assert got.shape == (len(groups), N, S)
    for k, g in enumerate(groups):
        want = np.mean([Ct[:, :, i, j] if i != j else np.ones_like(Ct[:, :, 0, 0]) for i, j in g], axis=0).T
        e = np.abs(got[k] - want).max()
        print(f"D={D} group {k} ({len(g)} entries): {e:.3e} (gate {GR.gate_group(D, len(g)):.3e})")
        assert e <= GR.gate_group(D, len(g))
    assert (got[3] == 1.0).all()
    assert np.array_equal(got[1], GR.group_ref(inp["pair_mu"], inp["pair_sd"], inp["z_p"], [[(0, D - 1)]])[0])


# ------------------------------------------------------------------------------------------------ parsing
@pytest.mark.parametrize("bad", [[], (), [[]], [[(1, 0)], []], [[(0, 1, 2)]], [[(0,)]], [[1, 2]], [[(0, 5)]],
                                 [[(-1, 0)]], [[(5, 5)]], "all", ["ab"], [["ab"]], [[(0.5, 1)]], 7, [[None]]])
def test_corr_groups_refused(bad):
    with pytest.raises(ValueError):
        predict._parse_corr_groups(bad, 5)


def test_corr_groups_keep_order_and_duplicates():
    src = [[(1, 0), (0, 1), (1, 0), (2, 2)], ((4, 3),), [np.array([3, 1]), (np.int64(2), 0)]]
    assert predict._parse_corr_groups(src, 5) == [[(1, 0), (0, 1), (1, 0), (2, 2)], [(4, 3)], [(3, 1), (2, 0)]]
    gen = predict._parse_corr_groups((g for g in src[:2]), 5)            # any iterable of groups
    assert gen == [[(1, 0), (0, 1), (1, 0), (2, 2)], [(4, 3)]]


def test_summarize_FY_refuses_bad_groups_before_any_device_work():
    """The model is never touched: a bare object passes for it."""
    class M:
        D = 5
    for bad in ([], [[]], "all", [[(0, 5)]], [[(0, 1, 2)]]):
        with pytest.raises(ValueError):
            predict.summarize_FY(M(), np.zeros(3), 4, corr_groups=bad)


# ------------------------------------------------------------------------------------------------ groups_from_labels
def test_groups_from_labels_order_and_names():
    groups, names = predict.groups_from_labels(["a", "b", "a", "c", "b", "a"])
    assert names == [("a", "a"), ("b", "b"), ("a", "b"), ("a", "c"), ("b", "c")]     # c is a singleton: no (c, c)
    assert groups[0] == [(2, 0), (5, 0), (5, 2)]
    assert groups[1] == [(4, 1)]
    assert sorted(groups[2]) == [(1, 0), (2, 1), (4, 0), (4, 2), (5, 1), (5, 4)]
    assert sorted(groups[3]) == [(3, 0), (3, 2), (5, 3)]
    assert sorted(groups[4]) == [(3, 1), (4, 3)]
    assert all(i > j for g in groups for i, j in g)


def test_groups_from_labels_within_only_and_degenerate():
    groups, names = predict.groups_from_labels([0, 1, 0, 1, 2], between=False)
    assert names == [(0, 0), (1, 1)] and groups == [[(2, 0)], [(3, 1)]]
    assert predict.groups_from_labels(["x"]) == ([], [])
    assert predict.groups_from_labels([]) == ([], [])
    groups, names = predict.groups_from_labels(["x", "y"])
    assert names == [("x", "y")] and groups == [[(1, 0)]]


@pytest.mark.parametrize("D,nets", [(6, 2), (17, 3), (50, 7)])
def test_groups_from_labels_partition_every_pair_once(D, nets):
    labels = [(3 * i + i // 4) % nets for i in range(D)]
    assert min(labels.count(a) for a in set(labels)) >= 2
    groups, names = predict.groups_from_labels(labels)
    assert len(groups) == len(names) == nets + nets * (nets - 1) // 2
    flat = [p for g in groups for p in g]
    assert sorted(flat) == sorted(GR.all_pairs(D)) and len(set(flat)) == len(flat)
    for g, (a, b) in zip(groups, names):
        assert all({labels[i], labels[j]} == {a, b} for i, j in g)
    assert predict._parse_corr_groups(groups, D) == groups


# ------------------------------------------------------------------------------------------------ refusals
FAKE = ctypes.c_void_p(0x1000)


def _group(lib, D=5, N=4, S=3, K=2, E=3, ld=None, ld_c=None, s_off=0, z_stride=1 << 20, **null):
    p = lambda name: None if name in null else FAKE
    return lib.nmgp_corr_group_f64(p("pair_mu"), p("pair_sd"), N if ld is None else ld, p("z_p"), z_stride, D, N, S,
                                   p("goff"), p("gent"), K, E, p("C"), s_off + S if ld_c is None else ld_c, s_off,
                                   None)


def test_corr_group_refuses_bad_arguments_before_launch():
    """Fake pointers, no GPU: every refusal comes before a launch."""
    lib = L.lib()
    for D in (0, 129, -1):
        assert _group(lib, D=D) == ERR_CGROUP_ARG
    assert _group(lib, N=-1) == ERR_CGROUP_ARG
    assert _group(lib, S=-1, ld_c=8) == ERR_CGROUP_ARG
    assert _group(lib, K=-1) == ERR_CGROUP_ARG
    assert _group(lib, K=4, E=3) == ERR_CGROUP_ARG                       # fewer entries than groups
    for name in ("pair_mu", "pair_sd", "z_p", "goff", "gent", "C"):
        assert _group(lib, **{name: None}) == ERR_CGROUP_ARG, name
    assert _group(lib, ld=3) == ERR_CGROUP_ARG
    assert _group(lib, ld_c=2) == ERR_CGROUP_ARG
    assert _group(lib, s_off=5, ld_c=7) == ERR_CGROUP_ARG
    assert _group(lib, s_off=-1, ld_c=8) == ERR_CGROUP_ARG
    assert _group(lib, z_stride=-1) == ERR_CGROUP_ARG
    for zero in ("N", "S"):
        assert _group(lib, **{zero: 0}) == 0
    assert _group(lib, K=0, E=0) == 0


def _pgroup(lib, D=5, N=256, S=3, P=0, K=2, E=3, ld_cg=None, sg_off=0, sums=False, **null):
    """N = 256: unsliced, so the sums need no workspace."""
    p = lambda name: None if name in null else FAKE
    s = FAKE if sums else None
    return lib.nmgp_pcorr_accum_groups_f64(p("pair_mu"), p("pair_sd"), N, p("z_p"), 1 << 20, D, N, S, s, s,
                                           FAKE if P else None, FAKE if P else None, P, FAKE if P else None, S, 0,
                                           p("goff"), p("gent"), K, E, p("Cg"), sg_off + S if ld_cg is None else ld_cg,
                                           sg_off, None, 0, None)


def test_pcorr_accum_groups_refuses_bad_arguments_before_launch():
    lib = L.lib()
    for D in (0, 129):
        assert _pgroup(lib, D=D) == ERR_PCORR_ARG
    assert _pgroup(lib, K=-1) == ERR_PCORR_ARG
    assert _pgroup(lib, K=0, E=0) == ERR_PCORR_ARG                       # neither sums nor pairs nor groups
    assert _pgroup(lib, K=4, E=3) == ERR_PCORR_ARG
    for name in ("pair_mu", "pair_sd", "z_p", "goff", "gent", "Cg"):
        assert _pgroup(lib, **{name: None}) == ERR_PCORR_ARG, name
    assert _pgroup(lib, ld_cg=2) == ERR_PCORR_ARG
    assert _pgroup(lib, sg_off=5, ld_cg=7) == ERR_PCORR_ARG
    assert _pgroup(lib, sg_off=-1, ld_cg=8) == ERR_PCORR_ARG
    assert _pgroup(lib, N=-1) == ERR_PCORR_ARG and _pgroup(lib, S=-1, ld_cg=8) == ERR_PCORR_ARG
    for zero in ("N", "S"):
        assert _pgroup(lib, **{zero: 0}) == 0
        assert _pgroup(lib, sums=True, P=2, **{zero: 0}) == 0


def test_group_table_is_validated_on_the_host():
    """hip_ops.group_table raises before anything is uploaded (the device argument is never used)."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import hip_ops as H
    for bad in ([], [[]], "all", [[(0, 5)]], [[(0, 1, 2)]], [[(-1, 0)]]):
        with pytest.raises(ValueError):
            H.group_table(bad, 5, "no-such-device")
    goff, gent = H.group_table([[(1, 0), (0, 1), (4, 4)], [(3, 2)]], 5, "cpu")
    assert goff.tolist() == [0, 3, 4] and gent.tolist() == [1 << 16, 1 << 16, (4 << 16) | 4, (3 << 16) | 2]
    assert goff.dtype == gent.dtype == torch.int32
