"""Group means of the output correlations on the MI355X: the fused kernel (csrc/cgroup.hip) and the group output of
csrc/pcorr.hip against the host references (tests/_cgroup_ref.py), and summarize_FY(corr_groups=...) against the
reference's recorded run and against group means computed from sample_FY's materialised correlations.

The gates are derived from the references, never measured on the kernel (tests/_cgroup_ref.py): gate_group(D, g) =
(D + 16) 2^-52 + g 2^-52 for a group of g correlations, gate_pgroup(D, g, e64) = 16 max(e64, (D + 17) 2^-52) + g 2^-52
for partial correlations, e64 the float64 reference's own error on the input."""
import numpy as np
import pytest
import torch

from oracle import nmgp_oracle as O
from tests import _cgroup_ref as GR
from tests import _fy_ref as R
from tests import _golden as G
from tests import _pcorr_ref as PR

pytestmark = pytest.mark.gpu

F64 = torch.float64
EPS = 2.0 ** -52
SENTINEL = -7.0
BASE_KEYS = {"tilde_ell_mean", "tilde_ell_quantiles", "Y_mean", "Y_quantiles", "corr_mean", "corr_sd"}
GROUP_KEYS = {"corr_group_sizes", "corr_group_mean", "corr_group_sd", "corr_group_quantiles"}
PGROUP_KEYS = {"pcorr_group_mean", "pcorr_group_sd", "pcorr_group_quantiles"}
SHAPES = [(1, 1, 1), (2, 11, 3), (15, 5, 4), (16, 3, 2), (17, 70, 37), (33, 9, 4), (50, 9, 6), (128, 3, 5),
          (17, 256, 3), (128, 256, 2)]


def _dev():
    return torch.device("cuda:0")


def _rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu().reshape(-1)
    b = torch.as_tensor(b).detach().double().cpu().reshape(-1)
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


# ------------------------------------------------------------------------------------------------ tables
def tables(D):
    """name -> list of groups; tables that need more outputs than D has are left out."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    i, j = D - 1, (D - 1) // 2
    out = {"one_pair": [[(i, j)]],
           "special": [[(i, j), (j, i), (i, j), (i, i)]],                # a pair, its transpose, again, a diagonal entry
           "diagonal": [[(d, d) for d in range(D)]]}
    if D >= 2:
        allp = GR.all_pairs(D)
        out["all"] = [allp]
        # 9 overlapping groups, more than waves: runs of the pair list that share half of their entries
        step = max(1, len(allp) // 10)
        out["overlap9"] = [allp[k * step:k * step + 2 * step] for k in range(9) if allp[k * step:k * step + 2 * step]]
    if D >= 6:
        out["blocks3"] = predict.groups_from_labels([3 * d // D for d in range(D)])[0]
        assert len(out["blocks3"]) == 6
    return out


def joined(D):
    """Every table of tables(D) in one list of groups: a group's value does not depend on its neighbours."""
    return [g for t in tables(D).values() for g in t]


# ------------------------------------------------------------------------------------------------ kernel
def _inputs(inp, s0, s1, embed):
    dev = _dev()
    S_all, Q, N = inp["z_p"].shape
    S = s1 - s0
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if embed:          # noise in a wider block [junk 5][z_p Q N][junk 7]; pair rows N + 3 apart; NaN around
        zc = torch.full((S, 5 + Q * N + 7), float("nan"), dtype=F64, device=dev)
        zc[:, 5:5 + Q * N] = t(inp["z_p"][s0:s1]).reshape(S, Q * N)
        wide = torch.full((2, Q, N + 3), float("nan"), dtype=F64, device=dev)
        wide[0, :, :N], wide[1, :, :N] = t(inp["pair_mu"]), t(inp["pair_sd"])
        return wide[0, :, :N], wide[1, :, :N], zc[:, 5:]
    return t(inp["pair_mu"]), t(inp["pair_sd"]), t(inp["z_p"][s0:s1]).reshape(S, Q * N)


def _run(inp, groups, s0=0, s1=None, embed=False, C=None, ld_c=None, s_off=0, partial=False, tab=None, pairs=None,
         sums=False):
    """One group launch on samples [s0, s1) -> C (K, N, ld_c) device tensor: nmgp_corr_group_f64, or with
    partial=True the group output of nmgp_pcorr_accum_groups_f64 (then -> (C, pc_sum, pc_sq, pair C))."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import hip_ops as H
    dev = _dev()
    S_all, Q, N = inp["z_p"].shape
    D = int(round((np.sqrt(8 * Q + 1) - 1) / 2))
    s1 = S_all if s1 is None else s1
    S = s1 - s0
    pm, ps, z_p = _inputs(inp, s0, s1, embed)
    goff, gent = H.group_table(groups, D, dev) if tab is None else tab
    if C is None:
        C = torch.full((goff.numel() - 1, N, S if ld_c is None else ld_c), SENTINEL, dtype=F64, device=dev)
    if not partial:
        H.corr_group_(pm, ps, z_p, goff, gent, C, s_off=s_off)
        torch.cuda.synchronize()
        return C
    kw, psum, psq, Cp = {}, None, None, None
    if sums:
        psum, psq = torch.zeros(N, D, D, dtype=F64, device=dev), torch.zeros(N, D, D, dtype=F64, device=dev)
    if pairs is not None:
        pij = torch.tensor(pairs, dtype=torch.int32).reshape(len(pairs), 2).to(dev)
        Cp = torch.full((len(pairs), N, S), SENTINEL, dtype=F64, device=dev)
        kw = {"pi": pij[:, 0].contiguous(), "pj": pij[:, 1].contiguous(), "C": Cp}
    H.pcorr_accum_(pm, ps, z_p, psum, psq, goff=goff, gent=gent, Cg=C, sg_off=s_off, **kw)
    torch.cuda.synchronize()
    return C, psum, psq, Cp


def _check(got, mat, groups, D, what, e64=None):
    """got (K, N, S) against the group means of the long-double samples mat, group by group at its own gate."""
    want = GR.group_means(mat, groups)
    got = got.cpu().numpy()
    assert got.shape == want.shape
    worst = 0.0
    for k, g in enumerate(groups):
        gate = GR.gate_group(D, len(g)) if e64 is None else GR.gate_pgroup(D, len(g), e64)
        e = GR.err(got[k], want[k])
        worst = max(worst, e / gate)
        assert e <= gate, (what, k, len(g), e, gate)
        if all(i == j for i, j in g):
            assert (got[k] == 1.0).all(), (what, k)                      # a group of diagonal entries is exactly 1
    print(f"{what}: {len(groups)} groups, worst error / gate {worst:.3f}")


@pytest.mark.parametrize("D,N,S", SHAPES)
def test_kernel_matches_host_reference(D, N, S):
    inp, corr, _, _ = GR.case(D, N, S)
    groups = joined(D)
    _check(_run(inp, groups), corr, groups, D, f"corr groups D={D} N={N} S={S}")


@pytest.mark.parametrize("D,N", [(17, 5), (128, 3)])
def test_group_of_one_pair_is_the_correlation_fy_accumulates(D, N):
    """cgroup.hip forms the normalised correlation as fy.hip does (loader and row sums shared in csrc/fy_tiles.hpp,
    the tile product a copy of fy.hip's), so a group of one pair is bit for bit what fy.hip accumulates.  At S = 1 the samples are never sliced and fy_accum_ onto zeroed
    sums leaves the sample's own correlation there.  The two-tile and the eight-tile instantiation, the latter with
    its single wave per SIMD in cgroup.hip."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import hip_ops as H
    inp = GR.case(D, N, 1)[0]
    pairs = [(i, j) for i in range(D) for j in range(i + 1)]
    C = _run(inp, [[p] for p in pairs])                                   # (Q, N, 1)
    pm, ps, z_p = _inputs(inp, 0, 1, False)
    z = lambda *shape: torch.zeros(*shape, dtype=F64, device=_dev())
    csum, csq = z(N, D, D), z(N, D, D)
    H.fy_accum_(pm, ps, z(1, D, N), z_p, z(1, N * D), 0.0, z(1, N, D), csum, csq)
    torch.cuda.synchronize()
    ii, jj = (list(v) for v in zip(*pairs))
    assert torch.equal(csum[:, ii, jj], C[:, :, 0].t())
    assert torch.equal(csum[:, jj, ii], C[:, :, 0].t())                   # fy.hip writes both triangles


@pytest.mark.parametrize("D,N,S", SHAPES)
def test_pcorr_groups_match_host_reference(D, N, S):
    inp, _, pc, e64 = GR.case(D, N, S)
    groups = joined(D)
    _check(_run(inp, groups, partial=True)[0], pc, groups, D, f"pcorr groups D={D} N={N} S={S}", e64)


@pytest.mark.parametrize("D,N,S", [(17, 70, 37), (128, 3, 5)])
@pytest.mark.parametrize("name", ["all", "one_pair", "blocks3", "overlap9", "special", "diagonal"])
def test_each_table_alone(D, N, S, name):
    inp, corr, pc, e64 = GR.case(D, N, S)
    groups = tables(D)[name]
    _check(_run(inp, groups), corr, groups, D, f"{name} D={D}")
    _check(_run(inp, groups, partial=True)[0], pc, groups, D, f"{name} D={D} partial", e64)


def test_a_single_pair_is_the_collected_correlation_bit_for_bit():
    """K groups of one pair each against nmgp_corr_collect_f64's gate and, for the partial correlations, against the
    pair list of the same launch bit for bit (the same LDS value, divided by 1)."""
    D, N, S = 17, 70, 37
    inp, corr, _, _ = GR.case(D, N, S)
    pairs = GR.all_pairs(D)[::7] + [(3, 3)]
    groups = [[p] for p in pairs]
    _check(_run(inp, groups), corr, groups, D, "single pairs")
    Cg, _, _, Cp = _run(inp, groups, partial=True, pairs=pairs)
    assert torch.equal(Cg, Cp)


def test_ill_conditioned_unit_scale_input():
    D, N, S = 17, 9, 6
    inp, corr, pc, e64 = GR.case(D, N, S, False)
    groups = joined(D)
    _check(_run(inp, groups), corr, groups, D, "ill-conditioned corr groups")
    _check(_run(inp, groups, partial=True)[0], pc, groups, D, f"ill-conditioned pcorr groups (e64 {e64:.3e})", e64)


@pytest.mark.parametrize("partial", [False, True])
@pytest.mark.parametrize("D,N,S", [(17, 70, 37), (17, 256, 3), (128, 3, 5)])
def test_bit_equality_of_runs_splits_and_subsets(D, N, S, partial):
    inp = GR.case(D, N, S)[0]
    groups = joined(D)
    run = lambda *a, **k: _run(inp, *a, partial=True, **k)[0] if partial else _run(inp, *a, **k)
    single = run(groups)
    assert torch.equal(run(groups), single)                              # two runs
    cut = S // 2 + 1
    C = run(groups, 0, cut, ld_c=S)                                      # the samples split over two calls
    C = run(groups, cut, S, C=C, s_off=cut)
    assert torch.equal(C, single)
    keep = [len(groups) - 1, 0, 2]                                       # groups removed and reordered
    sub = run([groups[k] for k in keep])
    for r, k in enumerate(keep):
        assert torch.equal(sub[r], single[k]), k


@pytest.mark.parametrize("partial", [False, True])
def test_wider_C_embedded_noise_and_strided_pair_rows(partial):
    D, N, S = 17, 70, 37
    inp = GR.case(D, N, S)[0]
    groups = joined(D)
    run = lambda *a, **k: _run(inp, *a, partial=True, **k)[0] if partial else _run(inp, *a, **k)
    single = run(groups)
    C = run(groups, 0, 20, ld_c=S + 6, s_off=2)
    assert (C[:, :, :2] == SENTINEL).all() and (C[:, :, 22:] == SENTINEL).all()
    C = run(groups, 20, S, C=C, s_off=22)
    assert (C[:, :, :2] == SENTINEL).all() and (C[:, :, 2 + S:] == SENTINEL).all()
    assert torch.equal(C[:, :, 2:2 + S], single)
    assert torch.equal(run(groups, embed=True), single)


@pytest.mark.parametrize("D,N,S", [(17, 70, 37), (17, 256, 3)])
def test_pcorr_sums_pairs_and_groups_in_one_launch(D, N, S):
    """The three outputs are independent switches: sums and pair collection as without groups, groups as alone."""
    from tests.test_gpu_pcorr import _run as pcorr_run
    inp = GR.case(D, N, S)[0]
    groups, pairs = joined(D), GR.all_pairs(D)
    Cg, psum, psq, Cp = _run(inp, groups, partial=True, pairs=pairs, sums=True)
    ps0, pq0, C0 = pcorr_run(inp, pairs=pairs)
    assert torch.equal(psum, ps0) and torch.equal(psq, pq0) and torch.equal(Cp, C0)
    assert torch.equal(Cg, _run(inp, groups, partial=True)[0])
    Cg2, psum2, psq2, _ = _run(inp, groups, partial=True, sums=True)
    assert torch.equal(Cg2, Cg) and torch.equal(psum2, ps0) and torch.equal(psq2, pq0)


@pytest.mark.parametrize("mu,q", [(800.0, 2), (-800.0, 0)])
def test_non_finite_rule(mu, q):
    """exp overflows on L_11 (pair 2) or underflows on L_00 (pair 0) at input 0: every correlation group that touches
    that row is NaN at input 0, as the reference's full-matrix expressions have it, and every partial-correlation
    group is; input 1 is within the gate."""
    D, N, S = 3, 2, 2
    inp = PR.make_inputs(D, N, S, seed=5)
    inp["pair_mu"][q, 0] = mu
    row = 1 if q == 2 else 0
    groups = [[(1, 0)], [(2, 0)], [(2, 1)], [(0, 0)], [(1, 1)], [(2, 2)], GR.all_pairs(D), [(2, 2), (row, row)]]
    got = _run(inp, groups).cpu().numpy()
    # exp(+-800) is finite and non-zero in long double: the NaN pattern is that of the float64 restatement
    want = GR.group_ref(inp["pair_mu"], inp["pair_sd"], inp["z_p"], groups)
    f64 = GR.group_f64(inp["pair_mu"], inp["pair_sd"], inp["z_p"], groups)
    touch = [any(row in p for p in g) for g in groups]
    for k, g in enumerate(groups):
        assert np.isnan(got[k, 0]).all() == touch[k] and np.isnan(got[k, 0]).any() == touch[k], (k, got[k, 0])
        assert np.array_equal(np.isnan(got[k]), np.isnan(f64[k])), k
        assert np.isfinite(got[k, 1]).all()
        assert np.abs(got[k, 1] - want[k, 1]).max() <= GR.gate_group(D, len(g)), k
        if not touch[k]:
            assert np.abs(got[k, 0] - f64[k, 0]).max() <= GR.gate_group(D, len(g)), k
    pgot = _run(inp, groups, partial=True)[0].cpu().numpy()
    pwant = GR.pgroup_ref(inp["pair_mu"], inp["pair_sd"], inp["z_p"], groups)
    assert np.isnan(pgot[:, 0]).all() and np.isfinite(pgot[:, 1]).all()
    assert np.abs(pgot[:, 1] - pwant[:, 1]).max() <= GR.gate_pgroup(D, 3, 0.0)


@pytest.mark.parametrize("partial", [False, True])
def test_out_of_range_entry_in_the_device_table_is_nan_for_its_group_only(partial):
    """Entries that the host validation would refuse, written straight into the device table: indices past D (inside
    and outside the 16-bit fields).  Their groups are NaN, the other groups keep their bits."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import hip_ops as H
    D, N, S = 17, 70, 37
    inp = GR.case(D, N, S)[0]
    groups = tables(D)["blocks3"]
    run = lambda **k: _run(inp, groups, partial=True, **k)[0] if partial else _run(inp, groups, **k)
    clean = run()
    goff, gent = H.group_table(groups, D, _dev())
    off = goff.tolist()
    gent[off[1] + 1] = (D << 16) | 3                                     # group 1: row D
    gent[off[3]] = (200 << 16) | 130                                     # group 3: past every tile
    gent[off[4 + 1] - 1] = -1                                            # group 4: all bits set
    got = run(tab=(goff, gent))
    for k in range(len(groups)):
        if k in (1, 3, 4):
            assert bool(torch.isnan(got[k]).all()), k
        else:
            assert torch.equal(got[k], clean[k]), k


# ------------------------------------------------------------------------------------------------ API
def _model_from(g, D, M, N, **kw):
    from collaborative_nonstationary_multivariate_gaussian_process_amd.nmgp_dsvi import NMGP
    m = NMGP(N, D, g["z"], **kw)
    with torch.no_grad():
        for k in O.PARAM_NAMES:
            if "p_" + k in g:
                getattr(m, k).data.copy_(torch.from_numpy(np.asarray(g["p_" + k])))
    return m


def _default_model(D, M, N):
    from collaborative_nonstationary_multivariate_gaussian_process_amd.nmgp_dsvi import NMGP
    return NMGP(N, D, np.linspace(0.0, 1.0, M)), torch.linspace(0.0, 1.0, N, dtype=F64)


def _six_groups(D=5):
    allp = GR.all_pairs(D)
    return [allp, [(1, 0)], [(4, 0), (0, 4), (4, 0), (2, 2)], [(d, d) for d in range(D)], allp[2:7], allp[5:]]


def _pcorr_two_ways(cs):
    """Partial correlations of the float64 correlation samples (S, N, D, D), by linalg.inv and by Cholesky plus
    solve_triangular (the construction of tests/test_gpu_pcorr.py)."""
    D = cs.shape[-1]

    def norm(Om):
        isd = torch.sqrt(1.0 / torch.diagonal(Om, dim1=-2, dim2=-1))
        pc = -Om * isd.unsqueeze(-1) * isd.unsqueeze(-2)
        i = torch.arange(D)
        pc[..., i, i] = 1.0
        return pc

    a = norm(torch.linalg.inv(cs))
    Lc = torch.linalg.cholesky(cs)
    W = torch.linalg.solve_triangular(Lc, torch.eye(D, dtype=F64, device=cs.device).expand_as(cs), upper=False)
    return a, norm(W.transpose(-1, -2) @ W)


def _np_group_means(mat, groups):
    """(S, N, D, D) numpy float64 -> (S, N, K): per sample, the group means with numpy."""
    return np.stack([np.mean([mat[:, :, i, j] for i, j in g], axis=0) for g in groups], axis=-1)


@pytest.mark.parametrize("N", [13, 300])
def test_summarize_FY_groups_match_the_materialised_route_same_seed(N):
    """N = 300: the kernels run unsliced, as they do at HCP / ECoG size."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    (m, xf), D, S = _default_model(5, 20, N), 5, 40
    qs = (0.0, 0.025, 0.5, 0.975, 1.0)
    groups = _six_groups(D)
    sizes = [len(g) for g in groups]
    torch.manual_seed(7)
    ts, _, cs = predict.sample_FY(m, xf, S)
    torch.manual_seed(7)
    out = predict.summarize_FY(m, xf, S, quantiles=qs, corr_groups=groups, partial=True, keep_samples=True)
    assert torch.equal(out["tilde_ells"], ts)                            # same code, same noise
    assert set(out) == BASE_KEYS | GROUP_KEYS | PGROUP_KEYS | {"pcorr_mean", "pcorr_sd", "Ys", "tilde_ells",
                                                                "corr_group_samples", "pcorr_group_samples"}
    assert out["corr_group_sizes"].tolist() == sizes and out["corr_group_sizes"].dtype == torch.long
    csn = cs.cpu().numpy()
    idx = np.arange(D)
    csn[:, :, idx, idx] = 1.0                                            # the diagonal entry of a group is exactly 1
    gm = _np_group_means(csn, groups)                                    # (S, N, K)
    got = {k: out[k].cpu().numpy() for k in GROUP_KEYS | PGROUP_KEYS}
    assert got["corr_group_mean"].shape == got["corr_group_sd"].shape == (N, len(groups))
    assert got["corr_group_quantiles"].shape == (len(qs), N, len(groups))
    lin = out["corr_mean"].cpu().numpy()
    lin[:, idx, idx] = 1.0
    lin = np.stack([np.mean([lin[:, i, j] for i, j in g], axis=0) for g in groups], axis=-1)   # (N, K)
    a, b = _pcorr_two_ways(cs)
    d = float((a - b).abs().max())
    pgm = _np_group_means(a.cpu().numpy(), groups)
    for k, g in enumerate(sizes):
        gg = GR.gate_group(D, g)
        e_m = np.abs(got["corr_group_mean"][:, k] - gm[:, :, k].mean(0)).max()
        e_s = np.abs(got["corr_group_sd"][:, k] - gm[:, :, k].std(0)).max()
        e_q = np.abs(got["corr_group_quantiles"][:, :, k] - np.quantile(gm[:, :, k], qs, axis=0)).max()
        e_l = np.abs(got["corr_group_mean"][:, k] - lin[:, k]).max()
        pg = 16 * max(d, R.gate_corr(D, S)) + g * EPS
        p_m = np.abs(got["pcorr_group_mean"][:, k] - pgm[:, :, k].mean(0)).max()
        p_s = np.abs(got["pcorr_group_sd"][:, k] - pgm[:, :, k].std(0)).max()
        p_q = np.abs(got["pcorr_group_quantiles"][:, :, k] - np.quantile(pgm[:, :, k], qs, axis=0)).max()
        print(f"N={N} group {k} (g={g}): mean {e_m:.3e} sd {e_s:.3e} q {e_q:.3e} (gate {2 * gg + 4 * EPS:.3e}); "
              f"linearity {e_l:.3e} (gate {R.gate_corr(D, S) + gg:.3e}); partial mean {p_m:.3e} sd {p_s:.3e} "
              f"q {p_q:.3e} (gate {pg:.3e}, d {d:.3e})")
        assert e_m <= 2 * gg + 4 * EPS and e_q <= 2 * gg + 4 * EPS, k
        assert e_s <= 2 * gg + (S + 16) * EPS, k
        assert e_l <= R.gate_corr(D, S) + gg, k
        assert p_m <= pg and p_s <= pg and p_q <= pg, k
    # the diagonal group: exactly 1, sd exactly 0
    assert (got["corr_group_mean"][:, 3] == 1.0).all() and (got["corr_group_sd"][:, 3] == 0.0).all()
    assert (got["corr_group_quantiles"][:, :, 3] == 1.0).all()
    # keep_samples: the returned statistics are those of the returned samples
    for pre in ("corr", "pcorr"):
        smp = out[pre + "_group_samples"]
        assert smp.shape == (len(groups), N, S)
        s = smp.cpu().numpy()
        # two sums of S terms of magnitude <= 1 in different orders: (S - 1) 2^-53 each, and the two-pass sd
        # inherits the error of the mean
        assert np.abs(s.mean(2).T - got[pre + "_group_mean"]).max() <= (S + 16) * EPS
        assert np.abs(s.std(2).T - got[pre + "_group_sd"]).max() <= (S + 16) * EPS
        want_q = np.quantile(s, qs, axis=2).transpose(0, 2, 1)
        assert np.abs(want_q - got[pre + "_group_quantiles"]).max() <= 4 * EPS


def test_summarize_FY_group_of_one_pair_is_the_golden_band():
    """D = 2, recorded noise tape: the group [(1, 0)] is the pair (1, 0)."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    g = G.load("sample_cases")
    S = int(g["n_sample"])
    m = _model_from(g, 2, 20, 200)
    qs = (0.025, 0.975)
    out = predict.summarize_FY(m, torch.from_numpy(g["xf"]), S, quantiles=qs, noise_tape=g["noise_f"],
                               corr_pairs="all", corr_groups=[[(1, 0)]])
    assert set(out) == BASE_KEYS | GROUP_KEYS | {"corr_pairs", "corr_quantiles"}
    gate = GR.gate_group(2, 1)
    e_q = float((out["corr_group_quantiles"][:, :, 0] - out["corr_quantiles"][:, :, 0]).abs().max())
    print(f"D=2 golden: group quantiles vs pair quantiles {e_q:.3e} (gate {gate:.3e})")
    assert e_q <= gate
    c = g["fy_corrs"][:, :, 1, 0]
    for got, want, what in ((out["corr_group_mean"][:, 0], c.mean(0), "mean"),
                            (out["corr_group_quantiles"][:, :, 0], np.quantile(c, qs, axis=0), "quantiles")):
        r = _rel(got, want)
        print(f"  {what}: rel {r:.3e}")
        assert r < 1e-7, (what, r)


@pytest.mark.parametrize("tape", [True, False])
@pytest.mark.parametrize("partial,pairs", [(False, None), (True, None), (False, "all"), (True, "all")])
def test_summarize_FY_groups_do_not_depend_on_the_batching(tape, partial, pairs):
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    D, M, N, S = 5, 20, 13, 40
    m, xf = _default_model(D, M, N)
    kw = {}
    if tape:
        per = M + N + (D * (D + 1) // 2) * N + D * N + N * D
        kw["noise_tape"] = np.random.default_rng(3).standard_normal(S * per)
    outs = []
    for bb in (4 * 8 * S * N, None):                                     # 6 groups in batches of 4 + 2; one batch
        torch.manual_seed(7)
        outs.append(predict.summarize_FY(m, xf, S, corr_groups=_six_groups(D), partial=partial, corr_pairs=pairs,
                                         **({} if bb is None else {"band_bytes": bb}), **kw))
    assert outs[0]["corr_group_quantiles"].shape == (2, N, 6)
    assert GROUP_KEYS <= set(outs[0]) and (PGROUP_KEYS <= set(outs[0])) == partial
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


@pytest.mark.parametrize("partial,pairs", [(False, None), (True, None), (False, [(1, 0)]), (True, [(1, 0)])])
def test_summarize_FY_default_is_unchanged(partial, pairs):
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    m, xf = _default_model(5, 20, 13)
    call = lambda **kw: (torch.manual_seed(7), predict.summarize_FY(m, xf, 20, corr_pairs=pairs, partial=partial,
                                                                    **kw))[1]
    a, b, c = call(), call(corr_groups=None), call(corr_groups=_six_groups())
    want = BASE_KEYS | ({"pcorr_mean", "pcorr_sd"} if partial else set())
    if pairs:
        want |= {"corr_pairs", "corr_quantiles"} | ({"pcorr_quantiles"} if partial else set())
    assert set(a) == set(b) == want
    assert set(c) == want | GROUP_KEYS | (PGROUP_KEYS if partial else set())
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k


def test_summarize_FY_groups_never_hold_the_samples():
    """A cap, not a measurement: at D = 50, N = 64, S = 256 (one chunk), the 7-network partition (28 groups) and
    partial=True, the peak allocation grows by less than ONE (S, N, D, D) fp64 tensor (328 MB)."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    D, M, N, S = 50, 20, 64, 256
    m, xf = _default_model(D, M, N)
    groups, names = predict.groups_from_labels([d % 7 for d in range(D)])
    assert predict._chunk_size(S, N, M) == S and len(groups) == 28
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    torch.manual_seed(3)
    out = predict.summarize_FY(m, xf, S, partial=True, corr_groups=groups)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    cap = S * N * D * D * 8
    print(f"peak allocation grew by {grown / 1e6:.1f} MB (cap {cap / 1e6:.1f} MB)")
    assert grown < cap
    for k in ("corr_group_mean", "corr_group_sd", "pcorr_group_mean", "pcorr_group_sd"):
        assert out[k].shape == (N, 28) and bool(torch.isfinite(out[k]).all()), k
    assert float(out["corr_group_mean"].abs().max()) <= 1.0 + 1e-12
    # the partition: the size-weighted mean of the group means is the mean over all pairs of corr_mean
    w = out["corr_group_sizes"].to(F64)
    i, j = np.tril_indices(D, -1)
    allmean = out["corr_mean"][:, i, j].mean(1)
    e = float(((out["corr_group_mean"] * w).sum(1) / w.sum() - allmean).abs().max())
    assert e <= R.gate_corr(D, S) + GR.gate_group(D, len(i)), e


def test_module_level_summarize_FY_groups_return_numpy():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import nmgp_dsvi as NM
    g = G.load("sample_cases")
    m = _model_from(g, 2, 20, 200)
    N, S = g["xf"].shape[0], 50
    torch.manual_seed(0)
    out = NM.summarize_FY(m, g["xf"], n_sample=S, quantiles=(0.025, 0.5, 0.975), partial=True,
                          corr_groups=[[(1, 0)], [(0, 1), (1, 1)]])
    shapes = {"corr_group_sizes": (2,), "corr_group_mean": (N, 2), "corr_group_sd": (N, 2),
              "corr_group_quantiles": (3, N, 2), "pcorr_group_mean": (N, 2), "pcorr_group_sd": (N, 2),
              "pcorr_group_quantiles": (3, N, 2)}
    assert set(out) == BASE_KEYS | {"pcorr_mean", "pcorr_sd"} | set(shapes)
    for k, shp in shapes.items():
        assert isinstance(out[k], np.ndarray) and out[k].shape == shp and np.isfinite(out[k]).all(), k
    assert out["corr_group_sizes"].tolist() == [1, 2] and (out["corr_group_sd"] >= 0).all()
    q = out["corr_group_quantiles"]
    assert (q[0] <= q[1]).all() and (q[1] <= q[2]).all()
    torch.manual_seed(0)
    assert set(NM.summarize_FY(m, g["xf"], n_sample=5)) == BASE_KEYS
