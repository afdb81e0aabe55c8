"""Partial correlations on the MI355X: the fused kernel (csrc/pcorr.hip) against the host references
(tests/_pcorr_ref.py), and summarize_FY(partial=True) against the reference's recorded run and against partial
correlations computed from sample_FY's materialised correlations.

The gates are measured against the references, never against the kernel (tests/_pcorr_ref.py): with e64 the float64
vs longdouble error of the sequential algorithm on the very input, gate = 16 max(e64, (D + S + 16) 2^-52) for
sum / S, twice that for sq / S, four times for the variance, and the S = 1 gate for a collected sample."""
import functools

import numpy as np
import pytest
import torch

from oracle import nmgp_oracle as O
from tests import _fy_ref as R
from tests import _golden as G
from tests import _pcorr_ref as PR

pytestmark = pytest.mark.gpu

F64 = torch.float64
SENTINEL = -7.0
BASE_KEYS = {"tilde_ell_mean", "tilde_ell_quantiles", "Y_mean", "Y_quantiles", "corr_mean", "corr_sd"}


def _dev():
    return torch.device("cuda:0")


def _rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu().reshape(-1)
    b = torch.as_tensor(b).detach().double().cpu().reshape(-1)
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


def all_pairs(D):
    return [(i, j) for i in range(D) for j in range(i)]


# ------------------------------------------------------------------------------------------------ kernel
@functools.lru_cache(maxsize=None)
def _case(D, N, S, scaled=True):
    """Inputs, their longdouble reference (sum, sq, per-sample pcorr, max |L^-1|) and e64, computed once per shape
    and shared (never modified).  scaled=False: the unit-scale inputs of _fy_ref, ill-conditioned on purpose."""
    seed = PR.seed_of(D, N, S)
    inp = PR.make_inputs(D, N, S, seed) if scaled else R.make_inputs(D, N, S, seed)
    ref = PR.pcorr_ref(inp["pair_mu"], inp["pair_sd"], inp["z_p"])
    e64 = PR.e64_of(PR.pcorr_f64(inp["pair_mu"], inp["pair_sd"], inp["z_p"]), ref[2])
    return inp, ref, e64


def _run(inp, s0=0, s1=None, out=None, embed=False, pairs=None, C=None, ld_c=None, s_off=0, sums=True):
    """One nmgp_pcorr_accum_f64 call on samples [s0, s1) -> (pc_sum, pc_sq, C) device tensors (None where absent)."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import hip_ops as H
    dev = _dev()
    S_all, Q, N = inp["z_p"].shape
    D = int(round((np.sqrt(8 * Q + 1) - 1) / 2))
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
    if sums and out is None:
        out = (torch.zeros(N, D, D, dtype=F64, device=dev), torch.zeros(N, D, D, dtype=F64, device=dev))
    if not sums:
        out = (None, None)
    kw = {}
    if pairs is not None:
        pij = torch.tensor(pairs, dtype=torch.int32).reshape(len(pairs), 2).to(dev)
        if C is None:
            C = torch.full((len(pairs), N, S if ld_c is None else ld_c), SENTINEL, dtype=F64, device=dev)
        kw = {"pi": pij[:, 0].contiguous(), "pj": pij[:, 1].contiguous(), "C": C, "s_off": s_off}
    H.pcorr_accum_(pm, ps, z_p, out[0], out[1], **kw)
    torch.cuda.synchronize()
    return out[0], out[1], C


def _check(got, ref, e64, D, S, what):
    psum, psq = (g.cpu().numpy() for g in got[:2])
    sr, qr, _, winf = ref
    g = PR.gate(D, S, e64)
    e_sum = np.abs(psum / S - sr / S).max()
    e_sq = np.abs(psq / S - qr / S).max()
    e_var = np.abs((psq / S - (psum / S) ** 2) - (qr / S - (sr / S) ** 2)).max()
    print(f"{what}: max|L^-1| {winf:.3g} e64 {e64:.3e}; pc_sum {e_sum:.3e} pc_sq {e_sq:.3e} var {e_var:.3e} "
          f"(gate {g:.3e})")
    assert np.isfinite(psum).all() and np.isfinite(psq).all()
    assert e_sum <= g, (what, e_sum, g)
    assert e_sq <= 2 * g, (what, e_sq, 2 * g)
    assert e_var <= 4 * g, (what, e_var, 4 * g)
    assert np.array_equal(psum, np.swapaxes(psum, 1, 2)) and np.array_equal(psq, np.swapaxes(psq, 1, 2))
    i = np.arange(D)
    assert (psum[:, i, i] == S).all() and (psq[:, i, i] == S).all()     # the diagonal is exactly 1 per sample
    assert np.abs(psum / S).max() <= 1.0 + g


@pytest.mark.parametrize("D,N,S", PR.GPU_SHAPES)
def test_kernel_matches_host_reference(D, N, S):
    from collaborative_nonstationary_multivariate_gaussian_process_amd import _lib as L
    inp, ref, e64 = _case(D, N, S)
    assert (L.lib().nmgp_pcorr_workspace_size(D, N, S) == 0) == ((D, N, S) in PR.UNSLICED or S == 1)
    _check(_run(inp), ref, e64, D, S, f"D={D} N={N} S={S}")


def test_kernel_follows_the_references_own_error_on_ill_conditioned_inputs():
    """Unit-scale off-diagonal rows at D = 17 (max |L^-1| = 156 on this input): the same gate formula, which follows
    the float64 reference's own error on that input (e64 = 1.0e-15 here: the normalisation is forgiving)."""
    D, N, S = 17, 9, 6
    inp, ref, e64 = _case(D, N, S, False)
    _check(_run(inp), ref, e64, D, S, f"ill-conditioned D={D} N={N} S={S}")


def test_kernel_reads_noise_inside_a_wider_block_and_strided_pair_rows():
    D, N, S = 17, 70, 37
    inp, ref, e64 = _case(D, N, S)
    pairs = all_pairs(D)
    got = _run(inp, embed=True, pairs=pairs)
    _check(got, ref, e64, D, S, "embedded")
    for a, b in zip(got, _run(inp, pairs=pairs)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("D,N,S", [(17, 70, 37), (17, 256, 3)])
def test_kernel_is_deterministic(D, N, S):
    inp, _, _ = _case(D, N, S)
    pairs = all_pairs(D)
    for x, y in zip(_run(inp, pairs=pairs), _run(inp, pairs=pairs)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("D,N,S,cut", [(17, 70, 37, 20), (17, 256, 3, 2)])
def test_kernel_two_calls_accumulate_to_the_single_call(D, N, S, cut):
    inp, ref, e64 = _case(D, N, S)
    single = _run(inp)
    ps, pq, _ = _run(inp, 0, cut)
    ps, pq, _ = _run(inp, cut, S, out=(ps, pq))
    _check((ps, pq), ref, e64, D, S, f"split {cut} + {S - cut}")
    g = PR.gate(D, S, e64)
    assert float((ps - single[0]).abs().max()) / S <= g
    assert float((pq - single[1]).abs().max()) / S <= 2 * g


def _special(D):
    """A pair, its transpose, the pair again, a diagonal pair."""
    i, j = D - 1, (D - 1) // 2
    return [(i, j), (j, i), (i, j), (i, i)]


def test_collection_matches_the_per_sample_reference():
    D, N, S = 17, 70, 37
    inp, ref, e64 = _case(D, N, S)
    pc = ref[2]                                                          # (S, N, D, D)
    pairs = all_pairs(D) + _special(D)
    ps, pq, C = _run(inp, pairs=pairs)
    want = np.stack([pc[:, :, i, j].T for i, j in pairs])                # (P, N, S)
    got = C.cpu().numpy()
    g = PR.gate(D, 1, e64)
    e = np.abs(got - want).max()
    print(f"collect D={D} N={N} S={S} ({len(pairs)} pairs): {e:.3e} (gate {g:.3e})")
    assert got.shape == want.shape and np.isfinite(got).all() and e <= g
    k = len(all_pairs(D))
    assert np.array_equal(got[k + 1], got[k]) and np.array_equal(got[k + 2], got[k])
    assert (got[k + 3] == 1.0).all()
    # the sums are those of the call without a pair list
    plain = _run(inp)
    assert torch.equal(ps, plain[0]) and torch.equal(pq, plain[1])
    # collect only: the same C, no sum touched
    _, _, C2 = _run(inp, pairs=pairs, sums=False)
    assert torch.equal(C2, C)


@pytest.mark.parametrize("D,N,S", [(128, 3, 5), (33, 256, 2)])
def test_collection_at_other_tile_counts(D, N, S):
    inp, ref, e64 = _case(D, N, S)
    pairs = _special(D) + [(D - 1, 0), (16, 15), (D // 2, D // 2 - 1)]
    _, _, C = _run(inp, pairs=pairs, sums=False)
    want = np.stack([ref[2][:, :, i, j].T for i, j in pairs])
    e = np.abs(C.cpu().numpy() - want).max()
    g = PR.gate(D, 1, e64)
    print(f"collect D={D} N={N} S={S}: {e:.3e} (gate {g:.3e})")
    assert e <= g


def test_collection_leaves_the_other_columns_of_a_wider_C_alone():
    D, N, S = 17, 70, 37
    inp, _, _ = _case(D, N, S)
    pairs = all_pairs(D)
    single = _run(inp, pairs=pairs, sums=False)[2]
    C = _run(inp, 0, 20, pairs=pairs, ld_c=S + 6, s_off=2, sums=False)[2]
    assert (C[:, :, :2] == SENTINEL).all() and (C[:, :, 22:] == SENTINEL).all()
    C = _run(inp, 20, S, pairs=pairs, C=C, s_off=22, sums=False)[2]
    assert (C[:, :, :2] == SENTINEL).all() and (C[:, :, 2 + S:] == SENTINEL).all()
    assert torch.equal(C[:, :, 2:2 + S], single)


@pytest.mark.parametrize("mu", [800.0, -800.0])
def test_kernel_non_finite_rule(mu):
    """An exp that overflows (inf) or underflows (0) on the diagonal of L at input 0: every partial correlation at
    that input is NaN -- the diagonal, the sums and C included -- and input 1 is untouched."""
    D, N, S = 3, 2, 2
    inp = PR.make_inputs(D, N, S, seed=5)
    inp["pair_mu"][2, 0] = mu                                            # pair (1, 1) at input 0
    pairs = R.pairs(D)
    ps, pq, C = (g.cpu().numpy() for g in _run(inp, pairs=pairs))
    assert np.isnan(ps[0]).all() and np.isnan(pq[0]).all() and np.isnan(C[:, 0]).all()
    clean = PR.pcorr_f64(inp["pair_mu"], inp["pair_sd"], inp["z_p"])
    g = PR.gate(D, S, 0.0)
    assert np.isfinite(ps[1]).all() and np.abs(ps[1] - clean[:, 1].sum(0)).max() / S <= g
    assert (ps[1][[0, 1, 2], [0, 1, 2]] == S).all()
    want = np.stack([clean[:, 1, i, j] for i, j in pairs])
    assert np.abs(C[:, 1] - want).max() <= g


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


def test_summarize_FY_partial_at_two_outputs_is_the_golden_correlation():
    """D = 2: nothing to condition on, the partial correlation IS the correlation -- of the same call within
    4 gate_corr, and of the reference's recorded samples at the path's existing 1e-7 relative gate."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    g = G.load("sample_cases")
    S = int(g["n_sample"])
    m = _model_from(g, 2, 20, 200)
    qs = (0.025, 0.975)
    out = predict.summarize_FY(m, torch.from_numpy(g["xf"]), S, quantiles=qs, noise_tape=g["noise_f"], partial=True,
                               corr_pairs="all")
    assert set(out) == BASE_KEYS | {"corr_pairs", "corr_quantiles", "pcorr_mean", "pcorr_sd", "pcorr_quantiles"}
    gate = 4 * R.gate_corr(2, S)
    e_m = float((out["pcorr_mean"][:, 1, 0] - out["corr_mean"][:, 1, 0]).abs().max())
    e_q = float((out["pcorr_quantiles"][:, :, 0] - out["corr_quantiles"][:, :, 0]).abs().max())
    print(f"D=2 golden: pcorr_mean vs corr_mean {e_m:.3e}, quantiles {e_q:.3e} (gate {gate:.3e})")
    assert e_m <= gate and e_q <= gate
    c = g["fy_corrs"][:, :, 1, 0]
    for got, want, what in ((out["pcorr_mean"][:, 1, 0], c.mean(0), "mean"), (out["corr_mean"][:, 1, 0], c.mean(0), "cm"),
                            (out["pcorr_quantiles"][:, :, 0], np.quantile(c, qs, axis=0), "quantiles"),
                            (out["corr_quantiles"][:, :, 0], np.quantile(c, qs, axis=0), "cq")):
        r = _rel(got, want)
        print(f"  {what}: rel {r:.3e}")
        assert r < 1e-7, (what, r)
    assert bool((torch.diagonal(out["pcorr_mean"], dim1=1, dim2=2) == 1.0).all())
    assert bool((torch.diagonal(out["pcorr_sd"], dim1=1, dim2=2) == 0.0).all())


def _pcorr_two_ways(cs):
    """Partial correlations of the float64 correlation samples (S, N, D, D), by linalg.inv and by Cholesky plus
    solve_triangular."""
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


@pytest.mark.parametrize("N", [13, 300])
def test_summarize_FY_partial_matches_the_materialised_route_same_seed(N):
    """N = 300: the kernel runs unsliced, as it does at HCP / ECoG size."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    (m, xf), D, S = _default_model(5, 20, N), 5, 40
    qs = (0.0, 0.025, 0.975, 1.0)
    torch.manual_seed(7)
    ts, _, cs = predict.sample_FY(m, xf, S)
    torch.manual_seed(7)
    out = predict.summarize_FY(m, xf, S, quantiles=qs, partial=True, corr_pairs="all", keep_samples=True)
    assert torch.equal(out["tilde_ells"], ts)                            # same code, same noise
    a, b = _pcorr_two_ways(cs)
    d = float((a - b).abs().max())
    gate = 16 * max(d, R.gate_corr(D, S))
    pairs = all_pairs(D)
    a = a.cpu().numpy()
    e_m = np.abs(out["pcorr_mean"].cpu().numpy() - a.mean(0)).max()
    e_s = np.abs(out["pcorr_sd"].cpu().numpy() - a.std(0)).max()
    pq = out["pcorr_quantiles"].cpu().numpy()
    assert pq.shape == (len(qs), N, len(pairs))
    e_q = max(np.abs(pq[:, :, p] - np.quantile(a[:, :, i, j], qs, axis=0)).max() for p, (i, j) in enumerate(pairs))
    print(f"N={N}: inv vs cholesky d {d:.3e}; pcorr_mean {e_m:.3e} pcorr_sd {e_s:.3e} pcorr_quantiles {e_q:.3e} "
          f"(gate {gate:.3e})")
    assert e_m <= gate and e_s <= gate and e_q <= gate


@pytest.mark.parametrize("tape", [True, False])
def test_summarize_FY_partial_does_not_depend_on_the_batching(tape):
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    D, M, N, S = 5, 20, 13, 40
    m, xf = _default_model(D, M, N)
    kw = {}
    if tape:
        per = M + N + (D * (D + 1) // 2) * N + D * N + N * D
        kw["noise_tape"] = np.random.default_rng(3).standard_normal(S * per)
    outs = []
    for bb in (4 * 8 * S * N, None):                                     # 10 pairs in batches of 4, 4, 2; one batch
        torch.manual_seed(7)
        outs.append(predict.summarize_FY(m, xf, S, corr_pairs="all", partial=True,
                                         **({} if bb is None else {"band_bytes": bb}), **kw))
    assert outs[0]["pcorr_quantiles"].shape == (2, N, 10)
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


def test_summarize_FY_partial_never_holds_the_samples():
    """A cap, not a measurement: at D = 50, N = 64, S = 256 (one chunk) the peak allocation grows by less than ONE
    (S, N, D, D) fp64 tensor (328 MB)."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    D, M, N, S = 50, 20, 64, 256
    m, xf = _default_model(D, M, N)
    assert predict._chunk_size(S, N, M) == S
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    torch.manual_seed(3)
    out = predict.summarize_FY(m, xf, S, partial=True)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    cap = S * N * D * D * 8
    print(f"peak allocation grew by {grown / 1e6:.1f} MB (cap {cap / 1e6:.1f} MB)")
    assert grown < cap
    pm, psd = out["pcorr_mean"], out["pcorr_sd"]
    assert pm.shape == psd.shape == (N, D, D) and bool(torch.isfinite(pm).all()) and bool(torch.isfinite(psd).all())
    assert torch.equal(pm, pm.transpose(1, 2))
    assert bool((torch.diagonal(pm, dim1=1, dim2=2) == 1.0).all()) and float(pm.abs().max()) <= 1.0 + 1e-12


def test_summarize_FY_default_is_unchanged():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    m, xf = _default_model(5, 20, 13)
    torch.manual_seed(7)
    a = predict.summarize_FY(m, xf, 20, corr_pairs=[(1, 0)])
    torch.manual_seed(7)
    b = predict.summarize_FY(m, xf, 20, corr_pairs=[(1, 0)], partial=False)
    torch.manual_seed(7)
    c = predict.summarize_FY(m, xf, 20, corr_pairs=[(1, 0)], partial=True)
    torch.manual_seed(7)
    d = predict.summarize_FY(m, xf, 20)
    assert set(d) == BASE_KEYS and set(a) == set(b) == BASE_KEYS | {"corr_pairs", "corr_quantiles"}
    assert set(c) == set(a) | {"pcorr_mean", "pcorr_sd", "pcorr_quantiles"}
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k


def test_module_level_summarize_FY_partial_returns_numpy():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import nmgp_dsvi as NM
    g = G.load("sample_cases")
    m = _model_from(g, 2, 20, 200)
    N, D, S = g["xf"].shape[0], 2, 50
    torch.manual_seed(0)
    out = NM.summarize_FY(m, g["xf"], n_sample=S, quantiles=(0.025, 0.5, 0.975), corr_pairs="all", partial=True)
    shapes = {"pcorr_mean": (N, D, D), "pcorr_sd": (N, D, D), "pcorr_quantiles": (3, N, 1)}
    assert set(out) == BASE_KEYS | {"corr_pairs", "corr_quantiles"} | set(shapes)
    for k, shp in shapes.items():
        assert isinstance(out[k], np.ndarray) and out[k].shape == shp and np.isfinite(out[k]).all(), k
    assert (out["pcorr_sd"] >= 0).all()
    q = out["pcorr_quantiles"]
    assert (q[0] <= q[1]).all() and (q[1] <= q[2]).all()
    torch.manual_seed(0)
    assert set(NM.summarize_FY(m, g["xf"], n_sample=5)) == BASE_KEYS
