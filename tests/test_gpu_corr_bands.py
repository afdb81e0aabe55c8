"""Credible bands of the output correlations on the MI355X: the two kernels of csrc/corrq.hip against the host
references (tests/_corrq_ref.py), and summarize_FY(corr_pairs=...) against the reference's recorded run and against
sample_FY's materialised correlations.

The gates are derived in tests/_corrq_ref.py, not measured: gate_c(D) = (D + 16) 2^-52 per collected sample, order
statistics bit-equal to np.sort, the interpolation within 4 2^-52 max(|a|, |b|), and end to end gate_c(D) + 4 2^-52
(a quantile is 1-Lipschitz in the sup norm of its samples)."""
import functools

import numpy as np
import pytest
import torch

from oracle import nmgp_oracle as O
from tests import _corrq_ref as CR
from tests import _fy_ref as R
from tests import _golden as G

pytestmark = pytest.mark.gpu

F64 = torch.float64
SHAPES = [(1, 1, 1), (2, 11, 3), (16, 3, 2), (17, 70, 37), (17, 65, 5), (50, 9, 6), (128, 3, 5), (33, 256, 2)]
QS = (0.0, 0.025, 0.5, 0.975, 1.0)
SENTINEL = -7.0


def _dev():
    return torch.device("cuda:0")


def _H():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import hip_ops as H
    return H


def _rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu().reshape(-1)
    b = torch.as_tensor(b).detach().double().cpu().reshape(-1)
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


# ------------------------------------------------------------------------------------------------ collect kernel
@functools.lru_cache(maxsize=None)
def _case(D, N, S, sd_zero=False):
    """Inputs and the host reference of EVERY pair (i, j <= i), row q = i (i + 1) / 2 + j of the reference;
    computed once per shape and shared (never modified)."""
    inp = R.make_inputs(D, N, S, seed=1000 * D + 10 * N + S, sd_zero=sd_zero)
    return inp, CR.collect_ref(inp["pair_mu"], inp["pair_sd"], inp["z_p"], R.pairs(D))


def _ref_of(full, pairs, N, S):
    if not pairs:
        return np.empty((0, N, S))
    return np.stack([full[max(i, j) * (max(i, j) + 1) // 2 + min(i, j)] for i, j in pairs])


def _special(D):
    """A pair, its transpose, a diagonal, the pair again, the other diagonal."""
    i, j = D - 1, (D - 1) // 2
    return [(i, j), (j, i), (i, i), (i, j), (j, j)]


def _collect(inp, pairs, s0=0, s1=None, embed=False, C=None, ld_c=None, s_off=0):
    """One nmgp_corr_collect_f64 call on samples [s0, s1) -> C (P, N, ld_c) device tensor."""
    H, dev = _H(), _dev()
    S_all, Q, N = inp["z_p"].shape
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
    pij = torch.tensor(pairs, dtype=torch.int32).reshape(len(pairs), 2).to(dev)
    if C is None:
        C = torch.full((len(pairs), N, S if ld_c is None else ld_c), SENTINEL, dtype=F64, device=dev)
    H.corr_collect_(pm, ps, z_p, pij[:, 0].contiguous(), pij[:, 1].contiguous(), C, s_off=s_off)
    torch.cuda.synchronize()
    return C


@pytest.mark.parametrize("D,N,S", SHAPES)
def test_collect_matches_host_reference(D, N, S):
    inp, full = _case(D, N, S)
    sp = _special(D)
    for what, pairs in (("all", CR.all_pairs(D)), ("one", [sp[0]]), ("special", sp)):
        got = _collect(inp, pairs).cpu().numpy()
        ref = _ref_of(full, pairs, N, S)
        assert got.shape == ref.shape == (len(pairs), N, S)
        e = np.abs(got - ref).max() if pairs else 0.0
        print(f"D={D} N={N} S={S} {what} ({len(pairs)} pairs): {e:.3e} (gate {CR.gate_c(D):.3e})")
        assert np.isfinite(got).all() and e <= CR.gate_c(D), (what, e)
        assert np.abs(got).max(initial=0.0) <= 1.0 + CR.gate_c(D)
    # got is the special list's: transposed and duplicate columns bit-equal, the diagonals exactly 1
    assert np.array_equal(got[1], got[0]) and np.array_equal(got[3], got[0])
    assert (got[2] == 1.0).all() and (got[4] == 1.0).all()


def test_collect_reads_noise_inside_a_wider_block_and_strided_pair_rows():
    D, N, S = 17, 70, 37
    inp, full = _case(D, N, S)
    pairs = CR.all_pairs(D) + _special(D)
    got = _collect(inp, pairs, embed=True)
    assert float(np.abs(got.cpu().numpy() - _ref_of(full, pairs, N, S)).max()) <= CR.gate_c(D)
    assert torch.equal(got, _collect(inp, pairs))


def test_collect_two_sample_ranges_equal_the_single_call():
    D, N, S = 17, 70, 37
    inp, _ = _case(D, N, S)
    pairs = CR.all_pairs(D) + _special(D)
    single = _collect(inp, pairs)
    C = _collect(inp, pairs, 0, 20, ld_c=S)
    assert (C[:, :, 20:] == SENTINEL).all()                             # the first call wrote its range only
    C = _collect(inp, pairs, 20, S, C=C, s_off=20)
    assert torch.equal(C, single)


def test_collect_leaves_the_padding_of_a_wider_C_alone():
    D, N, S = 17, 65, 5
    inp, _ = _case(D, N, S)
    pairs = CR.all_pairs(D)
    C = _collect(inp, pairs, ld_c=S + 6, s_off=2)
    assert (C[:, :, :2] == SENTINEL).all() and (C[:, :, 2 + S:] == SENTINEL).all()
    assert torch.equal(C[:, :, 2:2 + S], _collect(inp, pairs))


def test_collect_keeps_a_non_finite_diagonal():
    """An overflowing exp (cov_11 = inf at input 0) gives NaN for exactly the pairs that touch row 1 at that
    input, as the reference's full matrix product does (inf * 0), and leaves everything else alone."""
    D, N, S = 3, 2, 2
    inp = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in R.make_inputs(D, N, S, seed=5).items()}
    inp["pair_mu"][2, 0] = 800.0                                        # pair (1, 1) at input 0
    pairs = R.pairs(D) + [(0, 1), (1, 2)]
    got = _collect(inp, pairs).cpu().numpy()
    touch = np.array([1 in p for p in pairs])
    assert np.isnan(got[touch, 0]).all()
    assert np.isfinite(got[~touch, 0]).all() and np.isfinite(got[:, 1]).all()
    clean = CR.collect_ref(inp["pair_mu"], inp["pair_sd"], inp["z_p"], pairs)
    assert np.abs(got[:, 1] - clean[:, 1]).max() <= CR.gate_c(D)
    assert np.abs(got[~touch, 0] - clean[~touch, 0]).max() <= CR.gate_c(D)


def test_collect_gives_nan_for_an_output_index_out_of_range_in_that_pair_only():
    D, N, S = 5, 7, 3
    inp, full = _case(D, N, S)
    pairs = [(2, 1), (5, 0), (3, 3), (0, -1), (4, 2)]
    got = _collect(inp, pairs).cpu().numpy()
    assert np.isnan(got[1]).all() and np.isnan(got[3]).all()
    ok = [0, 2, 4]
    assert np.abs(got[ok] - _ref_of(full, [pairs[k] for k in ok], N, S)).max() <= CR.gate_c(D)


@pytest.mark.parametrize("D,N,S", [(17, 70, 37), (33, 256, 2)])
def test_collect_is_deterministic(D, N, S):
    inp, _ = _case(D, N, S)
    pairs = CR.all_pairs(D) + _special(D)
    assert torch.equal(_collect(inp, pairs), _collect(inp, pairs))


def test_collect_zero_pair_sd_gives_equal_samples():
    D, N, S = 17, 5, 6
    inp, full = _case(D, N, S, True)
    pairs = CR.all_pairs(D) + _special(D)
    got = _collect(inp, pairs).cpu().numpy()
    assert np.abs(got - _ref_of(full, pairs, N, S)).max() <= CR.gate_c(D)
    assert (got == got[:, :, :1]).all()


# ------------------------------------------------------------------------------------------------ quantile kernel
def _max_S():
    return _H().quantile_rows_max_S()


def _quantiles(C_np, qs=QS, ld=None):
    """C_np (rows, S) -> (got (nq, rows), device copy before, device copy after)."""
    H, dev = _H(), _dev()
    rows, S = C_np.shape
    if ld is None:
        buf = torch.from_numpy(np.ascontiguousarray(C_np)).to(dev)
        view = buf
    else:
        buf = torch.full((rows, ld), float("nan"), dtype=F64, device=dev)
        buf[:, :S] = torch.from_numpy(np.ascontiguousarray(C_np)).to(dev)
        view = buf[:, :S]
    before = buf.clone()
    got = H.quantile_rows(view, qs)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int64), before.view(torch.int64))       # C is not modified
    return got.cpu().numpy()


def _check_quantiles(got, C_np, qs, what):
    rows, S = C_np.shape
    srt = np.sort(C_np, axis=1)
    ref = CR.quantile_rows_ref(C_np, qs)
    assert got.shape == ref.shape == (len(qs), rows)
    worst = 0.0
    for k, q in enumerate(qs):
        pos = float(q) * (S - 1)
        lo = min(max(int(np.floor(pos)), 0), S - 1)
        hi = min(lo + 1, S - 1)
        if pos == lo:                                                    # an order statistic: bit-equal
            assert np.array_equal(got[k], srt[:, lo]), (what, q)
        scale = np.maximum(np.abs(srt[:, lo]), np.abs(srt[:, hi]))
        err = np.abs(got[k] - ref[k])
        worst = max(worst, float((err / np.maximum(scale, 1e-300)).max()))
        assert (err <= CR.GATE_LERP * scale).all(), (what, q, float(err.max()))
    print(f"{what}: worst |got - ref| / max(|a|, |b|) {worst:.3e} (gate {CR.GATE_LERP:.3e})")


@pytest.mark.parametrize("S", [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 1024, 1025, "max_S"])
def test_quantile_rows_match_sort_and_host_reference(S):
    S = _max_S() if S == "max_S" else S
    for rows in (1, 3, 257):
        C = np.random.default_rng(7 * S + rows).standard_normal((rows, S))
        _check_quantiles(_quantiles(C), C, QS, f"S={S} rows={rows}")
    if S % 2:
        assert QS[2] * (S - 1) == (S - 1) // 2                           # q = 0.5 was checked as an order statistic


def test_quantile_rows_more_quantiles_than_one_launch_carries():
    C = np.random.default_rng(3).standard_normal((5, 77))
    qs = tuple(np.linspace(0.0, 1.0, 41))
    _check_quantiles(_quantiles(C, qs), C, qs, "41 quantiles")


@pytest.mark.parametrize("S", [5, 300, 1024])
def test_quantile_rows_special_rows(S):
    g = np.random.default_rng(S)
    C = g.standard_normal((6, S))
    C[0] = 0.25                                                          # all equal
    C[1] = np.where(g.random(S) < 0.5, -0.5, 0.75)                       # two values repeated
    C[1, :2] = (-0.5, 0.75)
    C[2, 0], C[2, S - 1] = np.inf, -np.inf                               # +-inf sort as values
    C[4, S // 2] = np.nan                                                # a NaN row between two clean rows
    got = _quantiles(C)
    ok = [0, 1, 3, 5]
    _check_quantiles(got[:, ok], C[ok], QS, f"S={S} special rows")
    assert (got[:, 0] == 0.25).all()
    assert got[0, 1] == -0.5 and got[-1, 1] == 0.75
    assert np.isnan(got[:, 4]).all()
    ref2 = CR.quantile_rows_ref(C[2:3], QS)[:, 0]
    assert got[0, 2] == -np.inf and got[-1, 2] == np.inf
    assert np.array_equal(np.isnan(got[:, 2]), np.isnan(ref2))
    fin = np.isfinite(ref2)
    assert np.array_equal(np.isfinite(got[:, 2]), fin)
    assert (np.abs(got[fin, 2] - ref2[fin]) <= CR.GATE_LERP * np.abs(C[2, 1:S - 1]).max()).all()


@pytest.mark.parametrize("S", [3, 65, 1000])
def test_quantile_rows_do_not_read_the_padding(S):
    C = np.random.default_rng(S + 1).standard_normal((9, S))
    got = _quantiles(C, ld=S + 5)                                        # NaN padding
    assert np.isfinite(got).all()
    assert np.array_equal(got, _quantiles(C))


@pytest.mark.parametrize("S,rows", [(37, 300), (1000, 64)])
def test_quantile_rows_are_deterministic(S, rows):
    C = np.random.default_rng(S).standard_normal((rows, S))
    assert np.array_equal(_quantiles(C), _quantiles(C))


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


BASE_KEYS = {"tilde_ell_mean", "tilde_ell_quantiles", "Y_mean", "Y_quantiles", "corr_mean", "corr_sd"}


def test_summarize_FY_band_replays_reference_noise():
    """model.pt state and the reference's recorded noise: the band of the reference's own correlation samples, at
    the existing gate of this path (1e-7 relative: LU against Cholesky on a cond ~1e6 system)."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    g = G.load("sample_cases")
    S = int(g["n_sample"])
    m = _model_from(g, 2, 20, 200)
    qs = (0.025, 0.975)
    out = predict.summarize_FY(m, torch.from_numpy(g["xf"]), n_sample=S, quantiles=qs, noise_tape=g["noise_f"],
                               corr_pairs=[(1, 0)])
    want = np.quantile(g["fy_corrs"][:, :, 1, 0], qs, axis=0)
    width = want[1] - want[0]
    assert np.isfinite(want).all() and width.min() > 1e-3               # not vacuous
    assert set(out) == BASE_KEYS | {"corr_pairs", "corr_quantiles"}
    assert out["corr_pairs"].dtype == torch.int64 and out["corr_pairs"].tolist() == [[1, 0]]
    assert tuple(out["corr_quantiles"].shape) == (2, want.shape[1], 1)
    r = _rel(out["corr_quantiles"][:, :, 0], want)
    print(f"corr_quantiles: rel {r:.3e}; band width {width.min():.3g}..{width.max():.3g}")
    assert r < 1e-7, r


@pytest.mark.parametrize("which", ["golden", "D5", "golden_N300"])
def test_summarize_FY_band_matches_materialised_path_same_seed(which):
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    if which.startswith("golden"):
        g = G.load("sample_cases")
        m, xf, D = _model_from(g, 2, 20, 200), torch.from_numpy(g["xf"]), 2
        if which == "golden_N300":
            xf = torch.linspace(float(xf.min()), float(xf.max()), 300, dtype=F64)
    else:
        (m, xf), D = _default_model(5, 20, 13), 5
    S = 40
    qs = (0.0, 0.025, 0.975, 1.0)
    torch.manual_seed(7)
    _, _, cs = predict.sample_FY(m, xf, S)
    torch.manual_seed(7)
    out = predict.summarize_FY(m, xf, S, quantiles=qs, corr_pairs="all")
    pairs = CR.all_pairs(D)
    assert out["corr_pairs"].tolist() == [list(p) for p in pairs]
    cq = out["corr_quantiles"].cpu().numpy()
    cs = cs.cpu().numpy()
    assert cq.shape == (len(qs), xf.shape[0], len(pairs))
    gate = 2 * CR.gate_c(D) + CR.GATE_LERP
    e = max(np.abs(cq[:, :, p] - np.quantile(cs[:, :, i, j], qs, axis=0)).max() for p, (i, j) in enumerate(pairs))
    print(f"{which}: corr_quantiles {e:.3e} (gate {gate:.3e})")
    assert e <= gate
    cm = out["corr_mean"].cpu().numpy()
    gm = R.gate_corr(D, S)
    for p, (i, j) in enumerate(pairs):
        assert (cq[0, :, p] <= cm[:, i, j] + gm).all() and (cm[:, i, j] <= cq[-1, :, p] + gm).all()


def test_summarize_FY_band_does_not_depend_on_the_batching():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    (m, xf), D, S, N = _default_model(5, 20, 13), 5, 40, 13
    outs = []
    for bb in (8 * S * N, 3 * 8 * S * N, None):
        torch.manual_seed(7)
        kw = {} if bb is None else {"band_bytes": bb}
        outs.append(predict.summarize_FY(m, xf, S, corr_pairs="all", **kw))
    assert outs[0]["corr_quantiles"].shape == (2, N, 10)
    for o in outs[1:]:
        for k in outs[0]:
            assert torch.equal(o[k], outs[0][k]), k
    # order and duplicates are kept; (i, j) and (j, i) are the same curve
    torch.manual_seed(7)
    o = predict.summarize_FY(m, xf, S, corr_pairs=[(4, 2), (2, 4), (3, 3), (4, 2)], band_bytes=2 * 8 * S * N)
    q, allq = o["corr_quantiles"], outs[0]["corr_quantiles"]
    p42 = CR.all_pairs(D).index((4, 2))
    assert o["corr_pairs"].tolist() == [[4, 2], [2, 4], [3, 3], [4, 2]]
    assert torch.equal(q[:, :, 0], allq[:, :, p42]) and torch.equal(q[:, :, 1], q[:, :, 0])
    assert torch.equal(q[:, :, 3], q[:, :, 0]) and bool((q[:, :, 2] == 1.0).all())


def test_summarize_FY_default_has_no_band_keys():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    m, xf = _default_model(5, 20, 13)
    torch.manual_seed(7)
    a = predict.summarize_FY(m, xf, 20)
    torch.manual_seed(7)
    b = predict.summarize_FY(m, xf, 20, corr_pairs=None, band_bytes=1)
    torch.manual_seed(7)
    c = predict.summarize_FY(m, xf, 20, corr_pairs=[(1, 0)])
    assert set(a) == set(b) == BASE_KEYS
    for k in BASE_KEYS:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k


def test_summarize_FY_band_is_collected_in_batches_under_the_memory_cap():
    """A cap, not a measurement: at D = 50, N = 64, S = 256 with every pair and band_bytes = 32 MB the peak
    allocation still grows by less than ONE (S, N, D, D) fp64 tensor (328 MB).  The run without bands grew by
    249 MB and the batch buffer adds 32 MB; all 1225 pairs collected at once would add 160 MB and break the cap."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    D, M, N, S = 50, 20, 64, 256
    m, xf = _default_model(D, M, N)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    torch.manual_seed(3)
    out = predict.summarize_FY(m, xf, S, corr_pairs="all", band_bytes=32 << 20)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    cap = S * N * D * D * 8
    print(f"peak allocation grew by {grown / 1e6:.1f} MB (cap {cap / 1e6:.1f} MB)")
    assert grown < cap
    cq = out["corr_quantiles"]
    g = CR.gate_c(D)
    assert cq.shape == (2, N, 1225) and bool(torch.isfinite(cq).all())
    assert bool((cq[0] <= cq[1]).all()) and float(cq.min()) >= -1.0 - g and float(cq.max()) <= 1.0 + g


def test_summarize_FY_band_falls_back_to_a_sort_above_max_S():
    """n_sample = max_S + 1: the collected batch is sorted by torch.sort.  Checked against np.quantile of the
    correlations collected directly from the same noise stream; the kernel path at max_S is compared for shape
    and ordering only (other samples)."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    H, dev = _H(), _dev()
    D, M, N = 2, 20, 2
    m, xf = _default_model(D, M, N)
    qs = (0.0, 0.025, 0.5, 0.975, 1.0)
    S = _max_S() + 1
    torch.manual_seed(11)
    out = predict.summarize_FY(m, xf, S, quantiles=qs, corr_pairs=[(1, 0)])
    torch.manual_seed(11)
    st = predict._sampling_setup(m, xf.reshape(-1, 1).to(dev).contiguous())
    per = M + N + 3 * N + D * N + N * D
    assert predict._chunk_size(S, N, M) == S
    zc = predict._Draws(dev).take(S, per)
    C = torch.empty(1, N, S, dtype=F64, device=dev)
    pij = torch.tensor([1, 0], dtype=torch.int32, device=dev)
    H.corr_collect_(st["pair_mu"], st["pair_sd"], zc[:, M + N:], pij[:1], pij[1:], C)
    want = np.quantile(C[0].cpu().numpy(), qs, axis=1)
    got = out["corr_quantiles"][:, :, 0].cpu().numpy()
    e = np.abs(got - want).max()
    print(f"fallback at S={S}: {e:.3e} (gate {CR.GATE_LERP:.3e})")
    assert got.shape == (len(qs), N) and e <= CR.GATE_LERP
    torch.manual_seed(11)
    k = predict.summarize_FY(m, xf, S - 1, quantiles=qs, corr_pairs=[(1, 0)])["corr_quantiles"].cpu().numpy()
    assert k.shape == got.shape + (1,)
    assert (np.diff(k[:, :, 0], axis=0) >= 0).all() and (np.diff(got, axis=0) >= 0).all()


def test_summarize_FY_band_refuses_bad_pairs_and_the_module_wrapper_returns_numpy():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import nmgp_dsvi as NM
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    g = G.load("sample_cases")
    m = _model_from(g, 2, 20, 200)
    xf = torch.from_numpy(g["xf"])
    for bad in ([(0, 2)], [(-1, 0)], "every", [1, 2, 3], [(0, 1, 1)], 5):
        with pytest.raises(ValueError):
            predict.summarize_FY(m, xf, 5, corr_pairs=bad)
    N, S = g["xf"].shape[0], 50
    torch.manual_seed(0)
    out = NM.summarize_FY(m, g["xf"], n_sample=S, quantiles=(0.025, 0.5, 0.975), corr_pairs=[(1, 0), (0, 1)])
    assert set(out) == BASE_KEYS | {"corr_pairs", "corr_quantiles"}
    assert all(isinstance(v, np.ndarray) for v in out.values())
    assert out["corr_pairs"].dtype == np.int64 and out["corr_pairs"].tolist() == [[1, 0], [0, 1]]
    cq = out["corr_quantiles"]
    assert cq.shape == (3, N, 2) and np.isfinite(cq).all()
    assert (cq[0] <= cq[1]).all() and (cq[1] <= cq[2]).all() and np.array_equal(cq[:, :, 0], cq[:, :, 1])
    torch.manual_seed(0)
    assert set(NM.summarize_FY(m, g["xf"], n_sample=5)) == BASE_KEYS
