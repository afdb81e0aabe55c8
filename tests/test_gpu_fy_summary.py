"""summarize_FY on the MI355X: the fused kernel (csrc/fy.hip) against the host reference (tests/_fy_ref.py), and
the API against the reference's recorded run and against sample_FY's materialised path.

The gates are derived, not measured: after normalisation every term of a correlation dot product is bounded by 1
(Cauchy-Schwarz), and exp / fma / sqrt may differ by an ulp or two: |corr_sum / S - ref| <= (D + S + 16) 2^-52,
twice that for corr_sq / S, four times for the variance, |Y - ref| <= (D + 16) 2^-52 A elementwise."""
import functools

import numpy as np
import pytest
import torch

from oracle import nmgp_oracle as O
from tests import _fy_ref as R
from tests import _golden as G

pytestmark = pytest.mark.gpu

F64 = torch.float64
SHAPES = [(1, 1, 1), (2, 11, 3), (3, 7, 5), (15, 5, 4), (16, 3, 2), (17, 70, 37), (50, 9, 6), (128, 3, 5)]
# N >= 256: the samples are not sliced -- the branch summarize_FY takes at HCP / ECoG size (N = 1000): one workgroup
# per input loops over every sample and adds in place onto both triangles of corr_sum / corr_sq, no workspace.
# (40, 200, 5): sliced, with 3 and 2 samples per slice (the other sliced shapes mostly come out at 1).
UNSLICED = [(17, 256, 3), (33, 256, 2), (128, 256, 2)]
MULTI_SAMPLE_SLICES = [(40, 200, 5)]


def _rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu().reshape(-1)
    b = torch.as_tensor(b).detach().double().cpu().reshape(-1)
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


@functools.lru_cache(maxsize=None)
def _case(D, N, S, sd_zero=False):
    """Inputs and their host reference, computed once per shape and shared (never modified)."""
    inp = R.make_inputs(D, N, S, seed=1000 * D + 10 * N + S, sd_zero=sd_zero)
    return inp, R.fy_ref(**inp)


def _run(inp, s0=0, s1=None, out=None, embed=False):
    """One nmgp_fy_accum_f64 call on samples [s0, s1) -> (Y, corr_sum, corr_sq) device tensors."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import hip_ops as H
    dev = torch.device("cuda:0")
    S_all, D, N = inp["G"].shape
    s1 = S_all if s1 is None else s1
    S, Q = s1 - s0, D * (D + 1) // 2
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if embed:          # noise in a wider block [junk 5][z_p Q N][junk 3][z_f N D][junk 7]; pair rows N + 3 apart
        per = 5 + Q * N + 3 + N * D + 7
        zc = torch.full((S, per), float("nan"), dtype=F64, device=dev)
        zc[:, 5:5 + Q * N] = t(inp["z_p"][s0:s1]).reshape(S, Q * N)
        o_f = 5 + Q * N + 3
        zc[:, o_f:o_f + N * D] = t(inp["z_f"][s0:s1]).reshape(S, N * D)
        z_p, z_f = zc[:, 5:], zc[:, o_f:]
        wide = torch.full((2, Q, N + 3), float("nan"), dtype=F64, device=dev)
        wide[0, :, :N], wide[1, :, :N] = t(inp["pair_mu"]), t(inp["pair_sd"])
        pm, ps = wide[0, :, :N], wide[1, :, :N]
    else:
        per = Q * N + N * D
        zc = torch.cat([t(inp["z_p"][s0:s1]).reshape(S, Q * N), t(inp["z_f"][s0:s1]).reshape(S, N * D)], 1).contiguous()
        z_p, z_f = zc, zc[:, Q * N:]
        pm, ps = t(inp["pair_mu"]), t(inp["pair_sd"])
    if out is None:
        out = (torch.zeros(N, D, D, dtype=F64, device=dev), torch.zeros(N, D, D, dtype=F64, device=dev))
    Y = torch.full((S, N, D), float("nan"), dtype=F64, device=dev)
    H.fy_accum_(pm, ps, t(inp["G"][s0:s1]), z_p, z_f, inp["sd_err"], Y, out[0], out[1])
    torch.cuda.synchronize()
    return Y, out[0], out[1]


def _check(got, ref, D, S, what):
    Y, csum, csq = (g.cpu().numpy() for g in got)
    Yr, sr, qr, A = ref
    g = R.gate_corr(D, S)
    e_sum = np.abs(csum / S - sr / S).max()
    e_sq = np.abs(csq / S - qr / S).max()
    e_var = np.abs((csq / S - (csum / S) ** 2) - (qr / S - (sr / S) ** 2)).max()
    e_y = (np.abs(Y - Yr) / A).max()
    print(f"{what}: corr_sum {e_sum:.3e} corr_sq {e_sq:.3e} var {e_var:.3e} (gate {g:.3e}); "
          f"Y/A {e_y:.3e} (gate {R.gate_y(D):.3e})")
    assert np.isfinite(Y).all() and np.isfinite(csum).all() and np.isfinite(csq).all()
    assert e_sum <= g, (what, e_sum, g)
    assert e_sq <= 2 * g, (what, e_sq, 2 * g)
    assert e_var <= 4 * g, (what, e_var, 4 * g)
    assert e_y <= R.gate_y(D), (what, e_y, R.gate_y(D))
    assert np.array_equal(csum, np.swapaxes(csum, 1, 2)) and np.array_equal(csq, np.swapaxes(csq, 1, 2))
    # the diagonal is accumulated as exactly 1 per sample (documented in include/nmgp_hip.h): sums of S ones
    i = np.arange(D)
    assert (csum[:, i, i] == csum[0, 0, 0]).all() and (csq[:, i, i] == csum[0, 0, 0]).all()
    assert float(csum[0, 0, 0]).is_integer() and 1 <= csum[0, 0, 0] <= S


@pytest.mark.parametrize("D,N,S", SHAPES + UNSLICED + MULTI_SAMPLE_SLICES)
def test_kernel_matches_host_reference(D, N, S):
    from collaborative_nonstationary_multivariate_gaussian_process_amd import _lib as L
    inp, ref = _case(D, N, S)
    assert (L.lib().nmgp_fy_workspace_size(D, N, S) == 0) == ((D, N, S) in UNSLICED or S == 1)
    _check(_run(inp), ref, D, S, f"D={D} N={N} S={S}")


def test_kernel_reads_noise_inside_a_wider_block_and_strided_pair_rows():
    D, N, S = 17, 70, 37
    inp, ref = _case(D, N, S)
    got = _run(inp, embed=True)
    _check(got, ref, D, S, "embedded")
    plain = _run(inp)
    for a, b in zip(got, plain):
        assert torch.equal(a, b)


def test_kernel_zero_pair_sd_gives_zero_variance():
    D, N, S = 17, 5, 6
    inp, ref = _case(D, N, S, True)
    got = _run(inp)
    _check(got, ref, D, S, "pair_sd=0")
    csum, csq = got[1].cpu().numpy(), got[2].cpu().numpy()
    var = np.abs(csq / S - (csum / S) ** 2).max()
    print(f"pair_sd=0: |variance| {var:.3e} (gate {4 * R.gate_corr(D, S):.3e})")
    assert var <= 4 * R.gate_corr(D, S)


def test_kernel_two_calls_accumulate_to_the_single_call():
    D, N, S = 17, 70, 37
    inp, ref = _case(D, N, S)
    single = _run(inp)
    Ya, cs, cq = _run(inp, 0, 20)
    Yb, cs, cq = _run(inp, 20, S, out=(cs, cq))
    split = (torch.cat([Ya, Yb]), cs, cq)
    _check(split, ref, D, S, "split 20 + 17")
    g = R.gate_corr(D, S)
    assert torch.equal(split[0], single[0])
    assert float((split[1] - single[1]).abs().max()) / S <= g
    assert float((split[2] - single[2]).abs().max()) / S <= 2 * g


@pytest.mark.parametrize("D,N,S", [(17, 70, 37), (17, 256, 3)])
def test_kernel_is_deterministic(D, N, S):
    inp, _ = _case(D, N, S)
    a, b = _run(inp), _run(inp)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_kernel_unsliced_two_calls_accumulate_in_place():
    """N = 256: both calls add straight onto corr_sum / corr_sq (lower triangle and its mirror)."""
    D, N, S = 17, 256, 3
    inp, ref = _case(D, N, S)
    single = _run(inp)
    Ya, cs, cq = _run(inp, 0, 2)
    Yb, cs, cq = _run(inp, 2, S, out=(cs, cq))
    split = (torch.cat([Ya, Yb]), cs, cq)
    _check(split, ref, D, S, "unsliced split 2 + 1")
    assert torch.equal(split[0], single[0])
    assert float((split[1] - single[1]).abs().max()) / S <= R.gate_corr(D, S)
    assert float((split[2] - single[2]).abs().max()) / S <= 2 * R.gate_corr(D, S)


def test_kernel_keeps_a_non_finite_diagonal():
    """The diagonal is accumulated as exactly 1 only where the reference's expression is finite: an overflowing
    exp (cov_ii = inf) gives NaN on that diagonal entry and its row and column, as the reference does, and
    leaves the other inputs alone."""
    D, N, S = 3, 2, 2
    inp = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in R.make_inputs(D, N, S, seed=5).items()}
    inp["pair_mu"][2, 0] = 800.0                                        # pair (1, 1) at input 0: exp overflows
    _, csum, csq = (g.cpu().numpy() for g in _run(inp))
    assert np.isnan(csum[0, 1, :]).all() and np.isnan(csum[0, :, 1]).all() and np.isnan(csq[0, 1, 1])
    assert csum[0, 0, 0] == S and csum[0, 2, 2] == S and np.isfinite(csum[0, 2, 0])
    assert np.isfinite(csum[1]).all() and np.isfinite(csq[1]).all()


# ------------------------------------------------------------------------------------------------ API
def _model_from(g, D, M, N, **kw):
    from collaborative_nonstationary_multivariate_gaussian_process_amd.nmgp_dsvi import NMGP
    m = NMGP(N, D, g["z"], **kw)
    with torch.no_grad():
        for k in O.PARAM_NAMES:
            if "p_" + k in g:
                getattr(m, k).data.copy_(torch.from_numpy(np.asarray(g["p_" + k])))
    return m


def test_summarize_FY_replays_reference_noise():
    """model.pt state and the reference's recorded noise: the summaries of the reference's own samples, at the
    existing gate of this path (1e-7 relative: LU against Cholesky on a cond ~1e6 system)."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    g = G.load("sample_cases")
    S = int(g["n_sample"])
    m = _model_from(g, 2, 20, 200)
    qs = (0.025, 0.975)
    out = predict.summarize_FY(m, torch.from_numpy(g["xf"]), n_sample=S, quantiles=qs, noise_tape=g["noise_f"],
                               keep_samples=True)
    N, D = g["fy_Ys"].shape[1:]
    assert g["fy_corrs"].std(0).max() > 0.01                           # corr_sd is not vacuous
    want = {"Ys": g["fy_Ys"], "tilde_ells": g["fy_tilde_ells"], "corr_mean": g["fy_corrs"].mean(0),
            "corr_sd": g["fy_corrs"].std(0), "Y_mean": g["fy_Ys"].mean(0),
            "tilde_ell_mean": g["fy_tilde_ells"].mean(0), "Y_quantiles": np.quantile(g["fy_Ys"], qs, axis=0),
            "tilde_ell_quantiles": np.quantile(g["fy_tilde_ells"], qs, axis=0)}
    assert set(out) == set(want)
    for k, w in want.items():
        assert tuple(out[k].shape) == w.shape, k
        r = _rel(out[k], w)
        print(f"{k}: rel {r:.3e}")
        assert r < 1e-7, (k, r)
    assert out["corr_mean"].shape == (N, D, D)


def _default_model(D, M, N):
    from collaborative_nonstationary_multivariate_gaussian_process_amd.nmgp_dsvi import NMGP
    return NMGP(N, D, np.linspace(0.0, 1.0, M)), torch.linspace(0.0, 1.0, N, dtype=F64)


@pytest.mark.parametrize("which", ["golden", "D5", "golden_N300"])
def test_summarize_FY_matches_materialised_path_same_seed(which):
    """golden_N300: 300 inputs, so the kernel runs unsliced as it does at HCP / ECoG size."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    if which.startswith("golden"):
        g = G.load("sample_cases")
        m, xf, D = _model_from(g, 2, 20, 200), torch.from_numpy(g["xf"]), 2
        if which == "golden_N300":
            xf = torch.linspace(float(xf.min()), float(xf.max()), 300, dtype=F64)
    else:
        (m, xf), D = _default_model(5, 20, 13), 5
    S = 40
    torch.manual_seed(7)
    ts, ys, cs = predict.sample_FY(m, xf, S)
    torch.manual_seed(7)
    out = predict.summarize_FY(m, xf, S, keep_samples=True)
    assert torch.equal(out["tilde_ells"], ts)                            # same code, same noise
    e = float((out["corr_mean"] - cs.mean(0)).abs().max())
    print(f"{which}: corr_mean {e:.3e} (gate {2 * R.gate_corr(D, S):.3e}); Ys rel {_rel(out['Ys'], ys):.3e}")
    assert e <= 2 * R.gate_corr(D, S)
    assert _rel(out["Ys"], ys) < 1e-7


def test_summarize_FY_never_holds_the_correlation_samples():
    """A cap, not a measurement: at D = 50, N = 64, S = 256 (one chunk) the peak allocation grows by less than ONE
    (S, N, D, D) fp64 tensor (328 MB; the noise block is 180 MB).  sample_FY allocates at least three such
    tensors (cov, invstd, corr) and cannot meet the cap."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    D, M, N, S = 50, 20, 64, 256
    m, xf = _default_model(D, M, N)
    assert predict._chunk_size(S, N, M) == S
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    torch.manual_seed(3)
    out = predict.summarize_FY(m, xf, S)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    cap = S * N * D * D * 8
    print(f"peak allocation grew by {grown / 1e6:.1f} MB (cap {cap / 1e6:.1f} MB)")
    assert grown < cap
    cm = out["corr_mean"]
    assert cm.shape == (N, D, D) and out["corr_sd"].shape == (N, D, D)
    assert torch.equal(cm, cm.transpose(1, 2))
    assert float((torch.diagonal(cm, dim1=1, dim2=2) - 1.0).abs().max()) <= R.gate_corr(D, S)
    assert float(cm.abs().max()) <= 1.0 + R.gate_corr(D, S)


def test_module_level_summarize_FY_shapes_and_ordered_quantiles():
    from collaborative_nonstationary_multivariate_gaussian_process_amd import nmgp_dsvi as NM
    g = G.load("sample_cases")
    m = _model_from(g, 2, 20, 200)
    N, D, S = g["xf"].shape[0], 2, 50
    torch.manual_seed(0)
    out = NM.summarize_FY(m, g["xf"], n_sample=S, quantiles=(0.025, 0.5, 0.975))
    shapes = {"tilde_ell_mean": (N,), "tilde_ell_quantiles": (3, N), "Y_mean": (N, D), "Y_quantiles": (3, N, D),
              "corr_mean": (N, D, D), "corr_sd": (N, D, D)}
    assert set(out) == set(shapes)
    for k, shp in shapes.items():
        assert isinstance(out[k], np.ndarray) and out[k].shape == shp and np.isfinite(out[k]).all(), k
    for k in ("tilde_ell_quantiles", "Y_quantiles"):
        assert (out[k][0] <= out[k][1]).all() and (out[k][1] <= out[k][2]).all()
    assert (out["corr_sd"] >= 0).all()
