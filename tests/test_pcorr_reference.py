"""The host references of the fused partial correlations (tests/_pcorr_ref.py) pinned to the correlations of the
sample_FY path (tests/_fy_ref.py, the golden file), the conditioning of the GPU tests' inputs, and the library's
refusals before launch (no GPU needed)."""
import ctypes

import numpy as np
import pytest

from collaborative_nonstationary_multivariate_gaussian_process_amd import _lib as L
from tests import _fy_ref as R
from tests import _golden as G
from tests import _pcorr_ref as PR

ERR_PCORR_ARG = -63         # include/nmgp_hip.h NMGP_ERR_PCORR_ARG


@pytest.mark.parametrize("D,N,S", PR.GPU_SHAPES)
def test_inputs_of_the_gpu_shapes_are_well_conditioned(D, N, S):
    """A condition on the inputs, not on any code under test: max |L^-1| <= 16, everything float64 computes is
    finite.

    make_inputs draws again where the first draw misses the bound (three of these shapes: 19.8, 16.9, 20.9 at
    the first draw); this test recomputes the figure by the forward substitution the references use."""
    inp = PR.make_inputs(D, N, S, PR.seed_of(D, N, S))
    pc, winf = PR._pcorr(inp["pair_mu"], inp["pair_sd"], inp["z_p"], np.float64)
    print(f"D={D} N={N} S={S}: max|L^-1| {winf:.3g}")
    assert np.isfinite(pc).all()
    assert winf <= PR.BOUND_WINF
    assert np.abs(pc).max() <= 1.0 + 64 * PR.EPS


@pytest.mark.parametrize("D,N,S", [(2, 7, 5), (5, 6, 9), (17, 4, 3)])
def test_pcorr_ref_is_the_normalised_inverse_of_the_correlation_matrix(D, N, S):
    """Scale invariance: the partial correlations of the covariance L L^T, by forward substitution in longdouble,
    equal those of the CORRELATION matrix of _fy_ref.fy_ref (cov -> invstd -> corr; one sample per call, so that
    corr_sum is the sample's correlation matrix) inverted by np.linalg.inv in float64."""
    inp = PR.make_inputs(D, N, S, seed=100 + D)
    _, _, pc, _ = PR.pcorr_ref(inp["pair_mu"], inp["pair_sd"], inp["z_p"])
    e64 = PR.e64_of(PR.pcorr_f64(inp["pair_mu"], inp["pair_sd"], inp["z_p"]), pc)
    corr = np.stack([R.fy_ref(inp["pair_mu"], inp["pair_sd"], inp["G"][s:s + 1], inp["z_p"][s:s + 1],
                              inp["z_f"][s:s + 1], inp["sd_err"])[1] for s in range(S)])      # (S, N, D, D)
    cond = float(np.linalg.cond(corr).max())
    want = PR.from_corr(corr)
    e = float(np.abs(pc - want).max())
    gate = 16 * max(e64, D * PR.EPS * cond)
    print(f"D={D} N={N} S={S}: cond2(corr) {cond:.3g} e64 {e64:.3e} |ref - inv(corr)| {e:.3e} (gate {gate:.3e})")
    assert e <= gate
    i = np.arange(D)
    assert (pc[:, :, i, i] == 1.0).all() and np.array_equal(pc, np.swapaxes(pc, 2, 3))


def test_at_two_outputs_the_partial_correlation_is_the_golden_correlation():
    """D = 2: there is nothing to condition on, so the partial correlation computed from the reference's recorded
    fy_corrs by the normalised negative inverse is fy_corrs[:, :, 1, 0] itself (8 ulp), diagonal 1."""
    c = G.load("sample_cases")["fy_corrs"]                                # (S, N, 2, 2)
    assert c.shape[2:] == (2, 2)
    pc = PR.from_corr(c)
    u = float((np.abs(pc[:, :, 1, 0] - c[:, :, 1, 0]) / np.spacing(np.abs(c[:, :, 1, 0]))).max())
    print(f"golden fy_corrs: pcorr_10 vs corr_10 {u:.2f} ulp")
    assert u <= 8
    assert (pc[:, :, 0, 0] == 1.0).all() and (pc[:, :, 1, 1] == 1.0).all()


@pytest.mark.parametrize("mu", [800.0, -800.0])
def test_a_non_finite_or_zero_diagonal_makes_that_sample_nan_at_that_input_only(mu):
    """exp(800) = inf, exp(-800) = 0 in float64: every entry at that input is NaN (the diagonal, the sums), the
    other input is finite.  (In longdouble the exp neither over- nor underflows: the rule is stated on the float64
    L the kernel builds, so the float64 run is the one that must show it, and the longdouble run is checked on the
    clean input.)"""
    D, N, S = 3, 2, 2
    inp = PR.make_inputs(D, N, S, seed=5)
    inp["pair_mu"][2, 0] = mu                                            # pair (1, 1) at input 0
    pc = PR.pcorr_f64(inp["pair_mu"], inp["pair_sd"], inp["z_p"])
    assert np.isnan(pc[:, 0]).all()
    assert np.isfinite(pc[:, 1]).all() and (pc[:, 1, [0, 1, 2], [0, 1, 2]] == 1.0).all()
    psum, psq, ref, _ = PR.pcorr_ref(inp["pair_mu"], inp["pair_sd"], inp["z_p"])
    assert np.isfinite(ref[:, 1]).all() and np.isfinite(psum[1]).all() and np.isfinite(psq[1]).all()
    assert np.abs(ref[:, 1] - pc[:, 1]).max() <= 64 * PR.EPS


def _call(lib, D=5, N=4, S=3, ld=None, z_stride=1 << 20, mu="fake", sd="fake", z="fake", psum="fake", psq="fake",
          pi="fake", pj="fake", P=2, C="fake", ld_c=3, s_off=0, ws="fake", ws_bytes=None):
    fake = ctypes.c_void_p(0x1000)
    p = lambda v: fake if v == "fake" else v
    if ws_bytes is None:
        ws_bytes = lib.nmgp_pcorr_workspace_size(D, N, S)
    return lib.nmgp_pcorr_accum_f64(p(mu), p(sd), N if ld is None else ld, p(z), z_stride, D, N, S, p(psum), p(psq),
                                    p(pi), p(pj), P, p(C), ld_c, s_off, p(ws), ws_bytes, None)


def test_pcorr_accum_refuses_bad_arguments_before_launch():
    """Every case of the header's list returns NMGP_ERR_PCORR_ARG, S = 0 or N = 0 returns 0; nothing is launched in
    any of these (fake pointers, no GPU)."""
    lib = L.lib()
    for D in (0, 129, -1):
        assert _call(lib, D=D) == ERR_PCORR_ARG
    assert _call(lib, N=-1) == ERR_PCORR_ARG
    assert _call(lib, S=-1) == ERR_PCORR_ARG
    assert _call(lib, P=-1) == ERR_PCORR_ARG
    assert _call(lib, ld=3) == ERR_PCORR_ARG
    assert _call(lib, z_stride=-1) == ERR_PCORR_ARG
    for k in ("mu", "sd", "z"):
        assert _call(lib, **{k: None}) == ERR_PCORR_ARG
    assert _call(lib, psum=None, psq=None, P=0) == ERR_PCORR_ARG         # neither sums nor a pair list
    assert _call(lib, psum=None) == ERR_PCORR_ARG                        # exactly one of the sums
    assert _call(lib, psq=None) == ERR_PCORR_ARG
    for k in ("pi", "pj", "C"):
        assert _call(lib, **{k: None}) == ERR_PCORR_ARG
    assert _call(lib, ld_c=2) == ERR_PCORR_ARG
    assert _call(lib, s_off=5, ld_c=7) == ERR_PCORR_ARG
    assert _call(lib, s_off=-1, ld_c=8) == ERR_PCORR_ARG
    assert _call(lib, S=0) == 0
    assert _call(lib, N=0) == 0
    assert _call(lib, S=0, psum=None, psq=None) == 0                     # collect only
    # N = 4 inputs cannot fill the chip: the 3 samples are sliced and the sums need a workspace
    need = lib.nmgp_pcorr_workspace_size(5, 4, 3)
    assert need == 3 * 4 * 2 * 25 * 8
    assert _call(lib, ws=None) == ERR_PCORR_ARG
    assert _call(lib, ws_bytes=need - 1) == ERR_PCORR_ARG
    assert lib.nmgp_pcorr_workspace_size(5, 256, 3) == 0
    assert lib.nmgp_pcorr_workspace_size(5, 4, 1) == 0
    assert lib.nmgp_pcorr_workspace_size(0, 4, 3) == 0 and lib.nmgp_pcorr_workspace_size(129, 4, 3) == 0
