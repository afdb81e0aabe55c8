"""The host reference of the correlation-spectrum kernel (tests/_spec_ref.py) pinned to mpmath at 40 digits, to its
float64 restatement and to the oracle's float64 torch expressions; the gap condition of the loadings on every GPU
shape; the parsing of `spectrum`; the library's refusals before launch (no GPU)."""
import ctypes

import numpy as np
import pytest
import torch

from collaborative_nonstationary_multivariate_gaussian_process_amd import _lib as L
from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
from tests import _cgroup_ref as GR
from tests import _fy_ref as R
from tests import _spec_ref as SR
from tests.test_cgroup_reference import _torch_literal

LD = np.longdouble
ERR_SPECTRUM_ARG = -66      # include/nmgp_hip.h NMGP_ERR_SPECTRUM_ARG
SHAPES = [(2, 11, 3), (17, 70, 37), (50, 9, 6), (128, 3, 5)]


def _corr_ld(inp):
    return GR.corr_samples(inp["pair_mu"], inp["pair_sd"], inp["z_p"], LD)


@pytest.mark.parametrize("precondition", [True, False])
@pytest.mark.parametrize("D", [2, 3, 5])
def test_long_double_jacobi_matches_mpmath(D, precondition):
    """Eigenvalues of long-double correlation matrices against mpmath.eigsy at 40 digits, to 64 D 2^-63 lambda_1; the
    squared loadings of every mode to the same bound over the mode's gap."""
    mpmath = pytest.importorskip("mpmath")
    inp = R.make_inputs(D, 2, 2, seed=40 + D)
    A = _corr_ld(inp).reshape(4, D, D)
    lam, U = SR.eigh_ld(A, nvec=D, precondition=precondition)
    mpmath.mp.dps = 40
    worst = worst_u = 0.0
    for b in range(4):
        hi = A[b].astype(np.float64)
        lo = (A[b] - hi.astype(LD)).astype(np.float64)                   # hi + lo is the long double, exactly
        M = mpmath.matrix(D, D)
        for i in range(D):
            for j in range(D):
                M[i, j] = mpmath.mpf(float(hi[i, j])) + mpmath.mpf(float(lo[i, j]))
        ev, evec = mpmath.eigsy(M)
        order = sorted(range(D), key=lambda i: -ev[i])
        want = [ev[i] for i in order]
        tol = 64 * D * 2.0 ** -63 * float(want[0])
        for r in range(D):
            l = float(lam[b, r])
            e = abs(float((mpmath.mpf(l) + mpmath.mpf(float(lam[b, r] - LD(l)))) - want[r]))
            worst = max(worst, e / tol)
            assert e <= tol, (b, r, e, tol)
            gap = min(abs(float(want[r] - want[q])) for q in range(D) if q != r)
            for d in range(D):
                eu = abs(float(U[b, d, r]) ** 2 - float(evec[d, order[r]]) ** 2)
                worst_u = max(worst_u, eu * gap / tol)
                assert eu <= tol / gap + 2.0 ** -52, (b, r, d, eu)        # the comparison itself is in float64
    print(f"D={D} precondition={precondition}: eigenvalue error / tol {worst:.3f}, loading error x gap / tol {worst_u:.3f}")


def test_sliced_matmul_matches_numpy_long_double():
    g = np.random.default_rng(1)
    X = (g.standard_normal((3, 37, 128)) * np.exp(4 * g.standard_normal((3, 37, 1)))).astype(LD) * (LD(1) + LD(2) ** -61)
    Y = g.standard_normal((3, 128, 29)).astype(LD) / LD(3)
    scale = np.matmul(np.abs(X), np.abs(Y))
    e = float((np.abs(SR.matmul_ld(X, Y) - np.matmul(X, Y)) / scale).max())
    print(f"sliced matmul vs numpy long double: {e:.3e} of sum |x| |y|")
    assert e <= 130 * 2.0 ** -64                                          # numpy's own 128 roundings


@pytest.mark.parametrize("D,N,S", SHAPES)
def test_float64_restatement_is_within_the_gate_of_long_double(D, N, S):
    inp = SR.inputs(D, N, S)
    corr = _corr_ld(inp)
    ref = SR.spectrum_of(corr)
    f64 = SR.eig_f64(corr.astype(np.float64))
    e64 = SR.e64_of(f64, ref["eig"])
    gate = SR.gate_eig(D, e64)
    print(f"D={D} N={N} S={S}: e64 {e64:.3e}, gate_eig {gate:.3e}, leading gaps {ref['gap']}")
    assert ref["eig"].shape == (D, N, S) and np.isfinite(ref["eig"]).all() and e64 <= gate
    assert (np.diff(ref["eig"], axis=0) <= 0).all()
    assert np.abs(ref["eig"].sum(0) - D).max() <= D * gate                # the trace of a correlation matrix
    eff64 = D * D / (f64 * f64).sum(0)
    assert np.abs(eff64 - ref["eff"]).max() <= SR.gate_eff(D, e64)
    assert np.abs(ref["load2"].sum(2) - S).max() <= S * (D + 4) * SR.EPS  # every mode's squared loadings sum to 1
    # the float64 loadings of the leading modes, at the kernel's gate
    corr64 = corr.astype(np.float64)
    vec = np.linalg.eigh(corr64)[1][..., ::-1]                            # (S, N, D, D), columns descending
    for r in range(min(SR.NVEC, D)):
        e = np.abs((vec[..., r] ** 2).sum(0) - ref["load2"][:, r]).max()
        assert e <= SR.gate_load(D, S, e64, ref["gap"][r]), (r, e)
    # one noise entry moved by 1e-6: some leading eigenvalue leaves the gate by far, so the check can see a fault
    z = inp["z_p"].copy()
    z[0, 1, 0] += 1e-6
    moved = SR.spectrum_of(GR.corr_samples(inp["pair_mu"], inp["pair_sd"], z, LD))["eig"]
    d = np.abs(moved - ref["eig"])[:min(SR.NVEC, D)].max()
    print(f"  a noise entry moved by 1e-6 moves a leading eigenvalue by {d:.3e}")
    assert d > 100 * gate


@pytest.mark.parametrize("D,N,S", [(2, 7, 5), (5, 6, 9), (17, 4, 3)])
def test_reference_matches_eigvalsh_of_oracle_expressions(D, N, S):
    inp = R.make_inputs(D, N, S, seed=100 + D)
    ref, e64 = SR.reference(inp)
    want = torch.linalg.eigvalsh(torch.from_numpy(_torch_literal(inp))).numpy()[..., ::-1]    # (S, N, D)
    e = np.abs(ref["eig"] - np.transpose(want, (2, 1, 0))).max()
    print(f"D={D}: reference vs eigvalsh of the oracle's expressions {e:.3e} (gate {SR.gate_eig(D, e64):.3e})")
    assert e <= SR.gate_eig(D, e64)


@pytest.mark.parametrize("D,N,S", SR.GPU_SHAPES)
def test_leading_gaps_of_the_gpu_inputs(D, N, S):
    """The condition under which the loadings are compared: on the inputs of every GPU shape the eigenvalue of each
    mode r < min(4, D) stays MIN_GAP away from every other.  Gaps of 1e-3 are read off the float64 restatement."""
    if D == 1:
        return
    inp = SR.inputs(D, N, S)
    lam = SR.eig_f64(GR.corr_samples(inp["pair_mu"], inp["pair_sd"], inp["z_p"], np.float64))      # (D, N, S)
    nv = min(SR.NVEC, D)
    gaps = [min(np.abs(lam[q] - lam[r]).min() for q in range(D) if q != r) for r in range(nv)]
    print(f"D={D} N={N} S={S}: smallest gap of the leading modes {min(gaps):.3e}")
    assert min(gaps) >= SR.MIN_GAP


# ------------------------------------------------------------------------------------------------ parsing
@pytest.mark.parametrize("bad", [0, 6, -1, 2.0, True, False, "some", "ALL", [2], (1,), np.float64(2.0)])
def test_spectrum_refused(bad):
    with pytest.raises(ValueError):
        predict._parse_spectrum(bad, 5)


def test_spectrum_accepted():
    assert predict._parse_spectrum("all", 5) == 5
    assert predict._parse_spectrum(1, 5) == 1 and predict._parse_spectrum(5, 5) == 5
    assert predict._parse_spectrum(np.int64(3), 5) == 3


def test_summarize_FY_refuses_bad_spectrum_before_any_device_work():
    """The model is never touched: a bare object passes for it."""
    class M:
        D = 5
    for bad in (0, 6, 2.0, True, "some", [2]):
        with pytest.raises(ValueError):
            predict.summarize_FY(M(), np.zeros(3), 4, spectrum=bad)


# ------------------------------------------------------------------------------------------------ refusals
FAKE = ctypes.c_void_p(0x1000)


def _spec(lib, D=5, N=4, S=3, k=2, ld=None, ld_e=None, s_off=0, z_stride=1 << 20, load=False, ws=None, ws_bytes=0,
          **null):
    p = lambda name: None if name in null else FAKE
    return lib.nmgp_corr_spectrum_f64(p("pair_mu"), p("pair_sd"), N if ld is None else ld, p("z_p"), z_stride, D, N, S,
                                      k, p("E"), s_off + S if ld_e is None else ld_e, s_off, FAKE if load else None,
                                      ws, ws_bytes, p("unconverged"), None)


def test_corr_spectrum_refuses_bad_arguments_before_launch():
    """Fake pointers, no GPU: every refusal comes before a launch."""
    lib = L.lib()
    for D in (0, 129, -1):
        assert _spec(lib, D=D, k=1) == ERR_SPECTRUM_ARG
    for k in (0, 6, -1):
        assert _spec(lib, k=k) == ERR_SPECTRUM_ARG
    assert _spec(lib, N=-1) == ERR_SPECTRUM_ARG
    assert _spec(lib, S=-1, ld_e=8) == ERR_SPECTRUM_ARG
    for name in ("pair_mu", "pair_sd", "z_p", "E", "unconverged"):
        assert _spec(lib, **{name: None}) == ERR_SPECTRUM_ARG, name
    assert _spec(lib, ld=3) == ERR_SPECTRUM_ARG
    assert _spec(lib, ld_e=2) == ERR_SPECTRUM_ARG
    assert _spec(lib, s_off=5, ld_e=7) == ERR_SPECTRUM_ARG
    assert _spec(lib, s_off=-1, ld_e=8) == ERR_SPECTRUM_ARG
    assert _spec(lib, z_stride=-1) == ERR_SPECTRUM_ARG
    # loadings of sliced samples (N < 256, S > 1) need the workspace
    need = lib.nmgp_corr_spectrum_workspace_bytes(5, 4, 3, 2)
    assert need == 3 * 4 * 2 * 5 * 8
    assert _spec(lib, load=True) == ERR_SPECTRUM_ARG
    assert _spec(lib, load=True, ws=FAKE, ws_bytes=need - 1) == ERR_SPECTRUM_ARG
    assert _spec(lib, load=True, ws=FAKE, ws_bytes=-1) == ERR_SPECTRUM_ARG
    for zero in ("N", "S"):
        assert _spec(lib, **{zero: 0}) == 0
        assert _spec(lib, load=True, **{zero: 0}) == 0


def test_corr_spectrum_workspace_bytes():
    lib = L.lib()
    f = lib.nmgp_corr_spectrum_workspace_bytes
    assert f(50, 256, 100, 4) == 0 and f(50, 800, 41, 50) == 0           # unsliced: the sums are the caller's
    assert f(50, 9, 1, 4) == 0                                            # one sample, one slice
    assert f(128, 3, 5, 128) == 5 * 3 * 128 * 128 * 8
    assert f(17, 70, 37, 3) == 7 * 70 * 3 * 17 * 8                        # 512 // 70 = 7 slices
    for bad in ((0, 4, 3, 1), (129, 4, 3, 1), (5, 4, 3, 0), (5, 4, 3, 6), (5, 0, 3, 1), (5, 4, 0, 1)):
        assert f(*bad) == 0
