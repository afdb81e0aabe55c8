"""The host references of the correlation-band kernels (tests/_corrq_ref.py) pinned to np.quantile and to the oracle's
float64 torch expressions (oracle/nmgp_oracle.py:382-387), and the library's refusals before launch (no GPU)."""
import ctypes

import numpy as np
import pytest
import torch

from collaborative_nonstationary_multivariate_gaussian_process_amd import _lib as L
from tests import _corrq_ref as CR
from tests import _fy_ref as R
from tests import _golden as G

ERR_CORRQ_ARG = -62         # include/nmgp_hip.h NMGP_ERR_CORRQ_ARG
QS = (0.0, 0.025, 0.5, 0.975, 1.0)


def _ulps(got, want, C, qs):
    """|got - want| in ulps of max(|a|, |b|), the order statistics a quantile is interpolated between: np.quantile
    rounds b - a, its product and the sum in float64, so where a and b cancel (a band that straddles 0) its own
    error is an ulp of the operands, not of the small result.  C: (rows, S)."""
    S = C.shape[1]
    srt = np.sort(C, axis=1)
    lo = [min(max(int(np.floor(q * (S - 1))), 0), S - 1) for q in qs]
    scale = np.stack([np.maximum(np.abs(srt[:, l]), np.abs(srt[:, min(l + 1, S - 1)])) for l in lo])
    return np.abs(got - want) / np.maximum(np.spacing(scale), np.finfo(np.float64).tiny)


@pytest.mark.parametrize("rows,S", [(5, 1), (4, 2), (7, 3), (3, 64), (6, 257), (2, 1000)])
def test_quantile_rows_ref_matches_numpy(rows, S):
    C = np.random.default_rng(10 * rows + S).standard_normal((rows, S))
    got = CR.quantile_rows_ref(C, QS)
    want = np.quantile(C, QS, axis=1)
    u = _ulps(got, want, C, QS).max()
    print(f"rows={rows} S={S}: {u:.2f} ulp")
    assert got.shape == (len(QS), rows) and u <= 4
    assert np.array_equal(got[0], C.min(1)) and np.array_equal(got[-1], C.max(1))
    if S % 2:
        assert np.array_equal(got[2], np.sort(C, 1)[:, S // 2])


def test_quantile_rows_ref_matches_numpy_on_the_golden_correlations():
    c = G.load("sample_cases")["fy_corrs"][:, :, 1, 0]                   # (S = 3, N = 11)
    assert c.shape == (3, 11)
    C = np.ascontiguousarray(c.T)
    got = CR.quantile_rows_ref(C, QS)
    want = np.quantile(c, QS, axis=0)
    u = _ulps(got, want, C, QS).max()
    print(f"golden fy_corrs[:, :, 1, 0]: {u:.2f} ulp")
    assert u <= 4


def test_quantile_rows_ref_nan_row_and_infinities():
    C = np.array([[3.0, 1.0, 2.0], [1.0, np.nan, 0.0], [np.inf, -np.inf, 5.0]])
    got = CR.quantile_rows_ref(C, (0.0, 0.5, 1.0))
    assert np.array_equal(got[:, 0], [1.0, 2.0, 3.0])
    assert np.isnan(got[:, 1]).all()
    assert np.array_equal(got[:, 2], [-np.inf, 5.0, np.inf])


def _torch_literal(inp):
    """Per sample, the float64 expressions of the oracle's sample_FY tail -> corr (S, N, D, D)."""
    S, D, N = inp["G"].shape
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


@pytest.mark.parametrize("D,N,S", [(1, 4, 3), (2, 7, 5), (5, 6, 9)])
def test_collect_ref_matches_oracle_expressions(D, N, S):
    inp = R.make_inputs(D, N, S, seed=100 + D)
    pairs = CR.all_pairs(D) + [(0, 0), (0, D - 1), (D - 1, D - 1)]
    C = CR.collect_ref(inp["pair_mu"], inp["pair_sd"], inp["z_p"], pairs)
    Ct = _torch_literal(inp)
    assert C.shape == (len(pairs), N, S)
    e = max(np.abs(C[p] - Ct[:, :, i, j].T).max() for p, (i, j) in enumerate(pairs))
    print(f"D={D} N={N} S={S}: {e:.3e} (gate {CR.gate_c(D):.3e})")
    assert e <= CR.gate_c(D)
    for p, (i, j) in enumerate(pairs):
        if i == j:
            assert (C[p] == 1.0).all()


def _collect(lib, D=5, N=4, S=3, P=2, ld=None, ld_c=None, s_off=0, ptr=ctypes.c_void_p(0x1000), z_stride=1 << 20):
    fake = ctypes.c_void_p(0x1000)
    return lib.nmgp_corr_collect_f64(ptr, fake, N if ld is None else ld, fake, z_stride, fake, fake, P, D, N, S, fake,
                                     s_off + S if ld_c is None else ld_c, s_off, None)


def _quantile(lib, rows=4, S=3, ld=None, qs=(0.5,), ptr=ctypes.c_void_p(0x1000), nq=None):
    fake = ctypes.c_void_p(0x1000)
    arr = (ctypes.c_double * max(1, len(qs)))(*qs)
    return lib.nmgp_quantile_rows_f64(ptr, rows, S, S if ld is None else ld, ctypes.cast(arr, ctypes.c_void_p),
                                      len(qs) if nq is None else nq, fake, None)


def test_corr_collect_refuses_bad_arguments_before_launch():
    """Fake pointers, no GPU: every refusal comes before a launch."""
    lib = L.lib()
    for D in (0, 129, -1):
        assert _collect(lib, D=D) == ERR_CORRQ_ARG
    assert _collect(lib, N=-1) == ERR_CORRQ_ARG
    assert _collect(lib, S=-1, ld_c=8) == ERR_CORRQ_ARG
    assert _collect(lib, P=-1) == ERR_CORRQ_ARG
    assert _collect(lib, ptr=None) == ERR_CORRQ_ARG
    assert _collect(lib, ld=3) == ERR_CORRQ_ARG
    assert _collect(lib, ld_c=2) == ERR_CORRQ_ARG
    assert _collect(lib, s_off=5, ld_c=7) == ERR_CORRQ_ARG
    assert _collect(lib, s_off=-1, ld_c=8) == ERR_CORRQ_ARG
    assert _collect(lib, z_stride=-1) == ERR_CORRQ_ARG
    for zero in ("N", "S", "P"):
        assert _collect(lib, **{zero: 0}) == 0


def test_quantile_rows_refuses_bad_arguments_before_launch():
    lib = L.lib()
    max_S = lib.nmgp_quantile_rows_max_S()
    assert max_S >= 4096
    assert _quantile(lib, rows=-1) == ERR_CORRQ_ARG
    assert _quantile(lib, S=-1, ld=4) == ERR_CORRQ_ARG
    assert _quantile(lib, nq=-1) == ERR_CORRQ_ARG
    assert _quantile(lib, ptr=None) == ERR_CORRQ_ARG
    assert _quantile(lib, ld=2) == ERR_CORRQ_ARG
    assert _quantile(lib, S=max_S + 1) == ERR_CORRQ_ARG
    for q in (-1e-9, 1.0 + 1e-9, float("nan")):
        assert _quantile(lib, qs=(0.5, q)) == ERR_CORRQ_ARG
    assert _quantile(lib, rows=0) == 0
    assert _quantile(lib, S=0) == 0
    assert _quantile(lib, qs=()) == 0
