"""The host reference of the fused sample_FY summaries (tests/_fy_ref.py) pinned to the oracle's float64 torch
expressions (oracle/nmgp_oracle.py:382-387), and the library's refusals before launch (no GPU needed)."""
import ctypes

import numpy as np
import pytest
import torch

from collaborative_nonstationary_multivariate_gaussian_process_amd import _lib as L
from tests import _fy_ref as R

ERR_FY_ARG = -60            # include/nmgp_hip.h NMGP_ERR_FY_ARG


def _torch_literal(inp):
    """Per sample, the float64 expressions of the oracle's sample_FY tail."""
    S, D, N = inp["G"].shape
    Ys, Cs = [], []
    for s in range(S):
        l = torch.from_numpy(inp["pair_mu"] + inp["pair_sd"] * inp["z_p"][s])          # (Q, N)
        Lc = torch.zeros(D, D, N, dtype=torch.float64)
        for q, (i, j) in enumerate(R.pairs(D)):
            Lc[i, j] = torch.exp(l[q]) if i == j else l[q]
        G = torch.from_numpy(inp["G"][s])
        Ln = Lc.permute(2, 0, 1)                                                       # (N, D, D)
        F = torch.matmul(Ln, G.permute(1, 0).unsqueeze(2))[:, :, 0]
        Y = F + inp["sd_err"] * torch.from_numpy(inp["z_f"][s])
        cov = torch.matmul(Ln, Lc.permute(2, 1, 0))
        invstd = torch.sqrt(torch.diag_embed(1. / torch.diagonal(cov, dim1=-2, dim2=-1)))
        Ys.append(Y), Cs.append(torch.matmul(torch.matmul(invstd, cov), invstd))
    return torch.stack(Ys).numpy(), torch.stack(Cs).numpy()


@pytest.mark.parametrize("D,N,S", [(1, 4, 3), (2, 7, 5), (5, 6, 9)])
def test_fy_ref_matches_oracle_expressions(D, N, S):
    inp = R.make_inputs(D, N, S, seed=100 + D)
    Y, csum, csq, A = R.fy_ref(**inp)
    Yt, Ct = _torch_literal(inp)
    g = R.gate_corr(D, S)
    e_sum = np.abs(csum / S - Ct.mean(0)).max()
    e_sq = np.abs(csq / S - (Ct * Ct).mean(0)).max()
    e_var = np.abs((csq / S - (csum / S) ** 2) - Ct.var(0)).max()
    e_y = (np.abs(Y - Yt) / A).max()
    print(f"D={D} N={N} S={S}: corr_sum {e_sum:.3e} (gate {g:.3e}) corr_sq {e_sq:.3e} var {e_var:.3e} "
          f"Y/A {e_y:.3e} (gate {R.gate_y(D):.3e})")
    assert e_sum <= g
    assert e_sq <= 2 * g
    assert e_var <= 4 * g
    assert e_y <= R.gate_y(D)
    assert Y.shape == (S, N, D) and csum.shape == csq.shape == (N, D, D) and A.shape == (S, N, D)


def test_fy_accum_refuses_bad_arguments_before_launch():
    """D outside 1..128, a negative count, a NULL pointer, a short row stride and a missing workspace return
    NMGP_ERR_FY_ARG; S = 0 or N = 0 returns 0.  Nothing is launched in any of these (fake pointers, no GPU)."""
    lib = L.lib()
    fake = ctypes.c_void_p(0x1000)

    def call(D, N, S, ld=None, ptr=fake, ws=None, ws_bytes=0):
        return lib.nmgp_fy_accum_f64(ptr, fake, N if ld is None else ld, fake, fake, fake, 1 << 20, 0.1, D, N, S,
                                     fake, fake, fake, ws, ws_bytes, None)

    assert call(0, 4, 3) == ERR_FY_ARG
    assert call(129, 4, 3) == ERR_FY_ARG
    assert call(-1, 4, 3) == ERR_FY_ARG
    assert call(5, -1, 3) == ERR_FY_ARG
    assert call(5, 4, -1) == ERR_FY_ARG
    assert call(5, 4, 0) == 0
    assert call(5, 0, 3) == 0
    assert call(5, 4, 3, ptr=None) == ERR_FY_ARG
    assert call(5, 4, 3, ld=3) == ERR_FY_ARG
    # N = 4 inputs cannot fill the chip: the 3 samples are sliced and need a workspace
    need = lib.nmgp_fy_workspace_size(5, 4, 3)
    assert need == 3 * 4 * 2 * 25 * 8
    assert call(5, 4, 3) == ERR_FY_ARG
    assert call(5, 4, 3, ws=fake, ws_bytes=need - 1) == ERR_FY_ARG
    assert lib.nmgp_fy_workspace_size(5, 256, 3) == 0
    assert lib.nmgp_fy_workspace_size(5, 4, 1) == 0
