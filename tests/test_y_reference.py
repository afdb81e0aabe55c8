"""The host reference of the fused sample_Y summaries (tests/_y_ref.py) pinned to the oracle's float64 torch
expressions (oracle/nmgp_oracle.py:356-361), the library's refusals before launch, the binding of the two new
symbols, and summarize_Y's argument checks (no GPU needed)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from collaborative_nonstationary_multivariate_gaussian_process_amd import _lib as L
from tests import _fy_ref
from tests import _y_ref as R

ERR_Y_ARG = -61             # include/nmgp_hip.h NMGP_ERR_Y_ARG
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch_literal(inp):
    """Per sample, the float64 expressions of the oracle's sample_Y tail: the full L, its row I_n, F, Y."""
    S, D, N = inp["G"].shape
    rows, cols = torch.arange(N), torch.from_numpy(inp["I"])
    Ys, Fs, Ls = [], [], []
    for s in range(S):
        l = torch.from_numpy(inp["pair_mu"] + inp["pair_sd"] * inp["z_p"][s])          # (Q, N)
        Lc = torch.zeros(D, D, N, dtype=torch.float64)
        for q, (i, j) in enumerate(_fy_ref.pairs(D)):
            Lc[i, j] = torch.exp(l[q]) if i == j else l[q]
        G = torch.from_numpy(inp["G"][s])
        lr = Lc.permute(2, 0, 1)[rows, cols]
        F = torch.sum(lr * G.t(), 1)
        Ys.append(F + inp["sd_err"] * torch.from_numpy(inp["z_f"][s])), Fs.append(F), Ls.append(lr)
    return torch.stack(Ys), torch.stack(Fs), torch.stack(Ls)


@pytest.mark.parametrize("D,N,S", [(1, 4, 3), (2, 7, 5), (5, 6, 9)])
def test_y_ref_matches_oracle_expressions(D, N, S):
    inp = R.make_inputs(D, N, S, seed=100 + D, ids="random" if D == 5 else "blocks")
    ref = R.y_ref(**inp)
    Y, F, Lr = _torch_literal(inp)
    G = torch.from_numpy(inp["G"])
    got = {"Y": Y, "F": F, "F_sum": F.sum(0), "F_sq": (F * F).sum(0), "L_sum": Lr.sum(0), "L_sq": (Lr * Lr).sum(0),
           "G_sum": G.sum(0), "G_sq": (G * G).sum(0)}
    got = {k: v.numpy() for k, v in got.items()}
    y = torch.from_numpy(inp["y"])
    lpd = torch.logsumexp(torch.distributions.Normal(F, inp["sd_err"]).log_prob(y), 0) - np.log(S)
    res = R.errors(got, ref, D, S, lpd=lpd.numpy(), y=inp["y"], sd_err=inp["sd_err"])
    R.report(f"D={D} N={N} S={S}", res)
    for k, (ratio, err) in res.items():
        assert ratio <= 1.0, (k, ratio, err)
    assert ref["Y"].shape == ref["F"].shape == ref["A"].shape == ref["a"].shape == (S, N)
    assert ref["L_sum"].shape == (N, D) and ref["G_sum"].shape == (D, N) and ref["lpd"].shape == (N,)
    for n in range(N):
        assert (ref["L_sum"][n, inp["I"][n] + 1:] == 0).all()


def test_lpd_gate_is_small_and_plain_float64_sits_well_inside():
    """The lpd gate at the largest GPU shape: plain float64 numpy against the longdouble reference."""
    D, N, S = 17, 70, 37
    inp = R.make_inputs(D, N, S, seed=3)
    ref = R.y_ref(**inp)
    v = inp["sd_err"] ** 2
    a = -0.5 * np.log(2 * np.pi * v) - (inp["y"][None] - ref["F"]) ** 2 / (2 * v)
    m = a.max(0)
    lpd = m + np.log(np.exp(a - m).sum(0)) - np.log(S)
    gate = R.gate_lpd(ref, inp["y"], inp["sd_err"], D, S)
    ratio = float((np.abs(lpd - ref["lpd"]) / gate).max())
    print(f"lpd: worst {ratio:.3f} of its gate; largest gate {gate.max():.3e}")
    assert ratio <= 1.0 and gate.max() < 1e-9


def test_y_accum_refuses_bad_arguments_before_launch():
    """D < 1, a negative count, a NULL pointer, y without its log-sum-exp state, a short row stride and a missing
    or short workspace return NMGP_ERR_Y_ARG; S = 0 or N = 0 returns 0.  Nothing is launched in any of these
    (fake pointers, no GPU)."""
    lib = L.lib()
    fake = ctypes.c_void_p(0x1000)

    def call(D, N, S, ld=None, ptr=fake, y=None, lse_max=None, lse_sum=None, ws=None, ws_bytes=0, G_sq=fake):
        return lib.nmgp_y_accum_f64(ptr, fake, N if ld is None else ld, fake, fake, fake, 1 << 20, fake, y, 0.1,
                                    D, N, S, fake, fake, fake, fake, fake, fake, fake, G_sq, lse_max, lse_sum,
                                    ws, ws_bytes, None)

    assert call(0, 4, 3) == ERR_Y_ARG
    assert call(-1, 4, 3) == ERR_Y_ARG
    assert call(5, -1, 3) == ERR_Y_ARG
    assert call(5, 4, -1) == ERR_Y_ARG
    assert call(5, 4, 0) == 0
    assert call(5, 0, 3) == 0
    assert call(5, 4, 3, ptr=None) == ERR_Y_ARG
    assert call(5, 4, 3, G_sq=None) == ERR_Y_ARG
    assert call(5, 4, 3, ld=3) == ERR_Y_ARG
    # one tile of inputs x 6 rows cannot fill the chip: the 3 samples are sliced and need a workspace
    need = lib.nmgp_y_workspace_size(5, 4, 3)
    assert need == 3 * 4 * 6 * 4 * 8
    assert call(5, 4, 3) == ERR_Y_ARG
    assert call(5, 4, 3, ws=fake, ws_bytes=need - 1) == ERR_Y_ARG
    assert call(5, 4, 3, y=fake, lse_sum=fake, ws=fake, ws_bytes=need) == ERR_Y_ARG       # lse_max NULL
    assert call(5, 4, 3, y=fake, lse_max=fake, ws=fake, ws_bytes=need) == ERR_Y_ARG       # lse_sum NULL
    assert lib.nmgp_y_workspace_size(5, 4, 1) == 0
    # 8 tiles x 65 rows = 520 waves pass half the fill and are not sliced; 8 x 64 = 512 are cut in two
    assert lib.nmgp_y_workspace_size(64, 449, 3) == 0
    assert lib.nmgp_y_workspace_size(63, 449, 3) == 2 * 4 * 64 * 449 * 8
    sizes = [lib.nmgp_y_workspace_size(17, 70, s) for s in range(1, 80)]
    assert sizes == sorted(sizes)                                        # a full chunk's workspace covers a shorter one


def test_y_symbols_are_exported_and_bound_as_declared():
    lib = L.lib()
    src = open(os.path.join(ROOT, "include", "nmgp_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"#define\s+NMGP_ERR_Y_ARG\s+\(-61\)", src)
    for name in ("nmgp_y_workspace_size", "nmgp_y_accum_f64"):
        assert hasattr(lib, name) and name in L.exported_symbols(), name
        decl = re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(getattr(lib, name).argtypes), name


def test_summarize_Y_checks_its_arguments_before_any_device_work():
    """The checks read only model.D, so a stand-in model without a device shows that they come first."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import predict
    m = types.SimpleNamespace(D=3)
    X = [np.linspace(0, 1, 4), np.linspace(0, 1, 5)]
    with pytest.raises(ValueError):
        predict.summarize_Y(m, X, index=[0, 3])
    with pytest.raises(ValueError):
        predict.summarize_Y(m, X, index=[-1, 2])
    with pytest.raises(ValueError):
        predict.summarize_Y(m, X, quantiles=(0.025, 1.5))
    with pytest.raises(ValueError):
        predict.summarize_Y(m, X, n_sample=0)
    with pytest.raises(ValueError):
        predict.summarize_Y(m, X, Y_list=[np.zeros(4)])
    with pytest.raises(ValueError):
        predict.summarize_Y(m, X, Y_list=[np.zeros(4), np.zeros(4)])
