"""The DSVI step against the CPU oracle and the closed-form mirror at the sizes that pick its kernels.

tests/_engine_cases.py holds the cases: M one column past every stride of the row kernels (16, 64, 128, 256), on
both sides of the thresholds of DsviEngine's path flags (fuse_tp, pair_stream, big_side, kl_solve) and of the
Cholesky kernels (256 / 257 / blocked), D past the 64-lane stride over the outputs, empty and one-row outputs.
Each test first asserts the path flags its case is meant to select.  The inputs are generated
(tests/test_engine_cases_reference.py shows on the CPU that the two references agree to a tenth of the fp64 gates
on them), the gates are the project's: fp64 loss 1e-10 / gradient rel-norm 1e-8, fp32 loss 1e-3 / gradient 2e-2.

Measured on the MI355X (the tests print them as "PARITY shapes ..."), flags as fuse_tp pair_stream big_side kl_solve:

  fp64 case        flags  loss     SELBO_R  KL_W     KL_v     KL_U     gradient worst parameter
  D2-M17-1_4       0000   1.4e-16  1.1e-16  4.0e-16  0        7.1e-16  8.1e-15  1.0e-14 sigma2_L1_log
  D3-M65-9_0_22    0000   1.3e-15  1.2e-15  3.7e-16  6.6e-16  2.0e-15  6.2e-14  6.4e-14 sqrt_v
  D2-M127-33_30    0000   2.1e-13  2.2e-13  2.1e-13  4.4e-16  1.1e-15  6.2e-13  5.2e-12 sigma2_tildeell_log
  D2-M128-33_30    1100   3.4e-15  3.7e-15  3.2e-15  6.5e-16  7.9e-16  1.8e-13  1.0e-12 length_scales_tildeell_log
  D2-M129-33_30    1000   2.4e-14  2.6e-14  3.3e-15  2.1e-16  4.0e-16  2.3e-13  5.1e-11 length_scales_L1_log
  D3-M250-50_1_40  1000   3.0e-12  3.1e-12  1.0e-12  1.8e-16  2.5e-16  8.7e-12  8.7e-12 sqrt_v
  D3-M252-20_1_30  1100   1.4e-13  1.4e-13  1.7e-13  7.0e-16  1.0e-15  1.3e-12  1.9e-12 mu_W
  D2-M257-40_25    0000   9.5e-13  9.6e-13  3.1e-13  1.7e-16  4.1e-15  6.5e-12  6.5e-12 sqrt_v
  D2-M257-70_60    0000   3.0e-13  2.9e-13  1.5e-12  5.2e-16  4.9e-16  4.3e-12  4.5e-12 sigma2_tildeell_log
  D2-M513-30_35    0000   1.8e-12  1.8e-12  3.4e-12  5.4e-16  1.7e-15  1.4e-12  6.6e-12 mu_W
  D66-M20-2x66     0100   0        0        3.5e-16  1.5e-16  0        5.9e-15  3.5e-14 sqrt_U
  D2-M260-40_24    0100   2.2e-13  2.2e-13  4.2e-14  1.7e-16  9.6e-16  9.5e-13  1.1e-12 length_scales_L1_log
  intermediates against the mirror: worst stage of any case 2.7e-11 (gate 1e-7)

  fp32 case        flags  loss     gradient worst parameter
  D2-M127-33_30    0000   3.5e-06  7.3e-05  7.3e-05 sqrt_v
  D2-M129-33_30    0000   1.4e-07  9.8e-06  3.5e-04 length_scales_L1_log
  D3-M257-40_0_25  0000   8.6e-06  3.7e-05  3.7e-05 sqrt_v
  D2-M510-30_35    0000   1.8e-05  4.9e-04  4.9e-04 sqrt_v
  D2-M512-30_35    0011   5.3e-05  1.2e-03  2.6e-03 length_scales_tildeell_log
  D2-M514-30_35    0010   2.9e-05  9.6e-04  9.6e-04 sqrt_v
  D2-M520-90_80    0010   3.6e-06  1.1e-04  1.1e-04 sqrt_v
  D2-M600-30_35    0010   2.2e-05  2.8e-04  2.8e-04 sqrt_v
  D2-M512-30_34    0111   9.8e-06  4.0e-04  4.0e-04 sqrt_v

  compute_ELBO samples: D3-M65 1.6e-15, D2-M129 2.4e-14, D2-M257 1.0e-12 (per sample; gate 1e-10)

With the last column left out of the reconstruction row's dot products at M > 256 (tried once, not kept), every
fp64 case of M >= 257 fails: D2-M257-40_25 loss 6.9e-4, mu_W gradient 0.58; D2-M513 loss 1.1e-8 and mu_W 1.5e-6 while
its whole gradient, 8.2e-9, stays inside the gate -- hence the per-parameter check.  The fp32 gates do not see
one column in 257.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import nmgp_oracle as O
from tests import _engine_cases as EC

pytestmark = pytest.mark.gpu

SURVEY_FP64_LOSS, SURVEY_FP64_GRAD = 1e-10, 1e-8
FP32_LOSS, FP32_GRAD = 1e-3, 2e-2

FP64 = {EC.case_id(c): c for c in EC.FP64_CASES}
FP32 = {EC.case_id(c): c for c in EC.FP32_CASES}
ELBO = {EC.case_id(c): c for c in EC.ELBO_CASES}


@functools.lru_cache(maxsize=None)
def _case(D, M, sizes):
    """(inputs, oracle loss, oracle intermediates, oracle gradients), computed once per case and only read."""
    c = EC.make_case(D, M, list(sizes))
    return (c,) + EC.oracle_step(c)


def _run(D, M, sizes, dtype, flags):
    from collaborative_nonstationary_multivariate_gaussian_process_amd.engine import DsviEngine
    c, loss, inter, ref = _case(D, M, tuple(sizes))
    eng = DsviEngine(D, M, sum(sizes), c["z"], dtype=dtype)
    got = (eng.fuse_tp, eng.pair_stream, eng.big_side, eng.kl_solve)
    assert got == flags, f"path flags {dict(zip(EC.Flags, got))}, the case is meant for {dict(zip(EC.Flags, flags))}"
    theta = torch.cat([c["p"][k].reshape(-1) for k in O.PARAM_NAMES]).to("cuda", dtype)
    grad = torch.zeros_like(theta)
    eng.bind(theta, grad, N=c["N"])
    eng.load_batch(np.concatenate(c["xl"]), np.concatenate(c["yl"]), c["sizes"], noise=c["noise"])
    eng.forward_backward()
    torch.cuda.synchronize()
    eng.check_info()
    return c, loss, inter, ref, eng, grad


def _flag_str(eng):
    return " ".join(f"{k}={int(getattr(eng, k))}" for k in EC.Flags)


@pytest.mark.parametrize("cid", list(FP64))
def test_step_matches_oracle(cid):
    """One fp64 step: the loss, the reconstruction term and each KL term on their own (the KL terms are 1e3..1e6
    times the reconstruction term at these sizes and would hide it in the total), the whole gradient and every
    parameter's gradient against the oracle, at the project's fp64 gates."""
    D, M, sizes, flags = FP64[cid]
    c, loss, inter, ref, eng, grad = _run(D, M, sizes, torch.float64, flags)
    out = eng.out.double().cpu()
    lerr = abs(float(out[0]) - loss) / abs(loss)
    terms = {}
    for slot, name in ((1, "SELBO_R"), (2, "KL_W"), (3, "KL_v"), (4, "KL_U")):
        r = float(inter[name].detach())
        terms[name] = abs(float(out[slot]) - r) / abs(r)
    whole, errs = EC.grad_errs(EC.unflatten(eng, grad), ref)
    print(f"PARITY shapes {cid} fp64 [{_flag_str(eng)}]: loss rel {lerr:.3e}  "
          + "  ".join(f"{k} {e:.3e}" for k, e in terms.items())
          + f"  whole-gradient rel-norm {whole:.3e}  max grad rel-norm {max(errs.values()):.3e} ({max(errs, key=errs.get)})")
    assert lerr <= SURVEY_FP64_LOSS, lerr
    bad = {k: e for k, e in terms.items() if not e <= SURVEY_FP64_LOSS}
    assert not bad, f"ELBO terms {bad} (all: {terms})"
    assert whole <= SURVEY_FP64_GRAD, whole
    bad = {k: e for k, e in errs.items() if not e <= SURVEY_FP64_GRAD}
    assert not bad, f"gradient mismatch {bad} (all: {errs})"


@functools.lru_cache(maxsize=None)
def _mirror(D, M, sizes):
    return EC.mirror_step(_case(D, M, sizes)[0])


@pytest.mark.parametrize("cid", [k for k, c in FP64.items() if c[0] <= 3])
def test_intermediates_match_mirror(cid):
    """The same step kernel by kernel against the mirror (names the stage when test_step_matches_oracle fails):
    a lost tail column is an error of ~1/sqrt(M) in its stage, far above the 1e-7 gate."""
    D, M, sizes, flags = FP64[cid]
    c, _, _, _, eng, grad = _run(D, M, sizes, torch.float64, flags)
    loss, gr, it = _mirror(D, M, tuple(sizes))
    errs = EC.intermediate_errs(eng, grad, loss, gr, it)
    print(f"PARITY shapes {cid} intermediates: worst {max(errs, key=errs.get)} {max(errs.values()):.3e}")
    bad = {k: e for k, e in errs.items() if not e < 1e-7}
    assert not bad, f"mismatching intermediates {bad}; all {errs}"


@pytest.mark.parametrize("cid", list(FP32))
def test_fp32_step_within_fp32_gates(cid):
    """One fp32 step against the fp64 oracle at the project's fp32 gates (loss 1e-3, whole gradient 2e-2)."""
    D, M, sizes, flags = FP32[cid]
    c, loss, inter, ref, eng, grad = _run(D, M, sizes, torch.float32, flags)
    lerr = abs(float(eng.out[0]) - loss) / abs(loss)
    whole, errs = EC.grad_errs(EC.unflatten(eng, grad), ref)
    print(f"PARITY shapes {cid} fp32 [{_flag_str(eng)}]: loss rel {lerr:.3e}  whole-gradient rel-norm {whole:.3e}  "
          f"max grad rel-norm {max(errs.values()):.3e} ({max(errs, key=errs.get)})")
    assert lerr <= FP32_LOSS, lerr
    assert whole <= FP32_GRAD, whole


@pytest.mark.parametrize("cid", list(ELBO))
def test_elbo_sample_matches_oracle(cid):
    """compute_ELBO's samples (the reconstruction row gathers COLUMN I_n of L: dsvi_recon_kernel's ns = D - o
    branch) with N = B over 3 samples of a generated tape, the KL terms from the last one."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd.engine import DsviEngine
    D, M, sizes = ELBO[cid]
    B, S = sum(sizes), 3
    c = EC.make_case(D, M, sizes, n_sample=S, N=B)
    eng = DsviEngine(D, M, B, c["z"])
    theta = torch.cat([c["p"][k].reshape(-1) for k in O.PARAM_NAMES]).to("cuda")
    eng.bind(theta, torch.zeros_like(theta), N=B)
    per = M + B + D * (D + 1) // 2 * B
    x, y = np.concatenate(c["xl"]), np.concatenate(c["yl"])
    lps = []
    for s in range(S):
        eng.load_batch(x, y, c["sizes"], noise=c["noise"][s * per:(s + 1) * per])
        out = eng.elbo_sample(with_kl=(s == S - 1))
        lps.append(float(out[1]))
    kl = float(out[2] + out[3] + out[4])
    eng.check_info()
    tape = O.TapeNoise(c["noise"])
    elbo, ref = O.compute_ELBO(c["p"], c["xl"], c["yl"], c["z"], B, tape, n_sample=S)
    assert tape.done()
    ref = ref.numpy()
    print(f"PARITY shapes {cid} elbo: per-sample rel {np.abs((np.array(lps) - ref) / ref).max():.3e}  "
          f"elbo rel {abs(np.mean(lps) - kl - float(elbo)) / abs(float(elbo)):.3e}")
    np.testing.assert_allclose(lps, ref, rtol=1e-10)
    assert np.mean(lps) - kl == pytest.approx(float(elbo), rel=1e-10)
