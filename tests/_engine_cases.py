"""Generated DSVI step inputs at the sizes where DsviEngine changes kernels (shared by CPU and GPU tests).

The engine picks its kernels from (dtype, M, B, D): the fused prior launches (fp64, 128 <= M <= 256), the pair
streaming kernels (M % 4 == 0, B <= 32 D), the 128x128 f32 kernel (fp32, M >= 512), the KL solve form (that and
M % 128 == 0), the register-resident / fallback / blocked Cholesky (n <= 256 / 257 / above); its row kernels
stride by 64 over the M columns, by 256 in the reconstruction row, by 64 over the outputs, in 16x16 tiles in the
Gibbs K22.  The tables below sit one column past those strides and on both sides of every threshold; each case
names the path flags it is meant to select, so a moved threshold fails the sweep instead of thinning it.

Inputs: new_params with the three length scales at 0.75 / M on z = linspace(0, 1, M) (neighbouring inducing
points 4/3 length scales apart: the RBF priors' cond(K22 + 1e-4 I) stays below 10) and mu_v around
log(0.75 / M) (the Gibbs prior's length scales likewise, spread by the v sample: see CASE_SEEDS), so that the
oracle's LU inverses and the mirror's Cholesky agree to a tenth of the fp64 gates --
tests/test_engine_cases_reference.py asserts that, which leaves the gates to the kernels.  With length scales of
3 / M the two references already differ by up to 8e-10 on the loss at M = 257..600.
"""
import numpy as np
import torch

from oracle import nmgp_oracle as O

N_TOTAL = 1000.0
Flags = ("fuse_tp", "pair_stream", "big_side", "kl_solve")

# (D, M, sizes, (fuse_tp, pair_stream, big_side, kl_solve) of the fp64 engine)
FP64_CASES = [
    (2, 17, [1, 4], (False, False, False, False)),         # one column past a 16-tile; a one-row output
    (3, 65, [9, 0, 22], (False, False, False, False)),     # one column past the wave stride; an empty output
    (2, 127, [33, 30], (False, False, False, False)),      # last size below fuse_tp
    (2, 128, [33, 30], (True, True, False, False)),        # first fused size
    (2, 129, [33, 30], (True, False, False, False)),       # fused, a one-column tail in every 16 / 32-wide tile
    (3, 250, [50, 1, 40], (True, False, False, False)),    # fused; M % 4 != 0: no pair_stream
    (3, 252, [20, 1, 30], (True, True, False, False)),     # fused; pair_stream, M no multiple of 16
    (2, 257, [40, 25], (False, False, False, False)),      # past fuse_tp, past recon's 256 stride, Cholesky fallback
    (2, 257, [70, 60], (False, False, False, False)),      # the same with B > 32 D
    (2, 513, [30, 35], (False, False, False, False)),      # blocked Cholesky, odd M
    (66, 20, [2] * 66, (False, True, False, False)),       # second trip of every s < D lane loop; Q = 2211 pairs
    # beside the sweep above: M = 257 cannot stream its pairs (M % 4 != 0), so B <= 32 D against B > 32 D
    # changes no kernel there; this size past fuse_tp does stream them
    (2, 260, [40, 24], (False, True, False, False)),
]

# (D, M, sizes, flags of the fp32 engine)
FP32_CASES = [
    (2, 127, [33, 30], (False, False, False, False)),      # M below a 128-column tile, with a tail
    (2, 129, [33, 30], (False, False, False, False)),      # one column past a 128-column tile
    (3, 257, [40, 0, 25], (False, False, False, False)),   # past the 256-column stride; an empty output
    (2, 510, [30, 35], (False, False, False, False)),      # last size below big_side
    (2, 512, [30, 35], (False, False, True, True)),        # big_side + kl_solve
    (2, 514, [30, 35], (False, False, True, False)),       # big_side without kl_solve; ragged 128x128 edge of 2
    (2, 520, [90, 80], (False, False, True, False)),       # M % 4 == 0 with B > 32 D: pair_stream off
    (2, 600, [30, 35], (False, False, True, False)),       # big_side, M % 128 = 88
    # beside the sweep above: B = 65 > 32 D keeps every big_side case off the pair streaming kernels; one row
    # fewer puts the per-pair products on them beside the 128x128 factor products
    (2, 512, [30, 34], (False, True, True, True)),
]

ELBO_CASES = [(3, 65, [9, 0, 22]), (2, 129, [33, 30]), (2, 257, [40, 25])]

# Generator seed per case (0 where not listed).  sqrt_v = 0.1 randn(M, M) makes v spread by ~0.1 sqrt(M), so the
# Gibbs prior's cond(K_G22 + 1e-4 I) reaches ~1e5 from M = 250 up and the two CPU references differ by 1e-12..7e-12
# on the loss and up to 1.5e-9 on one parameter's gradient, depending on the draw (seeds 0..7, two BLAS thread
# counts).  These seeds keep that difference below a fifth of the bounds of tests/test_engine_cases_reference.py
# (loss 1e-11, gradient 1e-9) in both thread settings; seed 0 was within 2x of them at M = 260, 510 and 512.
CASE_SEEDS = {(2, 257, (40, 25)): 3, (2, 260, (40, 24)): 1, (3, 257, (40, 0, 25)): 1, (2, 510, (30, 35)): 4,
              (2, 512, (30, 35)): 6, (2, 514, (30, 35)): 5, (2, 520, (90, 80)): 4, (2, 600, (30, 35)): 2}


def case_id(case):
    D, M, sizes = case[:3]
    s = f"{sizes[0]}x{len(sizes)}" if len(sizes) > 4 else "_".join(str(n) for n in sizes)
    return f"D{D}-M{M}-{s}"


def make_case(D, M, sizes, seed=None, n_sample=1, N=N_TOTAL):
    """-> dict(p, xl, yl, z, N, noise): parameters (float64), per-output rows, inducing points, data-set size and
    the float64 noise tape of n_sample * (M + B + Q B) values; deterministic in the arguments (seed None: the
    case's seed of CASE_SEEDS).  (Draws O.new_params, which seeds torch's global generator.)"""
    assert len(sizes) == D
    if seed is None:
        seed = CASE_SEEDS.get((D, M, tuple(sizes)), 0)
    ls = float(np.log(0.75 / M))
    rng = np.random.default_rng([seed, D, M, len(sizes)] + [int(n) for n in sizes])
    p = O.new_params(D, M, seed)
    for k in ("length_scales_tildeell_log", "length_scales_L0_log", "length_scales_L1_log"):
        p[k] = torch.tensor(ls, dtype=O.DT)
    p["mu_v"] = torch.from_numpy(ls + 0.1 * rng.standard_normal(M))
    xl = [np.sort(rng.uniform(0, 1, n)) for n in sizes]
    yl = [rng.standard_normal(n) for n in sizes]
    B, Q = sum(sizes), D * (D + 1) // 2
    noise = rng.standard_normal(n_sample * (M + B + Q * B))
    return dict(p=p, xl=xl, yl=yl, z=np.linspace(0, 1, M), N=float(N), noise=noise, sizes=list(sizes))


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu().reshape(-1)
    b = torch.as_tensor(b).detach().double().cpu().reshape(-1)
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


def oracle_step(c):
    """The oracle's loss, intermediates and autograd gradients of a case (the tape must be used up)."""
    q = {k: v.clone().requires_grad_() for k, v in c["p"].items()}
    tape = O.TapeNoise(c["noise"])
    loss, inter = O.forward(q, c["xl"], c["yl"], c["z"], c["N"], tape)
    loss.backward()
    assert tape.done()
    return float(loss.detach()), inter, {k: q[k].grad for k in O.PARAM_NAMES}


def mirror_step(c):
    from tests import dsvi_mirror as MR
    x = torch.from_numpy(np.concatenate(c["xl"]))
    y = torch.from_numpy(np.concatenate(c["yl"]))
    return MR.forward_backward({k: v.clone() for k, v in c["p"].items()}, x, y, c["sizes"],
                               torch.from_numpy(c["z"]), c["N"], torch.from_numpy(c["noise"]))


def unflatten(eng, flat):
    out = {}
    for k in O.PARAM_NAMES:
        o, shp = eng.offs[k]
        n = int(np.prod(shp)) if shp else 1
        out[k] = flat[o:o + n].reshape(shp).cpu()
    return out


def grad_errs(gd, ref):
    """(whole-gradient rel-norm, {parameter: rel-norm} over the parameters with a non-zero reference gradient)."""
    whole = rel(torch.cat([gd[k].reshape(-1).double() for k in O.PARAM_NAMES]),
                torch.cat([ref[k].reshape(-1) for k in O.PARAM_NAMES]))
    return whole, {k: rel(gd[k], ref[k]) for k in O.PARAM_NAMES if float(ref[k].norm()) > 0}


def intermediate_errs(eng, grad, loss, gr, it):
    """Kernel-by-kernel rel-norm errors of an engine after forward_backward against the mirror's
    (loss, gradients, intermediates) of the same step: projections, inverses, the v / t-row samples, the Gibbs
    K12, the per-factor KL, the backward's R / A-bar / P-bar, the row adjoints, every gradient, the loss."""
    D = eng.D
    checks = {
        "P_t": (eng.P[0], it["P"]["t"]), "P_0": (eng.P[1], it["P"]["0"]), "P_1": (eng.P[2], it["P"]["1"]),
        "Ainv_t": (eng.Ainv[0], it["Ainv"]["t"]), "v": (eng.v, it["v"]), "ellX": (eng.ellX, it["ellX"]),
        "K_G12": (eng.K12[3], it["KG12"]), "Ainv_G": (eng.Ainv[3], it["Ainv"]["G"]), "P_G": (eng.P[3], it["P"]["G"]),
        "KL": (eng.facbuf[:eng.NF], torch.cat([it["KL"][:D], it["KL"][D + 1:], it["KL"][D:D + 1]])), "R_G": (eng.R[3], it["Rm"]["G"]), "R_0": (eng.R[1], it["Rm"]["0"]),
        "R_t": (eng.R[0], it["Rm"]["t"]), "Abar_G": (eng.Abar[3], it["Abar"]["G"]), "Abar_0": (eng.Abar[1], it["Abar"]["0"]),
        "Abar_t": (eng.Abar[0], it["Abar"]["t"]), "Pbar_G": (eng.Pbar[3], it["Pbar"]["G"]),
        "Pbar_0": (eng.Pbar[1], it["Pbar"]["0"]), "Pbar_t": (eng.Pbar[0], it["Pbar"]["t"]),
        "mbar": (eng.rowbuf[:D].t(), it["mbar"]), "sbar": (eng.rowbuf[D:2 * D].t(), it["sbar"]),
    }
    errs = {k: rel(a, b) for k, (a, b) in checks.items()}
    gd = unflatten(eng, grad)
    for k in O.PARAM_NAMES:
        if float(gr[k].norm()) > 0:
            errs["grad_" + k] = rel(gd[k], gr[k])
    errs["loss"] = abs(float(eng.out[0]) - float(loss)) / abs(float(loss))
    return errs
