"""Host restatement of the fused sample_FY summary kernel (include/nmgp_hip.h, nmgp_fy_accum_f64) in
np.longdouble, rounded to float64 at the end; shared by the CPU pin and the GPU tests."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52


def pairs(D):
    return [(i, j) for i in range(D) for j in range(i + 1)]


def make_inputs(D, N, S, seed, sd_zero=False):
    """The issue's input distributions: pair_mu ~ N(0, 0.5^2), pair_sd ~ U(0.05, 0.5), G, z ~ N(0, 1)."""
    g = np.random.default_rng(seed)
    Q = D * (D + 1) // 2
    pair_sd = np.zeros((Q, N)) if sd_zero else g.uniform(0.05, 0.5, (Q, N))
    return {"pair_mu": 0.5 * g.standard_normal((Q, N)), "pair_sd": pair_sd, "G": g.standard_normal((S, D, N)),
            "z_p": g.standard_normal((S, Q, N)), "z_f": g.standard_normal((S, N, D)), "sd_err": 0.3}


def fy_ref(pair_mu, pair_sd, G, z_p, z_f, sd_err):
    """-> Y (S, N, D), corr_sum (N, D, D), corr_sq (N, D, D), A (S, N, D) with
    A[s, n, i] = sum_j |L_ij| |G_j| + sd_err |z_f|, the scale of Y's rounding error."""
    S, D, N = G.shape
    l = pair_mu.astype(LD)[None] + pair_sd.astype(LD)[None] * z_p.astype(LD)          # (S, Q, N)
    Lm = np.zeros((S, N, D, D), LD)
    for q, (i, j) in enumerate(pairs(D)):
        Lm[:, :, i, j] = np.exp(l[:, q]) if i == j else l[:, q]
    Gn = np.transpose(G.astype(LD), (0, 2, 1))                                          # (S, N, D)
    F = np.einsum("snij,snj->sni", Lm, Gn)
    Y = F + LD(sd_err) * z_f.astype(LD)
    A = np.einsum("snij,snj->sni", np.abs(Lm), np.abs(Gn)) + LD(abs(sd_err)) * np.abs(z_f.astype(LD))
    cov = np.einsum("snik,snjk->snij", Lm, Lm)
    isd = np.sqrt(LD(1) / np.einsum("snii->sni", cov))
    corr = cov * isd[..., :, None] * isd[..., None, :]
    return (Y.astype(np.float64), corr.sum(0).astype(np.float64), (corr * corr).sum(0).astype(np.float64),
            A.astype(np.float64))


def gate_corr(D, S):
    """|corr_sum / S - ref| bound: every term of the normalised dot product is at most 1 (Cauchy-Schwarz), D
    products and S sums, exp / fma / sqrt within an ulp or two."""
    return (D + S + 16) * EPS


def gate_y(D):
    return (D + 16) * EPS
