"""Host restatement of the correlation-band kernels (include/nmgp_hip.h, nmgp_corr_collect_f64 and
nmgp_quantile_rows_f64) in np.longdouble, rounded to float64 at the end; shared by the CPU pin and the GPU tests.

The gates are derived, not measured:
  * gate_c(D) = (D + 16) 2^-52 per collected sample: after normalisation every term of a correlation dot product is
    at most 1 (Cauchy-Schwarz), there are D products, and exp / sqrt / fma are within an ulp or two (the argument
    of _fy_ref.gate_y);
  * the quantile kernel's order statistics are the values np.sort finds; the interpolated value is within
    GATE_LERP max(|a|, |b|) = 4 2^-52 max(|a|, |b|) of the long-double lerp (a subtraction, a product, a sum);
  * a quantile is 1-Lipschitz in the sup norm of its samples, so end to end |corr_quantiles - ref| <= gate_c(D) +
    4 2^-52 (|corr| <= 1)."""
import numpy as np

from tests import _fy_ref as F

LD = np.longdouble
EPS = 2.0 ** -52
GATE_LERP = 4 * EPS


def all_pairs(D):
    return [(i, j) for i in range(D) for j in range(i)]


def gate_c(D):
    return (D + 16) * EPS


def collect_ref(pair_mu, pair_sd, z_p, pairs):
    """-> C (P, N, S): the correlation samples of the listed (i, j), from the full D x D matrices (L is zero above
    its diagonal) as the reference builds them; the diagonal is exactly 1 where finite."""
    S, Q, N = z_p.shape
    D = int(round((np.sqrt(8 * Q + 1) - 1) / 2))
    l = pair_mu.astype(LD)[None] + pair_sd.astype(LD)[None] * z_p.astype(LD)          # (S, Q, N)
    Lm = np.zeros((S, N, D, D), LD)
    for q, (i, j) in enumerate(F.pairs(D)):
        Lm[:, :, i, j] = np.exp(l[:, q]) if i == j else l[:, q]
    with np.errstate(all="ignore"):
        cov = np.einsum("snik,snjk->snij", Lm, Lm)
        isd = np.sqrt(LD(1) / np.einsum("snii->sni", cov))
        out = np.empty((len(pairs), N, S), np.float64)
        for p, (i, j) in enumerate(pairs):
            c = (cov[:, :, i, j] * isd[:, :, i] * isd[:, :, j]).astype(np.float64)     # (S, N)
            if i == j:
                c = np.where(np.isfinite(c), 1.0, np.nan)
            out[p] = c.T
    return out


def quantile_rows_ref(C, qs):
    """(rows, S) -> (len(qs), rows): np.quantile's linear method on the sorted rows, lerp in long double; a row with
    a NaN is NaN, w == 0 returns the order statistic itself."""
    C = np.asarray(C, np.float64)
    rows, S = C.shape
    srt = np.sort(C, axis=1)
    bad = np.isnan(C).any(axis=1)
    out = np.empty((len(qs), rows), np.float64)
    with np.errstate(all="ignore"):
        for k, q in enumerate(qs):
            pos = float(q) * (S - 1)
            lo = min(max(int(np.floor(pos)), 0), S - 1)
            hi = min(lo + 1, S - 1)
            w = LD(pos - lo)
            a, b = srt[:, lo].astype(LD), srt[:, hi].astype(LD)
            r = a + (b - a) * w if w < 0.5 else b - (b - a) * (LD(1) - w)
            if w == 0:
                r = a
            out[k] = np.where(bad, np.nan, r.astype(np.float64))
    return out
