"""Host references of the fused conditional prediction of missing outputs (include/nmgp_hip.h,
nmgp_ycond_accum_f64), shared by the CPU pin and the GPU tests.

Given a sample, y(x_n) ~ N(L mu_g, L V L^T + s2 I) with V = diag(var_g + 1e-4).  Two forms of the conditional mean
and variance of the missing entries of a row given its observed ones, each with hand-written Cholesky and forward
substitution, each in np.longdouble (rounded to float64 at the end) and in plain float64:

  latent       A = V^-1 + L^T diag(w) L, b = V^-1 mu_g + L^T (w o y), A = R R^T, c = R^-1 b, w_h = R^-1 l_h,
               mu = w_h^T c, v = |w_h|^2 + s2                                  (the form the kernel computes)
  observation  mu_H + C_HO C_OO^-1 (y_O - mu_O), diag(C_HH - C_HO C_OO^-1 C_OH) with C = L V L^T + s2 I, written
               with K = M C M + (I - M) (M the observed mask as a diagonal), whose inverse restricted to O is
               C_OO^-1, so that every row has D x D matrices whatever its mask.

The gate is measured on the references, never on the kernel: e64 is the largest float64-vs-longdouble error of
either form on the very input, and gate = 16 max(e64, (D + 16) 2^-52 max(1, max |ref|)) for a collected mu or v;
with D + S + 16 for sum / S, twice that for the second moments, four times for the variance.  The factor 16 covers
the kernel's blocked MFMA summation order, as in _pcorr_ref."""
import functools

import numpy as np

from tests import _fy_ref as F
from tests import _pcorr_ref as PR

LD = np.longdouble
EPS = 2.0 ** -52
JIT = 1e-4
S2 = float(np.exp(-5.0) + JIT)
MASKS = ("random", "one_missing", "one_observed")

# (D, N, S) of the GPU kernel tests: one, two, three, four and eight tiles, a tile that is full or over by one,
# sliced and unsliced samples
SLICED = [(1, 1, 1), (2, 11, 3), (15, 5, 4), (16, 3, 2), (17, 70, 37), (33, 9, 4), (50, 9, 6), (128, 3, 5)]
UNSLICED = [(17, 256, 3), (128, 256, 2)]
GPU_SHAPES = SLICED + UNSLICED


def make_mask(D, N, kind, seed):
    """-> missing (N, D) bool.  random: 30 % missing; one_missing / one_observed: exactly one missing / observed
    output per row; each with an all-missing row 0 and, from N >= 3, an all-observed row 1 and a row 2 with a
    single observation.  first / last: the only missing output of every row is 0 / D - 1 (no special rows)."""
    g = np.random.default_rng([seed, 2, (MASKS + ("first", "last")).index(kind)])
    cols = g.integers(0, D, N)
    if kind == "random":
        miss = g.random((N, D)) < 0.3
    elif kind in ("one_missing", "first", "last"):
        miss = np.zeros((N, D), bool)
        miss[np.arange(N), {"one_missing": cols, "first": 0, "last": D - 1}[kind]] = True
        if kind != "one_missing":
            return miss
    elif kind == "one_observed":
        miss = np.ones((N, D), bool)
        miss[np.arange(N), cols] = False
    else:
        raise ValueError(kind)
    miss[0] = True
    if N >= 3:
        miss[1] = False
        miss[2] = True
        miss[2, g.integers(0, D)] = False
    return miss


def make_inputs(D, N, S, kind="random"):
    """_pcorr_ref.make_inputs (well-conditioned L) plus mu_g ~ N(0, 1), var_g ~ U(0.01, 1) (the kernel adds the
    jitter 1e-4), s2 = e^-5 + 1e-4, Y ~ N(0, 1) with the mask of `kind` as NaN; seeded from the shape."""
    seed = PR.seed_of(D, N, S)
    inp = dict(PR.make_inputs(D, N, S, seed))
    g = np.random.default_rng([seed, 1])
    inp["mu_g"] = g.standard_normal((S, N, D))
    inp["var_g"] = g.uniform(0.01, 1.0, (S, N, D))
    inp["s2"] = S2
    Y = g.standard_normal((N, D))
    inp["Y_full"] = Y.copy()
    inp["missing"] = make_mask(D, N, kind, seed)
    inp["Y_obs"] = np.where(inp["missing"], np.nan, Y)
    return inp


# ------------------------------------------------------------------------------------------------ linear algebra
def _chol(A):
    """Lower Cholesky factors of a batch (B, D, D), column by column."""
    D = A.shape[1]
    R = np.zeros_like(A)
    for j in range(D):
        v = A[:, j:, j] - np.einsum("bik,bk->bi", R[:, j:, :j], R[:, j, :j])
        d = np.sqrt(v[:, 0])
        R[:, j, j] = d
        R[:, j + 1:, j] = v[:, 1:] / d[:, None]
    return R


def _fwd(R, B):
    """R^-1 B by forward substitution, R (B, D, D) lower, B (B, D, K)."""
    X = np.zeros_like(B)
    for i in range(R.shape[1]):
        X[:, i] = (B[:, i] - np.einsum("bk,bkr->br", R[:, i, :i], X[:, :i])) / R[:, i, i][:, None]
    return X


def _gram(U, d, upper=True, blk=32):
    """U diag(d) U^T for a batch (..., D, D) of upper (or lower) triangular U, the inner index taken blk at a time
    with only the rows that are not zero there."""
    D = U.shape[-1]
    out = np.zeros_like(U)
    for k0 in range(0, D, blk):
        k1 = min(D, k0 + blk)
        rows = slice(0, k1) if upper else slice(k0, D)
        Uk = U[..., rows, k0:k1]
        out[..., rows, rows] += np.matmul(Uk * d[..., None, k0:k1], np.swapaxes(Uk, -1, -2))
    return out


def _build(inp, dt):
    """-> L (S, N, D, D), V (S, N, D), mu_g, observed mask m (N, D), y0 (N, D; 0 where missing), bad (S, N)."""
    pair_mu, pair_sd, z_p = (inp[k].astype(dt) for k in ("pair_mu", "pair_sd", "z_p"))
    S, Q, N = z_p.shape
    D = int(round((np.sqrt(8 * Q + 1) - 1) / 2))
    l = pair_mu[None] + pair_sd[None] * z_p
    Lm = np.zeros((S, N, D, D), dt)
    for q, (i, j) in enumerate(F.pairs(D)):
        Lm[:, :, i, j] = np.exp(l[:, q]) if i == j else l[:, q]
    V = inp["var_g"].astype(dt) + dt(JIT)
    diag = np.einsum("snii->sni", Lm)
    bad = ((diag == 0) | ~np.isfinite(diag)).any(-1) | (~np.isfinite(V) | ~(V > 0)).any(-1)
    Lm[bad] = np.eye(D, dtype=dt)                                 # placeholders: the bad samples are NaN at the end
    V[bad] = dt(1)
    m = ~inp["missing"]
    y0 = np.where(m, np.nan_to_num(inp["Y_obs"]), 0.0).astype(dt)
    return Lm, V, inp["mu_g"].astype(dt), m, y0, bad


def _latent(inp, dt):
    """-> mu, v (S, N, D) for EVERY output (the observed ones too), NaN where the sample is bad."""
    with np.errstate(all="ignore"):
        Lm, V, mu_g, m, y0, bad = _build(inp, dt)
        S, N, D, _ = Lm.shape
        s2 = dt(inp["s2"])
        w = (m / s2).astype(dt)                                                          # (N, D)
        A = _gram(np.swapaxes(Lm, 2, 3), np.broadcast_to(w[None], (S, N, D)))
        A[:, :, np.arange(D), np.arange(D)] += 1 / V
        b = mu_g / V + np.einsum("snki,nk->sni", Lm, w * y0)
        R = _chol(A.reshape(S * N, D, D))
        rhs = np.concatenate([np.swapaxes(Lm, 2, 3).reshape(S * N, D, D), b.reshape(S * N, D, 1)], 2)
        X = _fwd(R, rhs)
        mu = np.einsum("bjh,bj->bh", X[:, :, :D], X[:, :, D]).reshape(S, N, D)
        v = (X[:, :, :D] ** 2).sum(1).reshape(S, N, D) + s2
        mu[bad] = np.nan
        v[bad] = np.nan
    return mu, v


def _observation(inp, dt):
    """The textbook form -> mu, v (S, N, D) for every output; at an observed output the values are meaningless."""
    with np.errstate(all="ignore"):
        Lm, V, mu_g, m, y0, bad = _build(inp, dt)
        S, N, D, _ = Lm.shape
        s2 = dt(inp["s2"])
        C = _gram(Lm, V, upper=False)
        C[:, :, np.arange(D), np.arange(D)] += s2
        mean = np.einsum("snik,snk->sni", Lm, mu_g)
        md = m.astype(dt)
        K = C * md[None, :, :, None] * md[None, :, None, :]
        K[:, :, np.arange(D), np.arange(D)] += (1 - md)[None]
        G = _chol(K.reshape(S * N, D, D))
        r = (md[None] * (y0[None] - mean)).reshape(S * N, D, 1)
        MC = (C * md[None, :, :, None]).reshape(S * N, D, D)
        U = _fwd(G, np.concatenate([MC, r], 2))
        mu = mean + np.einsum("bjh,bj->bh", U[:, :, :D], U[:, :, D]).reshape(S, N, D)
        v = np.einsum("snii->sni", C) - (U[:, :, :D] ** 2).sum(1).reshape(S, N, D)
        mu[bad] = np.nan
        v[bad] = np.nan
    return mu, v


def _entries(inp, a):
    """(S, N, D) -> (S, E): the missing entries in (n, d) row-major order."""
    return a[:, inp["missing"]]


def _nanmax(a):
    a = np.abs(np.asarray(a, np.float64))
    return float(np.nanmax(a)) if np.isfinite(a).any() else 0.0


def rows_checked(D, N):
    """The inputs whose entries the host reference is computed for: all of them, or, where D N > 8192 (the
    unsliced eight-tile shape; 15 s of longdouble per mask otherwise), the special rows 0, 1, 2 and every 11th
    input after them, which reach every residue mod 8 of the kernel's placement of inputs.  The inputs are
    independent of each other in the kernel and in the reference; the kernel runs all of them."""
    return None if D * N <= 8192 else np.r_[0:3, 3:N:11]


def reference(inp, rows=None):
    """-> dict: Mu, Var (S, E') float64 from the longdouble latent form; MuL, VarL the same in longdouble; e64 the
    largest float64-vs-longdouble error of either form on the missing entries; forms the largest difference of the
    two longdouble forms; scale = max(1, max |Mu|, max |Var|); sel (E',) the positions of the E' entries among the
    E of the input (rows = None: all inputs, E' = E; else the entries of those inputs only)."""
    S, N, D = inp["mu_g"].shape
    sel = np.arange(int(inp["missing"].sum()))
    if rows is not None:
        sel = sel[np.isin(np.argwhere(inp["missing"])[:, 0], rows)]
        inp = dict(inp, pair_mu=inp["pair_mu"][:, rows], pair_sd=inp["pair_sd"][:, rows], z_p=inp["z_p"][:, :, rows],
                   mu_g=inp["mu_g"][:, rows], var_g=inp["var_g"][:, rows], missing=inp["missing"][rows],
                   Y_obs=inp["Y_obs"][rows])
    lat = [_entries(inp, a) for a in _latent(inp, LD)]
    obs = [_entries(inp, a) for a in _observation(inp, LD)]
    lat64 = [_entries(inp, a) for a in _latent(inp, np.float64)]
    obs64 = [_entries(inp, a) for a in _observation(inp, np.float64)]
    e64 = max(_nanmax(a64 - a) for a, a64 in zip(lat + obs, lat64 + obs64))
    forms = max(_nanmax(a - b) for a, b in zip(lat, obs))
    scale = max(1.0, _nanmax(lat[0]), _nanmax(lat[1]))
    return {"Mu": lat[0].astype(np.float64), "Var": lat[1].astype(np.float64), "MuL": lat[0], "VarL": lat[1],
            "e64": e64, "forms": forms, "scale": scale, "D": D, "S": S, "sel": sel}


def forms_bound(ref):
    """What the two longdouble forms may differ by."""
    return (ref["D"] + 16) * EPS * ref["scale"]


def gate(ref, S=1):
    """The gate of a collected mu or v (S = 1) or of sum / S over S samples."""
    D = ref["D"]
    return 16.0 * max(ref["e64"], (D + (S if S > 1 else 0) + 16) * EPS * ref["scale"])


def sums(ref):
    """-> mu_sum, y2_sum, f2_sum (E,) of all samples, summed in longdouble."""
    mu, v = ref["MuL"], ref["VarL"]
    return tuple(a.sum(0).astype(np.float64) for a in (mu, v + mu * mu, v - LD(S2) + mu * mu))


def log_density(y, mu, v):
    return -0.5 * (np.log(2 * np.pi * v) + (y - mu) ** 2 / v)


def lpd(y, mu, v):
    """log of the equal-weight mixture density at y (E,) of N(mu, v) (S, E), in the dtype of mu."""
    ll = log_density(y[None], mu, v)
    mx = ll.max(0)
    return mx + np.log(np.exp(ll - mx[None]).sum(0)) - np.log(mu.dtype.type(mu.shape[0]))


def gate_lpd(y, ref, g):
    """The largest change of a sample's log density under a perturbation of its (mu, v) by g, evaluated on the
    reference at the four corners; the mixture's log density is a soft maximum of the samples' and moves by no
    more than the largest of them.  Entries with a non-finite y are left out."""
    mu, v = ref["MuL"], ref["VarL"]
    ok = np.isfinite(y)
    base = log_density(y[None, ok].astype(LD), mu[:, ok], v[:, ok])
    worst = 0.0
    for dm in (-g, g):
        for dv in (-g, g):
            worst = max(worst, _nanmax(log_density(y[None, ok].astype(LD), mu[:, ok] + dm, v[:, ok] + dv) - base))
    return worst


@functools.lru_cache(maxsize=None)
def case(D, N, S, kind="random"):
    """Inputs and their reference, computed once per (shape, mask) and shared (never modified)."""
    inp = make_inputs(D, N, S, kind)
    return inp, reference(inp, rows_checked(D, N))
