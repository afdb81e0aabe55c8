"""Host reference of the local coefficient factors (csrc/prelocal.hip, pre_nmgp.pre_estimation_local).  It reads
nothing from the kernel; the window likelihood, the fixed search and the gates are those of tests/_preest_ref.py.

Per inducing point z_m: the rows with a finite |x_n - z_m| ordered by (|x_n - z_m|, n); the fit window is the first P
rows, the covariance window the next Pc rows (hold-out) or the first Pc rows, both in ascending row order.
  S_m = Y_w^T Y_w / (Pc - 1)   (uncentred, as est_L of code/pre_nmgp.py:71),
  B_m = (1 - alpha) S_m + alpha B,   B = Y^T Y / (N - 1) of all rows,   alpha = D / (D + Pc - 1) by default,
formed here in long double from the doubles w = (1 - alpha) / (Pc - 1) and alpha; L_m = chol(B_m); then the window
likelihood of the fit rows with B_m in place of B (mu_m, V_m of B_m, Yrot_loc = Y_loc V_m).
"""
import numpy as np

from tests import _preest_ref as PR

LD = np.longdouble
FLAG_FACTOR = 64
MAX_COV_ROWS = 1024
U = 2.0 ** -53


def gamma(k):
    return k * U / (1.0 - k * U)


def synth_local(N, D, M, seed, A=None, noise=0.5):
    """The generator of tests/test_gpu_pre_estimation.py with the mixing matrix blended along the input:
    Y = sum_k lat_k(u) [(1 - w(u)) A0 + w(u) A1]_k + noise randn, w = sigmoid(20 (u - 1/2)); A0 and A1 are drawn right
    after the latent phases (or given as A = (A0, A1)); z = linspace(0.1, 0.9, M)."""
    rng = np.random.default_rng(seed)
    u = np.sort(rng.uniform(0.0, 1.0, N))
    warp = u + 1.5 * u * u
    lat = np.stack([np.sin(2 * np.pi * (k + 1.5) * warp + rng.uniform(0, 2 * np.pi)) for k in range(3)], axis=1)
    A0, A1 = (rng.standard_normal((3, D)), rng.standard_normal((3, D))) if A is None else A
    w = 1.0 / (1.0 + np.exp(-20.0 * (u - 0.5)))
    Y = (lat * (1.0 - w)[:, None]).dot(A0) + (lat * w[:, None]).dot(A1) + noise * rng.standard_normal((N, D))
    return u, Y, np.linspace(0.1, 0.9, M)


def order(x, z_m):
    """The rows with a finite distance, by (|x_n - z_m|, n) ascending."""
    dist = np.abs(np.asarray(x, np.float64) - float(z_m))
    rows = np.nonzero(np.isfinite(dist))[0]
    return rows[np.argsort(dist[rows], kind="stable")]


def windows(x, z_m, P, Pc, holdout):
    """(fit rows, covariance rows), int32 and ascending, or None when fewer than P holdout + Pc distances are
    finite."""
    o = order(x, z_m)
    if o.size < P * bool(holdout) + Pc:
        return None
    cov = o[P:P + Pc] if holdout else o[:Pc]
    return np.sort(o[:P]).astype(np.int32), np.sort(cov).astype(np.int32)


def default_alpha(D, Pc):
    return D / (D + Pc - 1.0)


def weights(D, Pc, shrink=None):
    """(w, alpha) as the doubles the host hands to the kernel."""
    alpha = default_alpha(D, Pc) if shrink is None else float(shrink)
    return (1.0 - alpha) / (Pc - 1.0), alpha


def local_B(Y, cov, B, w, alpha):
    """B_m in long double, and the elementwise size w |Y_w|^T |Y_w| + alpha |B| that its rounding bound scales."""
    Yw = np.asarray(Y, LD)[cov]
    Bl = np.asarray(B, LD)
    Bm = LD(w) * Yw.T.dot(Yw) + LD(alpha) * Bl
    size = LD(w) * np.abs(Yw).T.dot(np.abs(Yw)) + LD(alpha) * np.abs(Bl)
    return Bm, size


def window_terms(Y_fit, Bm):
    """mu_m, V_m of the float64 B_m and Yrot_loc = Y_loc V_m."""
    mu, V = np.linalg.eigh(np.asarray(Bm, np.float64))
    return mu, V, np.asarray(Y_fit, np.float64).dot(V)


_CACHE = {}


def estimate_local(x, Y, z, P, Pc, shrink=None, holdout=True, search=True):
    """The whole host estimate -> dict of per-window lists: neighbours, cov_neighbours, B_ld (long double), B_size,
    B_local (float64), L, mu, V, Yrot_loc, xs, and the search's log_ell / log_s / nll / flags / box; plus "pre"
    (tests/_preest_ref.prepare), "w", "alpha".  A window whose B_m is not positive definite has L None and the flag
    FLAG_FACTOR."""
    pre = PR.prepare(x, Y)
    z = np.asarray(z, np.float64).reshape(-1)
    D = pre["Y"].shape[1]
    w, alpha = weights(D, Pc, shrink)
    keys = ("neighbours", "cov_neighbours", "B_ld", "B_size", "B_local", "L", "mu", "V", "Yrot_loc", "xs", "log_ell",
            "log_s", "nll", "flags", "box")
    out = {k: [] for k in keys}
    for zm in z:
        fit, cov = windows(pre["x"], zm, P, Pc, holdout)
        Bld, size = local_B(pre["Y"], cov, pre["B"], w, alpha)
        Bm = np.asarray(Bld, np.float64)
        Bm = np.tril(Bm) + np.tril(Bm, -1).T
        xs = pre["x"][fit]
        mu, V, Yr = window_terms(pre["Y"][fit], Bm)
        try:
            Lm = np.linalg.cholesky(Bm)
            r = PR.search(xs, Yr, mu) if search else dict(log_ell=np.nan, log_s=np.nan, nll=np.nan, flags=0,
                                                           box=(np.nan,) * 4)
        except np.linalg.LinAlgError:
            Lm = None
            r = dict(log_ell=np.nan, log_s=np.nan, nll=np.nan, flags=FLAG_FACTOR, box=(np.nan,) * 4)
        for k, v in (("neighbours", fit), ("cov_neighbours", cov), ("B_ld", Bld), ("B_size", size), ("B_local", Bm),
                     ("L", Lm), ("mu", mu), ("V", V), ("Yrot_loc", Yr), ("xs", xs)):
            out[k].append(v)
        for k in ("log_ell", "log_s", "nll", "flags", "box"):
            out[k].append(r[k])
    for k in ("log_ell", "log_s", "nll", "flags", "box"):
        out[k] = np.asarray(out[k])
    out.update(pre=pre, w=w, alpha=alpha, z=z, P=P, Pc=Pc, holdout=bool(holdout))
    return out


def cached_estimate_local(key, x, Y, z, P, Pc, shrink=None, holdout=True):
    """estimate_local(...) computed once per key and shared by the tests; callers must not change the result."""
    if key not in _CACHE:
        _CACHE[key] = estimate_local(x, Y, z, P, Pc, shrink=shrink, holdout=holdout)
    return _CACHE[key]


# (N, D, M, P, Pc, holdout, seed): the fixture shapes.  Seed None is the rule 100 + N + D.
FIXTURES = [(64, 5, 4, 10, 33, True, None), (64, 5, 4, 10, 33, False, None), (160, 64, 2, 32, 100, True, None),
            (200, 128, 2, 32, 160, True, None), (300, 64, 2, 10, 200, True, None), (90, 17, 3, 10, 33, False, None),
            (48, 5, 3, 10, 48, False, None), (40, 1, 2, 3, 3, True, 2), (60, 2, 3, 10, 10, True, 1)]


def fixture(fx):
    """(x, Y, z, host estimate) of one fixture shape, computed once."""
    N, D, M, P, Pc, holdout, seed = fx
    x, Y, z = synth_local(N, D, M, 100 + N + D if seed is None else seed)
    return x, Y, z, cached_estimate_local(("fixture",) + tuple(fx), x, Y, z, P, Pc, holdout=holdout)


# The sign-flip data: two outputs that move together on the left of the range and against each other on the right.
SIGN_A = (np.array([[1.0, 1.0], [0.8, 0.9], [1.1, 0.7]]), np.array([[1.0, -1.0], [0.8, -0.9], [1.1, -0.7]]))


def sign_flip_case(N=200, M=5, seed=5, noise=0.15):
    return synth_local(N, 2, M, seed, A=SIGN_A, noise=noise)


_GOLDEN = {}


def golden_cases(path):
    """tests/golden/prelocal_cases.npz -> {name: dict(x, Y, z, P, Pc, bfgs_*, same_basin)}, loaded once."""
    if not _GOLDEN:
        with np.load(path) as f:
            for name in f["names"]:
                name = str(name)
                _GOLDEN[name] = {k.split("/", 1)[1]: f[k] for k in f.files if k.startswith(name + "/")}
                _GOLDEN[name]["P"], _GOLDEN[name]["Pc"] = int(f["P"]), int(f["Pc"])
    return _GOLDEN
