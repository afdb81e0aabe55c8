"""Host reference of the local length-scale / noise pre-estimation (csrc/preest.hip, pre_nmgp.py).  It reads nothing
from the kernel: the neighbour rule, the eigen form of the window likelihood (float64 through LAPACK and long double
through a cyclic Jacobi written here), the fixed search of the kernel restated in numpy, and the gates.

Model of one window (code/pre_nmgp.py:48-56): vec(Y_loc) ~ N(0, K(ell) (x) B + s I) with K the RBF kernel of the P
window inputs and B = Y^T Y / (N - 1) of ALL complete rows.  With B = V_B diag(mu) V_B^T and K = V_K diag(lam) V_K^T,
  nll(log s, log ell) = 1/2 sum_pd [ log G_pd + E_pd / G_pd ] + 1/2 P D log 2 pi,
  G_pd = lam_p mu_d + s,  E = T o T,  T = V_K^T (Y_loc V_B).

Search (the same statement the kernel implements): log ell in [log(delta / 4), log(16 span)], log s in
log(mean mu) + [-14, 2]; 32 log-ell nodes, at each the profile over s (33 nodes, then a safeguarded Newton in the
bracket one node either side of the best, step <= 1e-10 or 60 iterations; the better of the Newton point and the
node is kept, the node on a tie); golden section on the profiled objective in the bracket one node either side of the
best ell node, to a width of 1e-9 or 64 iterations; the answer is the best of the node and the two final interior
points, the node on a tie -- so an optimum on a box edge is returned as the edge itself.
"""
import math

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
N_ELL, N_S = 32, 33
S_BOX = (-14.0, 2.0)
NEWTON_ITERS, NEWTON_STEP = 60, 1e-10
GOLDEN_ITERS, GOLDEN_WIDTH = 64, 1e-9
GOLDEN_R = 0.6180339887498949
FLAG_ELL_LO, FLAG_ELL_HI, FLAG_S_LO, FLAG_S_HI, FLAG_JACOBI, FLAG_DEGENERATE = 1, 2, 4, 8, 16, 32
P_MIN, P_MAX, D_MAX = 3, 32, 128


# ------------------------------------------------------------------------------------------------ data plumbing
def prepare(x, Y):
    """Complete rows only -> dict(x, Y, B, L, mu, VB, Yrot): what pre_estimation_partial computes before the launch."""
    x = np.asarray(x, np.float64).reshape(-1)
    Y = np.asarray(Y, np.float64)
    keep = ~np.isnan(Y).any(axis=1)
    x, Y = x[keep], Y[keep]
    N = Y.shape[0]
    B = Y.T.dot(Y) / (N - 1)
    mu, VB = np.linalg.eigh(B)
    return dict(x=x, Y=Y, B=B, L=np.linalg.cholesky(B), mu=mu, VB=VB, Yrot=Y.dot(VB))


def neighbours(x, z_m, P):
    """The P rows with the smallest |x_n - z_m|, ties to the lower row index, returned in ascending row order."""
    dist = np.abs(np.asarray(x, np.float64) - float(z_m))
    order = np.argsort(dist, kind="stable")[:P]
    return np.sort(order).astype(np.int32)


def no_tie_at(x, z_m, P):
    """True where the P-th and (P + 1)-th smallest distances differ (the P nearest rows are then a unique set)."""
    d = np.sort(np.abs(np.asarray(x, np.float64) - float(z_m)))
    return P >= d.size or d[P - 1] != d[P]


def seq_mean(v):
    """The mean as a left-to-right sum (the kernel's order)."""
    s = 0.0
    for a in np.asarray(v, np.float64):
        s += float(a)
    return s / len(v)


def window_box(xs, mu):
    """(lo_ell, hi_ell, lo_s, hi_s) of the search, or None for a degenerate window (span 0)."""
    xs = np.sort(np.asarray(xs, np.float64))
    span = xs[-1] - xs[0]
    if not span > 0.0:
        return None
    gaps = np.diff(xs)
    delta = gaps[gaps > 0.0].min()
    c = math.log(seq_mean(mu))
    return math.log(delta / 4.0), math.log(16.0 * span), c + S_BOX[0], c + S_BOX[1]


# ------------------------------------------------------------------------------------------------ the eigen form
def rbf(xs, log_ell, dtype=np.float64):
    """code/pre_nmgp.py:22-33 on one input column: divide, then difference, with the ell < 1e-8 clamp."""
    ell = np.exp(dtype(log_ell))
    if ell < 1e-8:
        ell = dtype(1e-8)
    u = np.asarray(xs, dtype) / ell
    d = u[:, None] - u[None, :]
    return np.exp(dtype(-0.5) * d * d)


def jacobi_ld(A, sweeps=60):
    """Cyclic two-sided Jacobi in long double -> (lam, V); stops after a sweep without a rotation."""
    A = np.array(A, LD)
    n = A.shape[0]
    V = np.eye(n, dtype=LD)
    eps = np.finfo(LD).eps
    for _ in range(sweeps):
        rotated = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[p, q]
                if abs(apq) <= eps * np.sqrt(abs(A[p, p] * A[q, q])) or abs(apq) < LD(1e-30):
                    continue
                tau = (A[q, q] - A[p, p]) / (2 * apq)
                t = (LD(1) if tau >= 0 else LD(-1)) / (abs(tau) + np.sqrt(1 + tau * tau))
                c = 1 / np.sqrt(1 + t * t)
                s = t * c
                rp, rq = A[p].copy(), A[q].copy()
                A[p], A[q] = c * rp - s * rq, s * rp + c * rq
                cp, cq = A[:, p].copy(), A[:, q].copy()
                A[:, p], A[:, q] = c * cp - s * cq, s * cp + c * cq
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = c * vp - s * vq, s * vp + c * vq
                rotated = True
        if not rotated:
            break
    return np.diag(A).copy(), V


def eig_terms(xs, Yrot_loc, log_ell, dtype=np.float64):
    """(lam (P,), E (P, D)) of one window at one length scale; float64 through LAPACK, long double through Jacobi."""
    K = rbf(xs, log_ell, dtype)
    if dtype is np.float64:
        lam, V = np.linalg.eigh(K)
    else:
        lam, V = jacobi_ld(K)
    T = V.T.dot(np.asarray(Yrot_loc, dtype))
    return lam, T * T


def nll_terms(lam, E, mu, log_s):
    dtype = lam.dtype.type
    G = lam[:, None] * np.asarray(mu, dtype)[None, :] + np.exp(dtype(log_s))
    return G, E


def nll_of(lam, E, mu, log_s):
    G, E = nll_terms(lam, E, mu, log_s)
    dtype = lam.dtype.type
    return dtype(0.5) * (np.log(G) + E / G).sum() + dtype(0.5) * G.size * np.log(2 * dtype(np.pi))


def nll(xs, Yrot_loc, mu, log_s, log_ell, dtype=np.float64):
    """The window's negative log-likelihood by the eigen form."""
    lam, E = eig_terms(xs, Yrot_loc, log_ell, dtype)
    return nll_of(lam, E, mu, log_s)


def gate_sum(xs, Yrot_loc, mu, log_s, log_ell):
    """sum_pd (|log G_pd| + E_pd / G_pd) of the evaluation gate, from the float64 restatement."""
    lam, E = eig_terms(xs, Yrot_loc, log_ell)
    G, E = nll_terms(lam, E, mu, log_s)
    return float((np.abs(np.log(G)) + E / G).sum())


# c of the evaluation gate: 8 x the worst |nll_f64 - nll_longdouble| / ((P + D) 2^-52 sum_pd(...)) over the fixture
# windows at their recorded BFGS points and host optima (tests/test_preest_reference.py measures and prints it):
# measured worst 1.263, at an hour-scale window.
GATE_C = 10.1


def eval_gate(xs, Yrot_loc, mu, log_s, log_ell, c=None):
    P, D = np.asarray(Yrot_loc).shape
    return (GATE_C if c is None else c) * (P + D) * EPS * gate_sum(xs, Yrot_loc, mu, log_s, log_ell)


def dense_nll(xs, Y_loc, B, log_s, log_ell):
    """The reference's objective without scipy: the dense P D x P D Gaussian (code/pre_nmgp.py:48-56)."""
    P, D = Y_loc.shape
    C = np.kron(rbf(xs, log_ell), B) + np.eye(P * D) * math.exp(log_s)
    w, U = np.linalg.eigh(C)
    t = U.T.dot(Y_loc.reshape(-1))
    return 0.5 * float(np.log(w).sum() + (t * t / w).sum()) + 0.5 * P * D * math.log(2 * math.pi)


# ------------------------------------------------------------------------------------------------ the search
def _f(G0, E, t, const):
    G = G0 + math.exp(t)
    return 0.5 * float((np.log(G) + E / G).sum()) + const


def _derivs(G0, E, t):
    s = math.exp(t)
    G = G0 + s
    r = s / G
    q = E / G
    g1 = 0.5 * float((r - q * r).sum())
    g2 = 0.5 * float((r - r * r - q * r + 2.0 * q * r * r).sum())
    return g1, g2


def profile_s(lam, E, mu, lo_s, hi_s):
    """min over log s in the box of the window nll at fixed eigen terms -> (log s, nll)."""
    G0 = lam[:, None] * np.asarray(mu, np.float64)[None, :]
    const = 0.5 * G0.size * math.log(2 * math.pi)
    h = (hi_s - lo_s) / (N_S - 1)
    node = lambda k: hi_s if k == N_S - 1 else lo_s + k * h
    kb, fb = 0, _f(G0, E, node(0), const)
    for k in range(1, N_S):
        fk = _f(G0, E, node(k), const)
        if fk < fb:
            kb, fb = k, fk
    a, b, t = node(max(kb - 1, 0)), node(min(kb + 1, N_S - 1)), node(kb)
    for _ in range(NEWTON_ITERS):
        g1, g2 = _derivs(G0, E, t)
        if g1 > 0.0:
            b = t
        else:
            a = t
        tn = t - g1 / g2 if g2 > 0.0 else float("nan")
        if not (tn > a and tn < b):
            tn = 0.5 * (a + b)
        step = abs(tn - t)
        t = tn
        if not step > NEWTON_STEP:
            break
    ft = _f(G0, E, t, const)
    if not ft < fb:
        t, ft = node(kb), fb
    return t, ft


def search(xs, Yrot_loc, mu):
    """The fixed search on one window -> dict(log_ell, log_s, nll, flags, box)."""
    box = window_box(xs, mu)
    if box is None:
        nan = float("nan")
        return dict(log_ell=nan, log_s=nan, nll=nan, flags=FLAG_DEGENERATE, box=(nan,) * 4)
    lo_e, hi_e, lo_s, hi_s = box

    def prof(le):
        lam, E = eig_terms(xs, Yrot_loc, le)
        t, f = profile_s(lam, E, mu, lo_s, hi_s)
        return t, f

    h = (hi_e - lo_e) / (N_ELL - 1)
    node = lambda j: hi_e if j == N_ELL - 1 else lo_e + j * h
    jb, (tb, fb) = 0, prof(node(0))
    for j in range(1, N_ELL):
        tj, fj = prof(node(j))
        if fj < fb:
            jb, tb, fb = j, tj, fj
    a, b = node(max(jb - 1, 0)), node(min(jb + 1, N_ELL - 1))
    c = b - GOLDEN_R * (b - a)
    d = a + GOLDEN_R * (b - a)
    (tc, fc), (td, fd) = prof(c), prof(d)
    for _ in range(GOLDEN_ITERS):
        if not b - a > GOLDEN_WIDTH:
            break
        if fc < fd:
            b, d, td, fd = d, c, tc, fc
            c = b - GOLDEN_R * (b - a)
            tc, fc = prof(c)
        else:
            a, c, tc, fc = c, d, td, fd
            d = a + GOLDEN_R * (b - a)
            td, fd = prof(d)
    le, ls, f = node(jb), tb, fb
    if fc < f:
        le, ls, f = c, tc, fc
    if fd < f:
        le, ls, f = d, td, fd
    flags = (FLAG_ELL_LO if le == lo_e else 0) | (FLAG_ELL_HI if le == hi_e else 0) | \
            (FLAG_S_LO if ls == lo_s else 0) | (FLAG_S_HI if ls == hi_s else 0)
    return dict(log_ell=le, log_s=ls, nll=f, flags=flags, box=box)


def fd_hessian_min_eig(xs, Yrot_loc, mu, log_s, log_ell, h=1e-3):
    """The smaller eigenvalue of the central-difference Hessian of the nll in (log s, log ell)."""
    f = lambda a, b: float(nll(xs, Yrot_loc, mu, a, b))
    f0 = f(log_s, log_ell)
    hss = (f(log_s + h, log_ell) - 2 * f0 + f(log_s - h, log_ell)) / (h * h)
    hee = (f(log_s, log_ell + h) - 2 * f0 + f(log_s, log_ell - h)) / (h * h)
    hse = (f(log_s + h, log_ell + h) - f(log_s + h, log_ell - h) - f(log_s - h, log_ell + h) +
           f(log_s - h, log_ell - h)) / (4 * h * h)
    return float(np.linalg.eigvalsh(np.array([[hss, hse], [hse, hee]]))[0])


_CASES, _OPTIMA = {}, {}


def golden_cases(path):
    """tests/golden/preest_cases.npz -> {name: dict(x, Y, z, bfgs_*, same_basin)}, loaded once."""
    if not _CASES:
        with np.load(path) as f:
            for name in f["names"]:
                name = str(name)
                _CASES[name] = {k.split("/", 1)[1]: f[k] for k in f.files if k.startswith(name + "/")}
                _CASES[name]["P"] = int(f["P"])
    return _CASES


def cached_estimate(key, x, Y, z, P):
    """estimate(...) computed once per key and shared by the tests; callers must not change the result."""
    if key not in _OPTIMA:
        _OPTIMA[key] = estimate(x, Y, z, P)
    return _OPTIMA[key]


def estimate(x, Y, z, P=10):
    """The whole host estimate on (x, Y) at z -> dict of arrays over the windows, plus the prepared data."""
    pre = prepare(x, Y)
    z = np.asarray(z, np.float64).reshape(-1)
    out = dict(log_ell=[], log_s=[], nll=[], flags=[], neighbours=[], box=[])
    for zm in z:
        idx = neighbours(pre["x"], zm, P)
        r = search(pre["x"][idx], pre["Yrot"][idx], pre["mu"])
        out["neighbours"].append(idx)
        for k in ("log_ell", "log_s", "nll", "flags", "box"):
            out[k].append(r[k])
    res = {k: np.asarray(v) for k, v in out.items()}
    res["pre"] = pre
    return res
