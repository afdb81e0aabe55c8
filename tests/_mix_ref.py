"""Host references of the exact mixture scores (csrc/mixscore.hip): a float64 closed form, a 40-digit mpmath form,
the case builders and the gates.

Per entry the predictive is the equal-weight mixture of N(mu_s, v_s), s < S; with sigma = sqrt(v):
  A(m, v) = m erf(m / sqrt(2 v)) + sqrt(2 v / pi) exp(-m^2 / (2 v)),
  pit = mean_s Phi((y - mu_s) / sigma_s),  t1 = mean_s A(y - mu_s, v_s),
  t2 = (1 / 2 S^2) sum_s sum_t A(mu_s - mu_t, v_s + v_t),  crps = t1 - t2.

Cases come from fixed seeds, (kind, S) -> 70 entries; E < 70 takes the first E.  mpmath may be absent where the GPU
tests run, so `python -m tests._mix_ref --write` stores, per case and for both variance variants (the case's tensor
then one scalar), the inputs and the 40-digit values rounded to float64 of the first entries in
tests/golden/mix_cases.npz (two arrays per case: npz entries cost a quarter of a KB each); a case built here takes
those entries' inputs from the file, so the stored values belong to the very inputs whatever the generator of the
numpy at hand does.

Gates, measured on the references and never on the kernel: with e64 the float64-vs-40-digit error on the fixture
entries of the very case, 16 max(e64, (S + 16) 2^-52 max(1, t1 + t2)) for crps, t1 and spread and the same with 1 in
place of t1 + t2 for pit."""
import functools
import math
import os
import sys

import numpy as np
import torch

EPS = 2.0 ** -52
KINDS = ("plain", "bimodal", "tight", "replicated", "tails")
S_LIST = (1, 2, 63, 64, 65, 129, 257)       # 129: one past the kernel's tile of 128 components (s-slice and t-tile)
E_LIST = (1, 3, 70)
E_MAX = 70
PS = (1e-6, 0.025, 0.5, 0.975)
QUANTITIES = ("crps", "t1", "t2", "pit")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mix_cases.npz")
SQRT2, SQRT_2_PI, SQRT_PI = math.sqrt(2.0), math.sqrt(2.0 / math.pi), math.sqrt(math.pi)


def n_fixture(S):
    """Entries of a case that carry 40-digit values (40-digit t2 at S = 257 costs seconds per entry)."""
    return 3 if S <= 65 else 2


def scalar_var(kind):
    return 1e-4 if kind == "tight" else 0.37


def build(kind, S, E=E_MAX):
    """Mu, Var (S, E), y (E,) of a kind from its fixed seed, before the fixture's entries are put in."""
    g = np.random.default_rng(1000 * KINDS.index(kind) + S)
    Mu = g.standard_normal((S, E)) + 0.5 * g.standard_normal(E)
    Var = 0.2 + 1.3 * g.random((S, E))
    y = 1.2 * g.standard_normal(E)
    if kind == "bimodal":
        Mu[S // 2:] += 40.0
        y = y + 40.0 * (np.arange(E) % 3 == 0)
    elif kind == "tight":
        Mu *= 0.05
        Var = 1e-4 + 1e-6 * g.random((S, E))
        y *= 0.05
    elif kind == "replicated":
        Mu = np.repeat(Mu[:1], S, 0)
        Var = np.repeat(Var[:1], S, 0)
    elif kind == "tails":
        mean = Mu.mean(0)
        sd = np.sqrt((Var + Mu * Mu).mean(0) - mean * mean)
        y = mean + 30.0 * sd * np.where(np.arange(E) % 2 == 0, 1.0, -1.0)
    return np.ascontiguousarray(Mu), np.ascontiguousarray(Var), y


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(GOLDEN, allow_pickle=False)) if os.path.exists(GOLDEN) else {}


# ------------------------------------------------------------------------------------------------ float64 form
def _erf(a):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))).numpy()


def _erfc(a):
    return torch.erfc(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))).numpy()


def _sum0(a):
    """Sum over the leading axis with numpy's pairwise summation (which it uses along a contiguous axis only: a
    plain sum over a slow axis adds S^2 terms one after the other and loses S^2 2^-53 on equal terms)."""
    return np.ascontiguousarray(a.reshape(a.shape[0], -1).T).sum(1).reshape(a.shape[1:])


def A64(m, v):
    s = np.sqrt(v)
    z = m / s
    return m * _erf(z / SQRT2) + s * SQRT_2_PI * np.exp(-0.5 * z * z)


def cdf64(q, Mu, Var):
    """The mixture CDF at q (broadcast against the entries) -> (E,)."""
    return _sum0(0.5 * _erfc(-(q - Mu) / (np.sqrt(Var) * SQRT2))) / Mu.shape[0]


def pdf64(q, Mu, Var):
    z = (q - Mu) / np.sqrt(Var)
    return _sum0(np.exp(-0.5 * z * z) / np.sqrt(2.0 * math.pi * Var)) / Mu.shape[0]


def scores64(Mu, Var, y=None):
    """float64 closed form -> dict of (E,) arrays: t2 (the spread) and, with y, pit, t1 and crps."""
    Mu, Var = np.asarray(Mu, np.float64), np.broadcast_to(np.asarray(Var, np.float64), np.shape(Mu))
    S = Mu.shape[0]
    pair = A64(Mu[:, None] - Mu[None], Var[:, None] + Var[None])                # the diagonal is 2 sigma / sqrt(pi)
    out = {"t2": _sum0(pair.reshape(S * S, -1)) / (2.0 * S * S)}
    if y is not None:
        y = np.asarray(y, np.float64)
        out["pit"] = cdf64(y[None], Mu, Var)
        out["t1"] = _sum0(A64(y[None] - Mu, Var)) / S
        out["crps"] = out["t1"] - out["t2"]
    return out


def bracket64(Mu, Var, p):
    """[min_s, max_s](mu_s + z_p sigma_s) widened by 1e-12 max_s(|mu_s| + |z_p| sigma_s) -> lo, hi (E,)."""
    zp = float(torch.special.ndtri(torch.tensor(p, dtype=torch.float64)))
    c = Mu + zp * np.sqrt(Var)
    w = 1e-12 * (np.abs(Mu) + abs(zp) * np.sqrt(Var)).max(0)
    return c.min(0) - w, c.max(0) + w


def quantile64(Mu, Var, p, max_steps=200):
    """float64 bisection of the mixture CDF from bracket64 down to adjacent doubles -> q (E,), steps taken."""
    Mu, Var = np.asarray(Mu, np.float64), np.broadcast_to(np.asarray(Var, np.float64), np.shape(Mu))
    lo, hi = bracket64(Mu, Var, p)
    fa, fb = np.full(lo.shape, np.inf), np.full(lo.shape, np.inf)
    steps = 0
    for steps in range(max_steps + 1):
        mid = lo + 0.5 * (hi - lo)
        live = (mid > lo) & (mid < hi)
        if not live.any():
            break
        res = cdf64(mid[None], Mu, Var) - p
        left = live & (res < 0)
        right = live & ~(res < 0)
        lo, fa = np.where(left, mid, lo), np.where(left, -res, fa)
        hi, fb = np.where(right, mid, hi), np.where(right, res, fb)
    return np.where(fa <= fb, lo, hi), steps


def quantile_bound(q, Mu, Var, S):
    """The bound on |F(q) - p| of a q that is the root to within one spacing: 4 (f(q) spacing(q) + (S + 16) 2^-52)."""
    return 4.0 * (pdf64(q[None], Mu, Var) * np.spacing(np.abs(q)) + (S + 16) * EPS)


def single_gaussian(m, v, y):
    """CRPS, PIT and spread of ONE Gaussian N(m, v): the closed form a replicated mixture must equal."""
    s = np.sqrt(v)
    z = (y - m) / s
    Phi = 0.5 * _erfc(-z / SQRT2)
    phi = np.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    return {"crps": s * (z * (2.0 * Phi - 1.0) + 2.0 * phi - 1.0 / SQRT_PI), "pit": Phi, "t2": s / SQRT_PI}


# ------------------------------------------------------------------------------------------------ 40-digit form
def scoresmp(Mu, Var, y, dps=40):
    """The 40-digit mpmath form, entry by entry -> dict of float64 (E,) arrays crps, t1, t2, pit."""
    import mpmath as mp
    Mu, Var = np.asarray(Mu, np.float64), np.broadcast_to(np.asarray(Var, np.float64), np.shape(Mu))
    S, E = Mu.shape
    out = {k: np.empty(E) for k in ("crps", "t1", "t2", "pit")}
    with mp.workdps(dps):
        def A(m, v):
            return m * mp.erf(m / mp.sqrt(2 * v)) + mp.sqrt(2 * v / mp.pi) * mp.exp(-m * m / (2 * v))

        for e in range(E):
            mu = [mp.mpf(float(a)) for a in Mu[:, e]]
            v = [mp.mpf(float(a)) for a in Var[:, e]]
            ye = mp.mpf(float(y[e]))
            t1 = mp.fsum(A(ye - mu[s], v[s]) for s in range(S)) / S
            pit = mp.fsum(mp.erfc(-(ye - mu[s]) / mp.sqrt(2 * v[s])) / 2 for s in range(S)) / S
            tri = mp.fsum(A(mu[s] - mu[t], v[s] + v[t]) for s in range(S) for t in range(s))
            diag = mp.fsum(2 * mp.sqrt(v[s]) / mp.sqrt(mp.pi) for s in range(S))
            t2 = (2 * tri + diag) / (2 * S * S)
            out["t1"][e], out["t2"][e], out["pit"][e], out["crps"][e] = float(t1), float(t2), float(pit), float(t1 - t2)
    return out


def cdfmp(q, mu, v, dps=40):
    """40-digit mixture CDF and density of one entry at q -> (float, float)."""
    import mpmath as mp
    with mp.workdps(dps):
        q = mp.mpf(float(q))
        comps = [(mp.mpf(float(m)), mp.mpf(float(w))) for m, w in zip(mu, v)]
        F = mp.fsum(mp.erfc(-(q - m) / mp.sqrt(2 * w)) / 2 for m, w in comps)
        f = mp.fsum(mp.exp(-(q - m) ** 2 / (2 * w)) / mp.sqrt(2 * mp.pi * w) for m, w in comps)
        return float(F / len(mu)), float(f / len(mu))


# ------------------------------------------------------------------------------------------------ cases and gates
@functools.lru_cache(maxsize=None)
def case(kind, S, het=True):
    """-> dict: Mu (S, 70), Var ((S, 70), or the kind's scalar with het=False), y (70,), ref (scores64 of all 70
    entries), nf and gold (the stored 40-digit values of the first nf entries; None without the fixture file), and
    the gates gate (70,) for crps / t1 / spread and gate_pit (scalar)."""
    Mu, Var, y = build(kind, S)
    g, key, nf = _golden(), f"{kind}_{S}", n_fixture(S)
    if key + "_in" in g:                                                  # rows: Mu (S), Var (S), y (1)
        Mu[:, :nf], Var[:, :nf], y[:nf] = g[key + "_in"][:S], g[key + "_in"][S:2 * S], g[key + "_in"][2 * S]
    V = Var if het else scalar_var(kind)
    ref = scores64(Mu, V, y)
    gold = None
    e64 = e64_pit = 0.0
    if key + "_mp" in g:                                                  # (variant h / s, quantity, entry)
        gold = dict(zip(QUANTITIES, g[key + "_mp"][0 if het else 1]))
        e64 = max(float(np.abs(ref[k][:nf] - gold[k]).max()) for k in ("crps", "t1", "t2"))
        e64_pit = float(np.abs(ref["pit"][:nf] - gold["pit"]).max())
    floor = (S + 16) * EPS
    return {"kind": kind, "S": S, "Mu": Mu, "Var": V, "y": y, "ref": ref, "nf": nf, "gold": gold, "e64": e64,
            "e64_pit": e64_pit, "gate": 16.0 * np.maximum(e64, floor * np.maximum(1.0, ref["t1"] + ref["t2"])),
            "gate_pit": 16.0 * max(e64_pit, floor)}


def write():
    out = {}
    for kind in KINDS:
        for S in S_LIST:
            Mu, Var, y = build(kind, S)
            nf, key = n_fixture(S), f"{kind}_{S}"
            out[key + "_in"] = np.concatenate([Mu[:, :nf], Var[:, :nf], y[None, :nf]])
            mp = [scoresmp(Mu[:, :nf], V, y[:nf]) for V in (Var[:, :nf], scalar_var(kind))]
            out[key + "_mp"] = np.array([[m[k] for k in QUANTITIES] for m in mp])
            print(key, flush=True)
    np.savez(GOLDEN, **out)
    print(f"{GOLDEN}: {os.path.getsize(GOLDEN)} bytes")


if __name__ == "__main__":
    if "--write" in sys.argv:
        write()
