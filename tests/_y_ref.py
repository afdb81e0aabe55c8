"""Host restatement of the fused sample_Y summary kernel (include/nmgp_hip.h, nmgp_y_accum_f64) in np.longdouble,
rounded to float64 at the end; shared by the CPU pin and the GPU tests.  The gates are derived bounds: an fma chain
of D terms, S sums, exp / log within an ulp or two, each error relative to the sum of the absolute terms."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
ID_PATTERNS = ("blocks", "random", "zeros", "last")


def make_ids(D, N, pattern, g):
    if pattern == "blocks":                  # piecewise constant and ascending, as the API builds them from lists
        return (np.arange(N, dtype=np.int64) * D) // N
    if pattern == "random":
        return g.integers(0, D, N).astype(np.int64)
    if pattern == "zeros":
        return np.zeros(N, np.int64)
    if pattern == "last":
        return np.full(N, D - 1, np.int64)
    raise ValueError(pattern)


def make_inputs(D, N, S, seed, ids="blocks"):
    """_fy_ref's distributions: pair_mu ~ N(0, 0.5^2), pair_sd ~ U(0.05, 0.5), G, z ~ N(0, 1), sd_err = 0.3;
    z_f is (S, N); y = F[0] + 0.3 N(0, 1)."""
    g = np.random.default_rng(seed)
    Q = D * (D + 1) // 2
    inp = {"pair_mu": 0.5 * g.standard_normal((Q, N)), "pair_sd": g.uniform(0.05, 0.5, (Q, N)),
           "G": g.standard_normal((S, D, N)), "z_p": g.standard_normal((S, Q, N)),
           "z_f": g.standard_normal((S, N)), "sd_err": 0.3}
    inp["I"] = make_ids(D, N, ids, g)
    noise = g.standard_normal(N)
    inp["y"] = None
    inp["y"] = y_ref(**inp)["F"][0] + 0.3 * noise
    return inp


def rows_of_L(pair_mu, pair_sd, z_p, I):
    """(S, N, D) longdouble: row I_n of the sampled L at input n, zero in the columns j > I_n."""
    S, Q, N = z_p.shape
    D = int(round((np.sqrt(8 * Q + 1) - 1) / 2))
    Lr = np.zeros((S, N, D), LD)
    for n in range(N):
        i = int(I[n])
        q0 = i * (i + 1) // 2
        l = pair_mu[q0:q0 + i + 1, n].astype(LD)[None] + pair_sd[q0:q0 + i + 1, n].astype(LD)[None] * \
            z_p[:, q0:q0 + i + 1, n].astype(LD)
        l[:, i] = np.exp(l[:, i])
        Lr[:, n, :i + 1] = l
    return Lr


def y_ref(pair_mu, pair_sd, G, z_p, z_f, I, sd_err, y=None):
    """-> dict of float64 arrays: Y, F (S, N); F_sum, F_sq (N); L_sum, L_sq (N, D); G_sum, G_sq (D, N);
    A (S, N) = sum_j |l_j| |G_j| + sd_err |z_f|, the scale of F's and Y's rounding error; the gate scales
    mean_A, mean_A2 (N), mean_l, mean_l2 (N, D), mean_G, mean_G2 (D, N); and with y: the unrounded log densities
    a (S, N), lse (N) = log sum_s exp(a) and lpd (N) = lse - log S."""
    S, D, N = G.shape
    Lr = rows_of_L(pair_mu, pair_sd, z_p, I)
    Gn = np.transpose(G.astype(LD), (0, 2, 1))                                          # (S, N, D)
    F = (Lr * Gn).sum(2)
    Y = F + LD(sd_err) * z_f.astype(LD)
    A = (np.abs(Lr) * np.abs(Gn)).sum(2) + LD(abs(sd_err)) * np.abs(z_f.astype(LD))
    Gl = G.astype(LD)
    f64 = lambda a: np.asarray(a, LD).astype(np.float64)
    out = {"Y": f64(Y), "F": f64(F), "F_sum": f64(F.sum(0)), "F_sq": f64((F * F).sum(0)),
           "L_sum": f64(Lr.sum(0)), "L_sq": f64((Lr * Lr).sum(0)), "G_sum": f64(Gl.sum(0)),
           "G_sq": f64((Gl * Gl).sum(0)), "A": f64(A), "mean_A": f64(A.mean(0)), "mean_A2": f64((A * A).mean(0)),
           "mean_l": f64(np.abs(Lr).mean(0)), "mean_l2": f64((Lr * Lr).mean(0)),
           "mean_G": f64(np.abs(Gl).mean(0)), "mean_G2": f64((Gl * Gl).mean(0))}
    if y is not None:
        v = LD(sd_err) * LD(sd_err)
        d = np.asarray(y).astype(LD)[None] - F
        a = -LD(0.5) * np.log(LD(2) * LD(np.pi) * v) - d * d / (LD(2) * v)
        m = a.max(0)
        lse = m + np.log(np.exp(a - m[None]).sum(0))
        out.update({"a": f64(a), "lse": f64(lse), "lpd": f64(lse - np.log(LD(S)))})
    return out


def gate_lpd(ref, y, sd_err, D, S):
    """(N,): max_s [ |y - F_s| (D + 16) EPS A_s / v + 4 EPS |a_s| ] + (S + 16) EPS."""
    v = sd_err * sd_err
    per_s = np.abs(y[None] - ref["F"]) * (D + 16) * EPS * ref["A"] / v + 4 * EPS * np.abs(ref["a"])
    return per_s.max(0) + (S + 16) * EPS


def errors(got, ref, D, S, lpd=None, y=None, sd_err=None):
    """Every gated quantity as (worst error / gate) with the worst error itself: {name: (ratio, err)}; got holds
    Y, F and the eight sums as float64 arrays.  S is the number of samples in the sums."""
    def worst(err, gate):
        err, gate = np.asarray(err, np.float64), np.asarray(gate, np.float64)
        ratio = np.where(err == 0.0, 0.0, err / np.where(gate > 0, gate, 1e-300))
        return float(ratio.max()), float(err.max())

    res = {}
    for k in ("Y", "F"):
        res[k] = worst(np.abs(got[k] - ref[k]), (D + 16) * EPS * ref["A"])
    c = (D + S + 16) * EPS
    res["F_sum"] = worst(np.abs(got["F_sum"] - ref["F_sum"]) / S, c * ref["mean_A"])
    res["F_sq"] = worst(np.abs(got["F_sq"] - ref["F_sq"]) / S, 2 * c * ref["mean_A2"])
    var = lambda d, a, b: d[b] / S - (d[a] / S) ** 2
    res["F_var"] = worst(np.abs(var(got, "F_sum", "F_sq") - var(ref, "F_sum", "F_sq")), 4 * c * ref["mean_A2"])
    c = (S + 16) * EPS
    for p, scale in (("L", "mean_l"), ("G", "mean_G")):
        res[p + "_sum"] = worst(np.abs(got[p + "_sum"] - ref[p + "_sum"]) / S, c * ref[scale])
        res[p + "_sq"] = worst(np.abs(got[p + "_sq"] - ref[p + "_sq"]) / S, 2 * c * ref[scale + "2"])
    if lpd is not None:
        res["lpd"] = worst(np.abs(lpd - ref["lpd"]), gate_lpd(ref, y, sd_err, D, S))
    return res


def report(what, res):
    print(f"{what}: " + "  ".join(f"{k} {e:.2e} ({r:.2f} of gate)" for k, (r, e) in res.items()))
