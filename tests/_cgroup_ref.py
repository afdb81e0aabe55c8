"""Host restatement of the group-mean kernels (include/nmgp_hip.h, nmgp_corr_group_f64 and the group output of
nmgp_pcorr_accum_groups_f64) in np.longdouble, rounded to float64 at the end, and the same in plain float64; shared
by the CPU pin and the GPU tests.

The gates are derived, not measured on the kernel:
  * gate_group(D, g) = _corrq_ref.gate_c(D) + g 2^-52: every term of a group is a correlation within gate_c(D) of its
    long-double value, so is their mean; a float64 sum of g terms of magnitude <= 1, divided by g, adds at most g ulps
    of 1 in any summation order;
  * for the partial correlations gate_pgroup(D, g, e64) = _pcorr_ref.gate(D, 1, e64) + g 2^-52, with e64 the float64
    vs longdouble error of the sequential algorithm on the very input (measured on the reference, never on the
    kernel)."""
import functools

import numpy as np

from tests import _corrq_ref as CR
from tests import _fy_ref as F
from tests import _pcorr_ref as PR

LD = np.longdouble
EPS = 2.0 ** -52


def gate_group(D, g):
    return CR.gate_c(D) + g * EPS


def gate_pgroup(D, g, e64):
    return PR.gate(D, 1, e64) + g * EPS


def corr_samples(pair_mu, pair_sd, z_p, dt=LD):
    """-> corr (S, N, D, D) in dtype dt, the construction of _corrq_ref.collect_ref: the full D x D matrices (L is
    zero above its diagonal), the diagonal exactly 1 where finite and NaN where not."""
    S, Q, N = z_p.shape
    D = int(round((np.sqrt(8 * Q + 1) - 1) / 2))
    with np.errstate(all="ignore"):
        l = pair_mu.astype(dt)[None] + pair_sd.astype(dt)[None] * z_p.astype(dt)      # (S, Q, N)
        Lm = np.zeros((S, N, D, D), dt)
        for q, (i, j) in enumerate(F.pairs(D)):
            Lm[:, :, i, j] = np.exp(l[:, q]) if i == j else l[:, q]
        cov = np.matmul(Lm, np.swapaxes(Lm, 2, 3))
        isd = np.sqrt(dt(1) / np.einsum("snii->sni", cov))
        c = cov * isd[..., :, None] * isd[..., None, :]
        idx = np.arange(D)
        c[:, :, idx, idx] = np.where(np.isfinite(c[:, :, idx, idx]), dt(1), dt(np.nan))
    return c


def group_means(mat, groups):
    """(S, N, D, D) samples -> (K, N, S) float64: per group the entries added one by one in the listed order in the
    dtype of mat, divided by the group's size, rounded at the end."""
    S, N = mat.shape[:2]
    out = np.empty((len(groups), N, S), np.float64)
    with np.errstate(all="ignore"):
        for k, g in enumerate(groups):
            acc = np.zeros((S, N), mat.dtype)
            for i, j in g:
                acc = acc + mat[:, :, max(i, j), min(i, j)]
            out[k] = (acc / mat.dtype.type(len(g))).astype(np.float64).T
    return out


def group_ref(pair_mu, pair_sd, z_p, groups):
    """-> (K, N, S): the group means of the correlation samples, np.longdouble, rounded at the end."""
    return group_means(corr_samples(pair_mu, pair_sd, z_p, LD), groups)


def group_f64(pair_mu, pair_sd, z_p, groups):
    """The same in plain float64."""
    return group_means(corr_samples(pair_mu, pair_sd, z_p, np.float64), groups)


def pgroup_ref(pair_mu, pair_sd, z_p, groups):
    """-> (K, N, S): the group means of the partial-correlation samples of _pcorr_ref, np.longdouble."""
    return group_means(PR._pcorr(pair_mu, pair_sd, z_p, LD)[0], groups)


def pgroup_f64(pair_mu, pair_sd, z_p, groups):
    return group_means(PR._pcorr(pair_mu, pair_sd, z_p, np.float64)[0], groups)


def all_pairs(D):
    return [(i, j) for i in range(D) for j in range(i)]


def err(got, want):
    """max |got - want| over the entries that are not NaN in both; the NaN patterns must agree."""
    assert np.array_equal(np.isnan(got), np.isnan(want))
    d = np.abs(got - want)
    return float(np.nanmax(d)) if np.isfinite(d).any() else 0.0


@functools.lru_cache(maxsize=None)
def case(D, N, S, scaled=True):
    """Inputs of a GPU kernel test, their long-double correlation and partial-correlation samples (S, N, D, D) and
    e64 of the partial correlations, computed once per shape and shared (never modified).  scaled: the well-
    conditioned recipe of _pcorr_ref, else the unit-scale one of _fy_ref."""
    seed = PR.seed_of(D, N, S)
    inp = PR.make_inputs(D, N, S, seed) if scaled else F.make_inputs(D, N, S, seed)
    corr = corr_samples(inp["pair_mu"], inp["pair_sd"], inp["z_p"], LD)
    pc = PR._pcorr(inp["pair_mu"], inp["pair_sd"], inp["z_p"], LD)[0]
    e64 = PR.e64_of(PR.pcorr_f64(inp["pair_mu"], inp["pair_sd"], inp["z_p"]), pc.astype(np.float64))
    return inp, corr, pc, e64
