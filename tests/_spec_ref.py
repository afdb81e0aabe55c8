"""Host reference of the correlation-spectrum kernel (include/nmgp_hip.h, nmgp_corr_spectrum_f64): eigenvalues and
eigenvectors of the correlation samples of _cgroup_ref.corr_samples in np.longdouble, rounded to float64 at the end,
and the float64 restatement (np.linalg.eigvalsh / eigh of the float64 correlation samples); shared by the CPU pin
and the GPU tests.  LAPACK has no long double, so the solver is written here.

The solver (eigh_ld) is a cyclic two-sided Jacobi in long double, vectorised over the batch, a round of the
round-robin ordering (D / 2 disjoint pairs) at a time.  Two things keep it affordable at D = 128:
  * it starts from the basis V of float64 LAPACK, made orthogonal to long-double accuracy by one Newton-Schulz step
    (V <- V - V (V^T V - I) / 2: the defect 1e-15 squares to 1e-30), and sweeps T = V^T A V, whose off-diagonal is
    already 1e-14; any orthogonal start gives the same eigenvalues, the start only saves sweeps;
  * a pair is rotated only where the rotation moves its diagonal entries, |t a_pq| > 2^-66 (|a_pp| + |a_qq|)
    (Rutishauser's rule), and only the batch members that need it are touched.  What is left unrotated moves an
    eigenvalue by at most D 2^-66 2 lambda_1 in first order, the size of the long-double rounding of the sums.
The eigenvectors of the leading modes (their gap to the rest at least 1e-3 by the condition below) are the
accumulated basis corrected to first order for the unrotated rest, x = e_r + sum_j T_jr / (T_rr - T_jj) e_j; the
second-order term is below (2^-33 / gap)^2.  tests/test_spec_reference.py pins the solver to mpmath at 40 digits.

Gates (derived where they can be; never measured on the kernel):
  * eigenvalues, absolute: gate_eig(D, e64) = D gate_c(D) + 8 e64.  Weyl: |d lambda| <= |dR|_2 <= |dR|_F <=
    D x (the element gate of a correlation, _corrq_ref.gate_c).  e64 is the float64-LAPACK vs long-double
    eigenvalue error on the very input, the solver's own error, which has no tight derivation; the factor 8 is the
    margin for a different but backward-stable rotation order;
  * effective dimension D^2 / sum lambda^2: 2 D gate_eig (d eff / eff = -2 sum lambda d lambda / sum lambda^2,
    sum lambda = D, eff <= D);
  * squared loadings of a mode summed over S samples: S 4 gate_eig / gap, gap the reference's smallest distance
    from that mode's eigenvalue to any other over the shape (Davis-Kahan).  Compared only for the modes
    r < min(4, D), and the inputs must keep those gaps >= 1e-3 (MIN_GAP; a condition on the inputs, checked on the
    CPU for every GPU shape).  Below the leading modes the spectra of the recipe cluster (gaps reach 1e-16 at
    D = 128), so the loadings of low modes are deliberately not compared.

Measured on the inputs of the GPU tests (_fy_ref.make_inputs with _pcorr_ref.seed_of; e64, smallest top-4 gap):
  (1, 1, 1) 0, -;  (2, 11, 3) 2.2e-16, 1.2e-2;  (3, 7, 5) 6.7e-16, 9.8e-2;  (15, 5, 4) 5.3e-15, 2.7e-2;
  (16, 3, 2) 3.1e-15, 9.3e-2;  (17, 70, 37) 8.0e-15, 1.6e-3;  (33, 9, 4) 7.1e-15, 4.1e-2;  (50, 9, 6) 1.1e-14,
  1.7e-2;  (128, 3, 5) 2.2e-14, 6.2e-2;  (17, 256, 3) 6.2e-15, 7.9e-3;  (33, 256, 2) 9.8e-15, 1.2e-2;
  (128, 256, 2) 3.2e-14, 7.6e-3;  (40, 200, 5) 1.2e-14, 8.3e-3.
The long-double solve of the 512 matrices of (128, 256, 2) takes some 15 s on a CPU core, most of it the three
sliced products; every other shape takes 2 s or less."""
import functools

import numpy as np

from tests import _cgroup_ref as GR
from tests import _corrq_ref as CR
from tests import _fy_ref as F
from tests import _pcorr_ref as PR

LD = np.longdouble
EPS = 2.0 ** -52
MIN_GAP = 1e-3
NVEC = 4
GPU_SHAPES = PR.GPU_SHAPES


def gate_eig(D, e64):
    return D * CR.gate_c(D) + 8.0 * e64


def gate_eff(D, e64):
    return 2.0 * D * gate_eig(D, e64)


def gate_load(D, S, e64, gap):
    return S * 4.0 * gate_eig(D, e64) / gap


def _rounds(np_):
    """The np_ - 1 rounds of the round-robin (circle) ordering of np_ (even) indices -> list of (P, Q) index arrays."""
    m = np_ - 1
    out = []
    for r in range(m):
        P, Q = [r % m], [m]
        for k in range(1, np_ // 2):
            P.append((r + k) % m)
            Q.append((r - k) % m)
        P, Q = np.array(P), np.array(Q)
        out.append((np.minimum(P, Q), np.maximum(P, Q)))
    return out


_SLICE_BITS = 22


def _slices(X, axis):
    """Three float64 slices of the long-double matrices X (B, m, n), each entry of a slice a multiple of a unit
    that is common to its row (axis = 2) or column (axis = 1) and at most 2^22 units large; their sum is X up to
    2^-66 of the row's (column's) largest entry."""
    mu = np.abs(X).max(axis=axis, keepdims=True)
    e = np.frexp(np.where(mu > 0, mu, LD(1)))[1].astype(np.int64)                      # mu <= 2^e
    out, rest = [], X
    for k in range(1, 4):
        unit = np.ldexp(LD(1), e - k * _SLICE_BITS)
        s = np.rint(rest / unit) * unit
        out.append(s.astype(np.float64))
        rest = rest - s
    return out


def _mm_sliced(xs, ys):
    """The product of two sliced operands (rows of the left one, columns of the right one): every float64 product of
    two slices is exact (2 x 22 + 7 bits for an inner dimension <= 128); the six products down to 2^-66 of
    |row| |column| are added in long double, smallest first (the three left out are below 2^-86)."""
    assert xs[0].shape[-1] <= 128
    acc = None
    for tot in (2, 1, 0):
        for a in range(tot + 1):
            p = np.matmul(xs[a], ys[tot - a]).astype(LD)
            acc = p if acc is None else acc + p
    return acc


def matmul_ld(X, Y):
    """X @ Y for batches of long-double matrices with inner dimension <= 128, through float64 BLAS: both operands are
    cut into slices of 22 bits against a common row / column exponent (Ozaki's scheme).  The result is within 2^-64
    |row of X| |column of Y| of the exact product -- as tight as numpy's long-double matmul, and several times
    faster."""
    return _mm_sliced(_slices(np.asarray(X, LD), 2), _slices(np.asarray(Y, LD), 1))


def eigh_ld(A, nvec=0, precondition=True, max_sweeps=40):
    """Eigenvalues (B, D) descending and the eigenvectors (B, D, nvec) of the nvec leading modes of the symmetric
    long-double matrices A (B, D, D).  A matrix with a non-finite entry gives NaN."""
    A = np.array(A, LD)
    B, D = A.shape[:2]
    good = np.isfinite(A).all((1, 2))
    A[~good] = np.eye(D, dtype=LD)
    A = (A + np.swapaxes(A, 1, 2)) / LD(2)
    eye = np.eye(D, dtype=LD)
    X = None
    if precondition and D > 1:
        # T = V'^T A V' for V' = V (I - X / 2), X = V^T V - I the float64 basis' defect (1e-15): to first order in
        # X, and T being diagonal up to 1e-14, T'_ij = T_ij - X_ij (T_ii + T_jj) / 2; what is dropped is 1e-29
        V = np.linalg.eigh(A.astype(np.float64))[1].astype(LD)
        vs = _slices(V, 1)                                                # by columns; transposed, V^T by rows
        vts = [np.swapaxes(v, 1, 2) for v in vs]
        X = _mm_sliced(vts, vs) - eye
        T = _mm_sliced(vts, _slices(_mm_sliced(_slices(A, 2), vs), 1))
        dg = np.einsum("bii->bi", T)
        T = T - X * (dg[:, :, None] + dg[:, None, :]) / LD(2)
        T = (T + np.swapaxes(T, 1, 2)) / LD(2)
    else:
        V = np.broadcast_to(eye, A.shape).copy()
        T = A
    Jm = np.broadcast_to(eye, A.shape).copy() if nvec else None                         # the rotations, accumulated
    tol = LD(2.0) ** -66
    np_ = D + (D & 1)
    rounds = [(P[Q < D], Q[Q < D]) for P, Q in _rounds(np_)] if D > 1 else []
    with np.errstate(all="ignore"):
        for sweep in range(max_sweeps):
            rotated = False
            for P, Q in rounds:
                app, aqq, apq = T[:, P, P], T[:, Q, Q], T[:, P, Q]                  # (B, H)
                tau = (aqq - app) / (LD(2) * apq)
                t = np.where(tau >= 0, LD(1), LD(-1)) / (np.abs(tau) + np.sqrt(LD(1) + tau * tau))
                t = np.where(apq == 0, LD(0), t)
                need = np.abs(t * apq) > tol * (np.abs(app) + np.abs(aqq))
                bi, pi = np.nonzero(need)
                if bi.size == 0:
                    continue
                rotated = True
                # only the (batch member, pair) that need a rotation are touched; the pairs of a round are disjoint
                Pn, Qn = P[pi], Q[pi]
                t = t[bi, pi]
                c = (LD(1) / np.sqrt(LD(1) + t * t))[:, None]
                s = t[:, None] * c
                rp, rq = T[bi, Pn, :], T[bi, Qn, :]                                  # rows  <-  J^T T, (m, D)
                T[bi, Pn, :], T[bi, Qn, :] = c * rp - s * rq, s * rp + c * rq
                cp, cq = T[bi, :, Pn], T[bi, :, Qn]                                  # columns  <-  T J, (m, D)
                T[bi, :, Pn], T[bi, :, Qn] = c * cp - s * cq, s * cp + c * cq
                if nvec:
                    vp, vq = Jm[bi, :, Pn], Jm[bi, :, Qn]
                    Jm[bi, :, Pn], Jm[bi, :, Qn] = c * vp - s * vq, s * vp + c * vq
            if not rotated:
                break
        else:
            raise RuntimeError("eigh_ld: no convergence")
        d = np.einsum("bii->bi", T).copy()
        order = np.argsort(-d, axis=1, kind="stable")
        lam = np.take_along_axis(d, order, 1)
        U = None
        if nvec:
            nvec = min(nvec, D)
            U = np.empty((B, D, nvec), LD)
            rows = np.arange(B)
            for r in range(nvec):
                j = order[:, r]
                den = d[rows, j][:, None] - d                                        # T_rr - T_jj
                x = T[rows, :, j] / np.where(den == 0, LD(1), den)
                x[rows, j] = LD(1)
                y = np.einsum("bij,bj->bi", Jm, x)
                if X is not None:
                    y = y - np.einsum("bij,bj->bi", X, y) / LD(2)                     # V' = V (I - X / 2)
                u = np.einsum("bij,bj->bi", V, y)
                U[:, :, r] = u / np.sqrt((u * u).sum(1))[:, None]
            U[~good] = np.nan
        lam[~good] = np.nan
    return lam, U


def spectrum_of(corr, nvec=NVEC):
    """Long-double correlation samples (S, N, D, D) -> dict of float64 arrays: "eig" (D, N, S) descending, "eff"
    (N, S), "load2" (N, min(nvec, D), D) the squared loadings of the leading modes summed over the samples, "gap"
    (min(nvec, D),) the smallest distance of each leading mode's eigenvalue to any other over the shape (inf for
    D = 1).  A sample with a non-finite correlation is NaN (and makes load2 NaN at its input)."""
    S, N, D = corr.shape[:3]
    lam, U = eigh_ld(corr.reshape(S * N, D, D), nvec)
    lam = lam.reshape(S, N, D)
    nv = min(nvec, D)
    with np.errstate(all="ignore"):
        eff = LD(D) * LD(D) / (lam * lam).sum(-1)
        load2 = np.transpose((U * U).reshape(S, N, D, nv).sum(0), (0, 2, 1))
        gap = np.full(nv, np.inf)
        for r in range(nv):
            others = np.delete(lam, r, axis=2)
            if others.shape[2]:
                gap[r] = float(np.nanmin(np.abs(others - lam[:, :, r:r + 1])))
    return {"eig": np.transpose(lam, (2, 1, 0)).astype(np.float64), "eff": eff.T.astype(np.float64),
            "load2": load2.astype(np.float64), "gap": gap}


def eig_f64(corr64):
    """The float64 restatement: np.linalg.eigvalsh of float64 correlation samples (S, N, D, D) -> (D, N, S)
    descending; NaN where a sample is not finite."""
    S, N, D = corr64.shape[:3]
    good = np.isfinite(corr64).all((2, 3))
    c = np.where(good[..., None, None], corr64, np.eye(D))
    lam = np.linalg.eigvalsh(c)[..., ::-1].copy()
    lam[~good] = np.nan
    return np.transpose(lam, (2, 1, 0))


def e64_of(eig64, eig_ref):
    d = np.abs(eig64 - eig_ref)
    return float(np.nanmax(d)) if np.isfinite(d).any() else 0.0


def inputs(D, N, S):
    """The inputs of the GPU tests at a shape: the unit-scale recipe of _fy_ref with the seed of _pcorr_ref."""
    return F.make_inputs(D, N, S, PR.seed_of(D, N, S))


def reference(inp):
    """-> (spectrum_of the long-double correlation samples of the inputs, e64 of their eigenvalues)."""
    corr = GR.corr_samples(inp["pair_mu"], inp["pair_sd"], inp["z_p"], LD)
    ref = spectrum_of(corr)
    return ref, e64_of(eig_f64(corr.astype(np.float64)), ref["eig"])


@functools.lru_cache(maxsize=None)
def case(D, N, S):
    """Inputs of a GPU kernel test, their reference and e64, computed once per shape and shared (never modified)."""
    inp = inputs(D, N, S)
    ref, e64 = reference(inp)
    return inp, ref, e64
