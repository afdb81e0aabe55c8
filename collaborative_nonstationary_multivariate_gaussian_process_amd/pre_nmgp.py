"""code/pre_nmgp.py on the MI355X: local stationary fits around the inducing points, to seed mu_v, mu_U and
sigma2_err_log (the reference imports pre_estimation_partial as nmgp_dsvi.pre_estimation, code/nmgp_dsvi.py:16).

Around every inducing point z_m the reference fits vec(Y_loc) ~ N(0, K(ell) (x) B + s I) on the nearest rows, with
B = Y^T Y / (N - 1) of all rows, by BFGS from (log s, log ell) = (-6, -6) on the dense P D x P D Gaussian.  Here B is
eigendecomposed once, Y rotated once (Yrot = Y V_B), and one launch (csrc/preest.hip) finds every window's optimum
in the eigen form of the likelihood by a fixed, bounded search.  The search is not BFGS: it returns the minimum over
a box (log ell in [log(delta / 4), log(16 span)] of the window's inputs, log s in log(mean eig B) + [-14, 2]) and
says in `flags` when the answer sits on an edge of it.
"""
import numpy as np
import torch

from . import hip_ops as H

F64 = torch.float64
tridiagonal_jitter = 1e-6


def _device(device=None):
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise RuntimeError("the pre-estimation runs on the GPU; there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _flag_list(flags, bit):
    return [int(m) for m in np.nonzero(flags & bit)[0]]


def _spectral_data(B_dev, Y_dev):
    """mu, Yrot = Y V_B of a (D, D) device matrix B through the library's Jacobi solver and one GEMM."""
    mu, VB = H.syevj(B_dev)
    return mu, H.matmul(Y_dev, VB)


def _local_plan(N, D, P, cov_rows, shrink, holdout):
    """The checks of the local run that need no device -> (Pc, w, alpha, holdout), w and alpha the doubles the kernel
    evaluates B_m = w Y_w^T Y_w + alpha B with."""
    Pc, holdout = int(cov_rows), bool(holdout)
    if not P <= Pc <= H.PRE_MAX_COV_ROWS:
        raise ValueError(f"cov_rows must lie in P = {P}..{H.PRE_MAX_COV_ROWS}, got {Pc}")
    if P * holdout + Pc > N:
        raise ValueError(f"{N} complete rows, fewer than the {'P + ' if holdout else ''}cov_rows = "
                         f"{P * holdout + Pc} the windows need")
    alpha = D / (D + Pc - 1.0) if shrink is None else float(shrink)       # B counts as D pseudo-rows
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"shrink must lie in [0, 1], got {shrink}")
    return Pc, (1.0 - alpha) / (Pc - 1.0), alpha, holdout


def pre_estimate(x, Y, z, P=10, device=None, cov_rows=None, shrink=None, holdout=True):
    """The run behind pre_estimation_partial as a dict: "v_array" (M,) = log ell, "L_tensor" (D, D, M),
    "sigma2_err_log_array" (M,) = log s, "nll" (M,) the windows' minimal negative log-likelihoods, "flags" (M,) int32
    (hip_ops.PRE_FLAG_*: 1 / 2 log ell at the lower / upper edge of its box, 4 / 8 log s at its lower / upper edge),
    "neighbours" (M, P) int32 rows of the complete-row arrays in ascending order, "B" (D, D), all numpy, and "box"
    (M, 4).  Raises as pre_estimation_partial does.

    cov_rows = Pc switches to the local run behind pre_estimation_local (csrc/prelocal.hip): per inducing point
    B_m = (1 - alpha) Y_w^T Y_w / (Pc - 1) + alpha B over its covariance window Y_w -- the Pc rows that follow the P
    fit rows in the order by (|x_n - z_m|, n) (holdout, the default), or the first Pc rows of it -- alpha = shrink, or
    D / (D + Pc - 1) for None; "L_tensor" then holds chol(B_m) and the fit uses B_m in place of B.  The dict adds
    "B_local" (M, D, D), "cov_neighbours" (M, Pc), "shrink" (the alpha used) and "holdout".  A B_m that is not
    positive definite raises numpy.linalg.LinAlgError naming the z indices."""
    x = np.asarray(x, np.float64).reshape(-1)
    Y = np.asarray(Y, np.float64)
    z = np.asarray(z, np.float64).reshape(-1)
    P = int(P)
    if Y.ndim != 2 or Y.shape[0] != x.shape[0]:
        raise ValueError(f"Y must be (N, D) with N = len(x) = {x.shape[0]}, got {Y.shape}")
    if not H.PRE_MIN_P <= P <= H.PRE_MAX_P:
        raise ValueError(f"P must lie in {H.PRE_MIN_P}..{H.PRE_MAX_P}, got {P}")
    keep = ~np.isnan(Y).any(axis=1)
    x, Y = x[keep], Y[keep]
    N, D = Y.shape
    if N < P:
        raise ValueError(f"{N} complete rows, fewer than the P = {P} a window needs")
    if not 1 <= D <= H.PRE_MAX_D:
        raise ValueError(f"D must lie in 1..{H.PRE_MAX_D}, got {D}")
    plan = None if cov_rows is None else _local_plan(N, D, P, cov_rows, shrink, holdout)
    dev = _device(device)
    Yd = torch.from_numpy(np.ascontiguousarray(Y)).to(dev)
    B = H.matmul(Yd, Yd, transA=True, alpha=1.0 / (N - 1))
    B = 0.5 * (B + B.T)                       # exactly symmetric, whatever order the GEMM summed its tiles in
    if plan is not None:
        return _pre_estimate_local(x, Yd, B, z, P, plan, dev)
    Lf = B.clone()
    info = H.potrf_(Lf)
    if int(info.reshape(-1)[0].item()) != 0:
        raise np.linalg.LinAlgError("Matrix is not positive definite")       # numpy's words, as in the reference
    Lf = torch.tril(Lf)
    mu, Yrot = _spectral_data(B, Yd)
    res = H.pre_estimate_(torch.from_numpy(x).to(dev), Yrot, mu, torch.from_numpy(z).to(dev), P)
    out = {k: v.cpu().numpy() for k, v in res.items()}
    flags = out["flags"]
    bad = _flag_list(flags, H.PRE_FLAG_DEGENERATE)
    if bad:
        raise ValueError(f"degenerate windows (all inputs equal, or fewer than P finite inputs) at z index {bad}")
    bad = _flag_list(flags, H.PRE_FLAG_JACOBI)
    if bad:
        raise RuntimeError(f"the Jacobi eigensolver did not converge in the windows at z index {bad}")
    Ln = Lf.cpu().numpy()
    return {"v_array": out["log_ell"], "L_tensor": np.stack([Ln for _ in range(z.shape[0])], axis=-1),
            "sigma2_err_log_array": out["log_s"], "nll": out["nll"], "flags": flags,
            "neighbours": out["neighbours"], "B": B.cpu().numpy(), "box": out["box"]}


def _pre_estimate_local(x, Yd, B, z, P, plan, dev):
    """The local run on the complete rows: the factor launch, the windows' eigenbases (existing batched Jacobi and
    GEMM, on the P fit rows only), the search on the windows."""
    Pc, w, alpha, holdout = plan
    fac = H.pre_local_factor_(torch.from_numpy(x).to(dev), Yd, B, torch.from_numpy(z).to(dev), P, Pc, w, alpha, holdout)
    fflags = fac["flags"].cpu().numpy()
    bad = _flag_list(fflags, H.PRE_FLAG_DEGENERATE)
    if bad:
        raise ValueError(f"degenerate windows (fewer than {P * holdout + Pc} finite inputs) at z index {bad}")
    bad = _flag_list(fflags, H.PRE_FLAG_FACTOR)
    if bad:
        raise np.linalg.LinAlgError(f"the local matrix is not positive definite at z index {bad}")
    mu, V = H.syevj(fac["B_local"])
    res = H.pre_estimate_windows_(fac["xs"], H.bmm(fac["Yloc"], V), mu)
    out = {k: v.cpu().numpy() for k, v in res.items()}
    flags = out["flags"]
    bad = _flag_list(flags, H.PRE_FLAG_DEGENERATE)
    if bad:
        raise ValueError(f"degenerate windows (all inputs equal, or fewer than P finite inputs) at z index {bad}")
    bad = _flag_list(flags, H.PRE_FLAG_JACOBI)
    if bad:
        raise RuntimeError(f"the Jacobi eigensolver did not converge in the windows at z index {bad}")
    return {"v_array": out["log_ell"], "L_tensor": np.ascontiguousarray(fac["L"].permute(1, 2, 0).cpu().numpy()),
            "sigma2_err_log_array": out["log_s"], "nll": out["nll"], "flags": flags,
            "neighbours": fac["neighbours"].cpu().numpy(), "B": B.cpu().numpy(), "box": out["box"],
            "B_local": fac["B_local"].cpu().numpy(), "cov_neighbours": fac["cov_neighbours"].cpu().numpy(),
            "shrink": alpha, "holdout": holdout}


def pre_estimation_local(x, Y, z, P=10, cov_rows=40, shrink=None, holdout=True, device=None):
    """What code/pre_nmgp.py:64-100 (pre_estimation_all) set out to return and never did: (v_array (M,), L_tensor
    (D, D, M), sigma2_err_log_array (M,)) with a coefficient factor of its own per inducing point.

    L_tensor[:, :, m] = chol((1 - alpha) Y_w^T Y_w / (cov_rows - 1) + alpha Y^T Y / (N - 1)) over the covariance window
    Y_w of z_m, uncentred as the reference's est_L (:71); v_array[m] and sigma2_err_log_array[m] minimise the
    likelihood of the P fit rows under that matrix.  holdout (default) keeps the fit rows out of the covariance window:
    rows that are iid under a covariance estimated from themselves drive the fit to ell -> 0 and s to the lower edge
    of its box once D is not small against cov_rows.  shrink = alpha in [0, 1]; None counts the global matrix as D
    pseudo-rows, alpha = D / (D + cov_rows - 1).  Limits: 3 <= P <= 32, P <= cov_rows <= 1024, D <= 128 and
    P holdout + cov_rows complete rows.  Raises as pre_estimation_partial does; a local matrix that is not positive
    definite raises numpy.linalg.LinAlgError naming the z indices.  The reference's route (BFGS over the D (D + 1) / 2
    factor entries on the dense P D x P D Gaussian) is not taken."""
    r = pre_estimate(x, Y, z, P=P, device=device, cov_rows=cov_rows, shrink=shrink, holdout=holdout)
    return r["v_array"], r["L_tensor"], r["sigma2_err_log_array"]


def pre_estimation_partial(x, Y, z, P=10, device=None):
    """code/pre_nmgp.py:102-125 -> (v_array (M,), L_tensor (D, D, M), sigma2_err_log_array (M,)) as numpy.

    x (N,), Y (N, D), z (M,).  Rows of Y that contain NaN are dropped first; fewer than P complete rows raise
    ValueError.  L_tensor[:, :, m] is the Cholesky factor of Y^T Y / (N - 1) for every m, as in the reference (a
    non-positive-definite matrix raises numpy.linalg.LinAlgError, as numpy does there); v_array[m] = log ell and
    sigma2_err_log_array[m] = log s minimise the likelihood of the window of z_m.

    P is honoured (3..32): the window holds the P nearest rows.  The reference takes 10 rows whatever P says
    (code/pre_nmgp.py:11), so the default P = 10 is the reference's behaviour.  A window whose inputs are all equal
    raises ValueError naming it; an eigensolve that did not converge raises RuntimeError; answers on an edge of the
    search box are returned as they are and flagged in pre_estimate(...)["flags"]."""
    r = pre_estimate(x, Y, z, P=P, device=device)
    return r["v_array"], r["L_tensor"], r["sigma2_err_log_array"]


def pre_estimation_all(x, Y, z, P=10):
    """code/pre_nmgp.py:64-100 also fits the coefficient factor per window; the reference stops in pdb inside its
    loop (:89-90) and never returns.  Not provided; pre_estimation_local gives per-window factors by another route."""
    raise NotImplementedError("pre_estimation_all is not provided: the reference's own version stops in a debugger; "
                              "use pre_estimation_partial")


def compute_loglik_part(pars, x, Y, L, device=None):
    """code/pre_nmgp.py:48-56: the log-likelihood of the rows (x (P,), Y (P, D)) under K(exp(pars[1])) (x) L L^T +
    exp(pars[0]) I, through the evaluation entry of the kernel (3 <= P <= 32 rows, D <= 128)."""
    pars = np.asarray(pars, np.float64).reshape(-1)
    x = np.asarray(x, np.float64).reshape(-1)
    Y = np.asarray(Y, np.float64)
    L = np.asarray(L, np.float64)
    Pn, D = Y.shape
    if x.shape[0] != Pn or L.shape != (D, D):
        raise ValueError(f"x must be ({Pn},) and L ({D}, {D}) for Y {Y.shape}")
    if not H.PRE_MIN_P <= Pn <= H.PRE_MAX_P or not 1 <= D <= H.PRE_MAX_D:
        raise ValueError(f"the evaluation takes {H.PRE_MIN_P}..{H.PRE_MAX_P} rows and up to {H.PRE_MAX_D} outputs, "
                         f"got {Y.shape}")
    dev = _device(device)
    Ld = torch.from_numpy(np.ascontiguousarray(L)).to(dev)
    mu, Yrot = _spectral_data(H.matmul(Ld, Ld, transB=True), torch.from_numpy(np.ascontiguousarray(Y)).to(dev))
    xd = torch.from_numpy(x).to(dev)
    pr = torch.tensor([[[pars[0], pars[1]]]], dtype=F64, device=dev)
    res = H.pre_loglik_(xd, Yrot, mu, xd[:1], Pn, pr)
    if int(res["flags"][0].item()) & H.PRE_FLAG_JACOBI:
        raise RuntimeError("the Jacobi eigensolver did not converge")
    return -float(res["nll"][0, 0].item())


def compute_loglik(pars, x, Y, device=None):
    """code/pre_nmgp.py:35-46: as compute_loglik_part with the factor's lower triangle in pars[2:]."""
    pars = np.asarray(pars, np.float64).reshape(-1)
    D = np.asarray(Y).shape[1]
    L = np.zeros([D, D])
    L[np.tril_indices(D)] = pars[2:]
    return compute_loglik_part(pars[:2], x, Y, L, device=device)


def objective(pars, x, Y):
    return -compute_loglik(pars, x, Y)


def objective_part(pars, x, Y, L):
    return -compute_loglik_part(pars, x, Y, L)
