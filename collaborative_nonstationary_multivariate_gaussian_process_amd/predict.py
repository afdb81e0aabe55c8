"""Posterior-mean prediction on the MI355X (reference NMGP.predict_Y, code/nmgp_dsvi.py:666-722).

All kernel matrices come from the HIP builder, the four solves K12 (K22 + 1e-4 I)^{-1} mu go
through the HIP Cholesky / triangular inverse / MFMA GEMM; only the final per-row gather
(est_Y[n] = sum_j L[I_n, j, n] G[j, n], the reference's permute + index, :721-722) is a small
elementwise reduction.
"""
import numpy as np
import torch

from . import _lib as L
from . import hip_ops as H

F64 = torch.float64
JIT = 1e-4


def prepare_inputs(model, inputs_list, index=None):
    """Device copies of the prediction inputs (x as a column, the output id of every row): made once
    when the same test inputs are predicted every iteration (inference(X_test_list=...))."""
    dev = model.device_
    xs = [torch.as_tensor(x).reshape(-1).to(F64) for x in inputs_list]
    ids = list(range(len(xs))) if index is None else list(index)
    I = torch.cat([torch.full((x.shape[0],), int(j), dtype=torch.long) for x, j in zip(xs, ids)]).to(dev)
    x = torch.cat([t.to(dev) for t in xs]).reshape(-1, 1).contiguous()
    return x, I


class PredictPlan:
    """NMGP.predict_Y (code/nmgp_dsvi.py:666-722) for one fixed set of prediction inputs, in fp64.

    The four GP systems of the prediction -- the three RBF priors (tilde-ell, L0, L1) and the Gibbs prior,
    whose K22 needs only ell_Z = exp(mu_v) -- are built by ONE pairwise launch (K22 + 1e-4 I and the three
    RBF cross kernels) and factored by ONE batched fused Cholesky + inverse launch; each solve
    K12 (K22 + 1e-4 I)^{-1} rhs is K12 (C^-T (C^-1 rhs)).  Buffers and kernel descriptors are made once, the
    hyper-parameters and means are read from theta on the device when the plan runs, so with graph=True the
    whole prediction is one HIP graph replay (inference(X_test_list=...) predicts after every iteration,
    code/nmgp_dsvi.py:865-868).  `info_acc` keeps the largest Cholesky info word of every run since the
    plan was made (0: all factorizations succeeded)."""

    def __init__(self, model, prepared, graph=False):
        self.model = model
        self.x, self.I = prepared
        dev, D, M = model.device_, model.D, model.M
        Bn = self.x.shape[0]
        Z = model.Z.to(F64)
        self.Z = Z
        e = lambda *shape: torch.empty(*shape, dtype=F64, device=dev)
        self.K22, self.Ci, self.K12 = e(4, M, M), e(4, M, M), e(3, Bn, M)
        self.KG12, self.ellZ, self.ellX, self.hyp64 = e(Bn, M), e(M), e(Bn), e(7)
        self.info = torch.zeros(4, dtype=torch.int32, device=dev)
        self.info_acc = torch.zeros(4, dtype=torch.int32, device=dev)
        descs = [H.pairwise_desc(self.K22[k], Z, Z, mode=L.RBF, hyp=self.hyp64, hyp_off=2 * k, hyp_log=True,
                                 diag_add=JIT) for k in range(3)]
        descs.append(H.pairwise_desc(self.K22[3], Z, Z, mode=L.GIBBS, ellX=self.ellZ, ellZ=self.ellZ, diag_add=JIT))
        descs += [H.pairwise_desc(self.K12[k], self.x, Z, mode=L.RBF, hyp=self.hyp64, hyp_off=2 * k, hyp_log=True)
                  for k in range(3)]
        self.build = H.PairwiseGroup(descs, dev)
        self.build_g12 = H.PairwiseGroup([H.pairwise_desc(self.KG12, self.x, Z, mode=L.GIBBS, ellX=self.ellX,
                                                          ellZ=self.ellZ)], dev)
        self.rows = torch.arange(Bn, device=dev)
        self.diag = torch.eye(D, dtype=torch.bool, device=dev).reshape(-1)
        if model.packed:
            ii, jj = np.tril_indices(D)
            self.pair_ij = (torch.from_numpy(ii).to(dev), torch.from_numpy(jj).to(dev))
        self.graph, self.est = None, None
        if graph:
            cur = torch.cuda.current_stream(dev)
            s = torch.cuda.Stream(device=dev)
            s.wait_stream(cur)
            with torch.cuda.stream(s):
                self._body()                    # warm-up: library load, GEMM paths, allocator pool
            cur.wait_stream(s)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.est = self._body()

    def _solve(self, k, K12, rhs):
        """K12 (K22_k + 1e-4 I)^{-1} rhs = K12 C_k^-T (C_k^-1 rhs), C_k^-1 lower triangular."""
        Ck = self.Ci[k]
        y = H.matmul(Ck, rhs, maskA=L.A_LOWER)
        y = H.matmul(Ck, y, transA=True, maskA=L.A_UPPER)
        return H.matmul(K12, y)

    def _body(self):
        m = self.model
        D, M = m.D, m.M
        o = m._offs["sigma2_tildeell_log"][0]
        self.hyp64.copy_(m._theta.detach()[o:o + 7])
        mu_v = m.mu_v.detach().to(F64).reshape(-1)
        torch.exp(mu_v, out=self.ellZ)
        self.build(F64)                                                   # K22 + 1e-4 I (x4), K12 (x3)
        H.chol_inv_(self.K22, out=self.Ci, info=self.info)                 # one batched launch
        torch.maximum(self.info_acc, self.info, out=self.info_acc)
        t_ell = self._solve(0, self.K12[0], mu_v.reshape(-1, 1).contiguous()).reshape(-1)
        torch.exp(t_ell, out=self.ellX)
        if m.packed:
            muU = torch.zeros(D, D, M, dtype=F64, device=m.device_)
            muU[self.pair_ij] = m.mu_U.detach().to(F64)
        else:
            muU = m.mu_U.detach().to(F64)
        muU = muU.reshape(D * D, M).t().contiguous()                      # (M, D*D)
        L0 = self._solve(1, self.K12[1], muU)                             # (B, D*D)
        L1 = self._solve(2, self.K12[2], muU)
        self.build_g12(F64)                                               # K_G12 from ell_X, ell_Z
        Gm = self._solve(3, self.KG12, m.mu_W.detach().to(F64).t().contiguous())   # (B, D)
        Bn = self.x.shape[0]
        Lr = torch.where(self.diag, torch.exp(L1), L0).reshape(Bn, D, D)
        Lr = torch.tril(Lr)                                               # est_L[i, j] for j <= i
        rowsL = Lr[self.rows, self.I]                                     # (B, D): row I_n of L at n
        return (rowsL * Gm).sum(1)

    def __call__(self):
        """The posterior means (N,) of the current parameters (no host synchronisation)."""
        if self.graph is not None:
            self.graph.replay()
            return self.est
        return self._body()


def predict_mean(model, inputs_list, index=None, prepared=None, defer_check=False):
    """NMGP.predict_Y (code/nmgp_dsvi.py:666-722) -> (N,) device tensor, computed in fp64 (PredictPlan).

    The four Cholesky info words are checked at the end -- or, with defer_check=True, left to the model's
    next check_numerics() (the caller's existing synchronisation point).  `prepared`: the (x, I) of
    prepare_inputs."""
    plan = PredictPlan(model, prepared if prepared is not None else prepare_inputs(model, inputs_list, index))
    est = plan()
    if defer_check:
        model._pending_info.append(plan.info_acc)
    elif int(plan.info_acc.max().cpu()) != 0:
        raise torch.linalg.LinAlgError("cholesky: K22 + 1e-4 I is not positive-definite")
    return est


# ==================================================================================== sampling (§8f f1)
class _Draws:
    """Standard normals in the reference's call order per sample (code/nmgp_dsvi.py:436-476):
    z_v (M), z_t (N), Q x (N) pair noise in (i, j <= i) order, G (D, N), then z_F.  ``tape`` (a flat
    float64 vector, tests only) replays recorded reference noise; otherwise draws come from the
    HIP Philox generator seeded from torch's CPU generator (so ``torch.manual_seed`` makes runs
    reproducible; the stream itself is not the reference's float32 CPU stream)."""

    def __init__(self, dev, tape=None):
        self.dev, self.pos = dev, 0
        self.tape = None if tape is None else torch.as_tensor(np.asarray(tape, np.float64)).to(dev)
        self.seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if tape is None else 0

    def take(self, S, per_sample):
        """(S, per_sample) block: the next S samples' noise."""
        n = S * per_sample
        if self.tape is not None:
            out = self.tape[self.pos:self.pos + n]
            assert out.numel() == n, "noise tape exhausted"
        else:
            out = H.normal_(torch.empty(n, dtype=F64, device=self.dev), self.seed, offset=self.pos)
        self.pos += n
        return out.reshape(S, per_sample)

    def rewind(self):
        """Back to the first sample: the same takes give the same noise again (the tape, or Philox, which is a
        pure function of (seed, position))."""
        self.pos = 0


def _tril(t):
    return torch.tril(t)


def _chol_inv_checked(A, what):
    Ci, info = H.chol_inv_(A)
    if int(info.max().cpu()) != 0:
        raise torch.linalg.LinAlgError(f"cholesky: {what} + 1e-4 I is not positive-definite")
    return A, Ci                                                         # A now holds L


def _proj_var(K12, K22, d11):
    """P = K12 (K22 + 1e-4 I)^-1 and d11 - rowsum(P o K12) (code/utils.py:117-120)."""
    A = K22.clone()
    A.diagonal().add_(JIT)
    _, Ci = _chol_inv_checked(A, "K22")
    Ainv = H.matmul(Ci, Ci, transA=True, maskA=L.A_UPPER, maskB=L.B_LOWER)
    P = H.matmul(K12, Ainv)
    return P, d11 - (P * K12).sum(1)


def _sampling_setup(model, x):
    """Everything the samples share: P, means and variances of the three RBF-prior GPs (the pair
    marginals do not depend on the sample), the Cholesky factor of Sigma_v, tril(sqrt_W)."""
    dev = model.device_
    D, M = model.D, model.M
    Z = model.Z
    p = {k: getattr(model, k).detach().to(F64) for k in ["mu_W", "sqrt_W", "mu_v", "sqrt_v"]}
    p["mu_U"] = model.mu_U_dense().to(F64)
    hyp = {k: float(torch.exp(getattr(model, k).detach().to(F64))) for k in
           ["sigma2_tildeell_log", "length_scales_tildeell_log", "sigma2_L0_log", "length_scales_L0_log",
            "sigma2_L1_log", "length_scales_L1_log", "sigma2_err_log"]}
    N = x.shape[0]

    def rbf(a, b, s2, ls):
        return H.pairwise(a, b, mode=L.RBF, scale2=s2, length_scale=ls)

    st = {"N": N, "D": D, "M": M, "Z": Z, "x": x, "mu_W": p["mu_W"], "s2_err": hyp["sigma2_err_log"]}
    Kt12 = rbf(x, Z, hyp["sigma2_tildeell_log"], hyp["length_scales_tildeell_log"])
    Kt22 = rbf(Z, Z, hyp["sigma2_tildeell_log"], hyp["length_scales_tildeell_log"])
    st["Pt"], st["var_t"] = _proj_var(Kt12, Kt22, torch.full((N,), hyp["sigma2_tildeell_log"], dtype=F64,
                                                              device=dev))
    # v ~ N(mu_v, Sigma_v): chol(Sigma_v + 1e-4 I) (code/utils.py:40-47, 225-226)
    lv = _tril(p["sqrt_v"])
    Sv = H.matmul(lv, lv, transB=True, maskA=L.A_LOWER, maskB=L.B_UPPER)
    Sv.diagonal().add_(JIT)
    st["Cv"], _ = _chol_inv_checked(Sv, "Sigma_v")
    st["mu_v"] = p["mu_v"]
    # pair marginals (code/utils.py:106-125): mean P mu_ij, variance d - rowsum(P o K12) +
    # rowsum((P tril(S_ij))^2)  (= rowsum((P Sigma_ij) o P) since Sigma_ij = tril(S) tril(S)^T)
    K012 = rbf(x, Z, hyp["sigma2_L0_log"], hyp["length_scales_L0_log"])
    K022 = rbf(Z, Z, hyp["sigma2_L0_log"], hyp["length_scales_L0_log"])
    K112 = rbf(x, Z, hyp["sigma2_L1_log"], hyp["length_scales_L1_log"])
    K122 = rbf(Z, Z, hyp["sigma2_L1_log"], hyp["length_scales_L1_log"])
    P0, b0 = _proj_var(K012, K022, torch.full((N,), hyp["sigma2_L0_log"], dtype=F64, device=dev))
    P1, b1 = _proj_var(K112, K122, torch.full((N,), hyp["sigma2_L1_log"], dtype=F64, device=dev))
    pairs = [(i, j) for i in range(D) for j in range(i + 1)]
    mus, sds = [], []
    for (i, j) in pairs:
        P, base = (P1, b1) if i == j else (P0, b0)
        mus.append(H.matmul(P, p["mu_U"][i, j].reshape(M, 1).contiguous()).reshape(N))
        PL = H.matmul(P, _tril(model.sqrt_U_pair(i, j).detach().to(F64)).contiguous(), maskB=L.B_LOWER)
        sds.append(torch.sqrt(base + (PL * PL).sum(1) + JIT))
    st["pairs"], st["pair_mu"], st["pair_sd"] = pairs, torch.stack(mus), torch.stack(sds)   # (Q, N)
    st["lW"] = _tril(p["sqrt_W"]).contiguous()                           # (D, M, M)
    return st


def _noise_layout(st, fy):
    """The noise of one sample, in the reference's call order: [z_v M][z_t N][z_p Q N][z_g D N][z_f], z_f being N D
    wide for the sample_FY family (fy=True) and N wide for the sample_Y family -> (per, o_p, o_g, o_f): the length of
    the block and the offsets of z_p, z_g and z_f in it."""
    N, D, M = st["N"], st["D"], st["M"]
    o_p = M + N
    o_g = o_p + len(st["pairs"]) * N
    o_f = o_g + D * N
    return o_f + (N * D if fy else N), o_p, o_g, o_f


def _chunks(draws, n_sample, chunk, per, rewind=False):
    """The walk over the noise stream in chunks of up to `chunk` samples: yields (done, S, zc), zc the (S, per) noise
    of the samples done .. done + S.  rewind=True starts the stream over first, so the walk sees the noise of the
    walk before it."""
    if rewind:
        draws.rewind()
    done = 0
    while done < n_sample:
        S = min(chunk, n_sample - done)
        yield done, S, draws.take(S, per)
        done += S


def _check_sampling_args(quantiles, n_sample):
    """quantiles and n_sample of the summaries -> ([float], int), ValueError where they make no sense."""
    qs = [float(q) for q in quantiles]
    if any(not 0.0 <= q <= 1.0 for q in qs):
        raise ValueError("quantiles must lie in [0, 1]")
    n_sample = int(n_sample)
    if n_sample < 1:
        raise ValueError("n_sample must be at least 1")
    return qs, n_sample


def _sample_T_moments(st, zc):
    """The part of a chunk that every sampler shares up to the latent's marginals: tilde-ell T (S, N) and, given it,
    the MGP_d marginals of the latent G, mu_g (S, N, D) and var_g (S, D, N), of S samples from their noise block zc
    (S, per-sample noise, laid out as _noise_layout says).  Also returns the column offsets of z_p, z_g and z_f in
    zc."""
    N, D, M = st["N"], st["D"], st["M"]
    S = zc.shape[0]
    _, o_p, o_g, o_f = _noise_layout(st, False)                          # the offsets do not depend on z_f's width
    z_v, z_t = zc[:, :M], zc[:, M:o_p]
    # v = mu_v + chol(Sigma_v + 1e-4 I) z_v ; t = P_t v + sqrt(var_t + 1e-4) z_t   (JGP_S)
    V = st["mu_v"].reshape(1, M) + H.matmul(z_v.contiguous(), st["Cv"], transB=True, maskB=L.B_UPPER)
    T = H.matmul(V, st["Pt"], transB=True) + torch.sqrt(st["var_t"] + JIT).reshape(1, N) * z_t
    # G | ell  (MGP_d with the sample's Gibbs kernel; code/nmgp_dsvi.py:468-472)
    ellZ, ellX = torch.exp(V), torch.exp(T)
    KG12 = torch.empty(S, N, M, dtype=F64, device=V.device)
    KG22 = torch.empty(S, M, M, dtype=F64, device=V.device)
    descs = []
    for s_ in range(S):
        descs.append(H.pairwise_desc(KG12[s_], st["x"], st["Z"], mode=L.GIBBS, ellX=ellX[s_], ellZ=ellZ[s_]))
        descs.append(H.pairwise_desc(KG22[s_], st["Z"], st["Z"], mode=L.GIBBS, ellX=ellZ[s_], ellZ=ellZ[s_]))
    H.PairwiseGroup(descs, V.device)(F64)
    A = KG22.clone()
    A.diagonal(dim1=1, dim2=2).add_(JIT)
    _, Ci = _chol_inv_checked(A, "K_G22")
    Ainv = H.bmm(Ci, Ci, transA=True, maskA=L.A_UPPER, maskB=L.B_LOWER)
    PG = H.bmm(KG12, Ainv)                                               # (S, N, M)
    mu_g = H.bmm(PG, st["mu_W"].contiguous(), transB=True)              # (S, N, D)
    var0 = 1.0 - (PG * KG12).sum(2)                                      # (S, N)
    var_g = torch.empty(S, D, N, dtype=F64, device=V.device)
    for d in range(D):
        PL = H.bmm(PG, st["lW"][d], maskB=L.B_LOWER)
        var_g[:, d] = var0 + (PL * PL).sum(2)
    return T, mu_g, var_g, o_p, o_g, o_f


def _sample_TG(st, zc):
    """The part of a chunk that sample_Y, sample_FY and summarize_FY share: tilde-ell T (S, N) and the latent
    G (S, D, N) drawn from the marginals of _sample_T_moments with the z_g of the noise block.  Also returns the
    column offsets of z_p and z_f in zc."""
    N, D = st["N"], st["D"]
    S = zc.shape[0]
    T, mu_g, var_g, o_p, o_g, o_f = _sample_T_moments(st, zc)
    z_g = zc[:, o_g:o_g + D * N].reshape(S, D, N)
    G = mu_g.transpose(1, 2) + torch.sqrt(var_g + JIT) * z_g           # (S, D, N)
    return T, G, o_p, o_f


def _sample_chunk(st, zc, fy):
    """S samples from their noise block zc (S, per-sample noise).  Returns t (S,N), Lfull (S,D,D,N),
    G (S,D,N) and the F-noise (S, N) or (S, N, D)."""
    N, D = st["N"], st["D"]
    Q = len(st["pairs"])
    S = zc.shape[0]
    T, G, o_p, o_f = _sample_TG(st, zc)
    z_p = zc[:, o_p:o_p + Q * N].reshape(S, Q, N)
    z_f = zc[:, o_f:].reshape(S, N, D) if fy else zc[:, o_f:o_f + N]
    # pair samples (S, Q, N); the diagonal pairs are log L_ii
    Ls = st["pair_mu"].unsqueeze(0) + st["pair_sd"].unsqueeze(0) * z_p
    Lfull = torch.zeros(S, D, D, N, dtype=F64, device=T.device)
    for q, (i, j) in enumerate(st["pairs"]):
        Lfull[:, i, j] = torch.exp(Ls[:, q]) if i == j else Ls[:, q]
    return T, Lfull, G, z_f


def _chunk_size(n_sample, N, M):
    return max(1, min(n_sample, (1 << 25) // max(1, N * M)))


def sample_Y(model, X_list, n_sample=1000, index=None, noise_tape=None):
    """NMGP.sample_Y (code/nmgp_dsvi.py:406-490) on the device -> (Ys (S, N), Ls (S, N, D),
    Gs (S, D, N), tilde_ells (S, N)), torch tensors on the model's device."""
    dev = model.device_
    x, I = prepare_inputs(model, X_list, index)
    st = _sampling_setup(model, x)
    N, M = st["N"], st["M"]
    per = _noise_layout(st, False)[0]
    sd_err = (st["s2_err"] + JIT) ** 0.5
    rows = torch.arange(N, device=dev)
    Ys, Ls, Gs, Ts = [], [], [], []
    for _, _, zc in _chunks(_Draws(dev, noise_tape), n_sample, _chunk_size(n_sample, N, M), per):
        T, Lfull, G, z_f = _sample_chunk(st, zc, fy=False)
        l = Lfull.permute(0, 3, 1, 2)[:, rows, I]                       # (S, N, D): row I_n of L
        F = (l * G.transpose(1, 2)).sum(2)
        Ys.append(F + sd_err * z_f), Ls.append(l), Gs.append(G), Ts.append(T)
    return torch.cat(Ys), torch.cat(Ls), torch.cat(Gs), torch.cat(Ts)


def sample_FY(model, x, n_sample=1000, noise_tape=None):
    """NMGP.sample_FY (code/nmgp_dsvi.py:492-580) on the device -> (tilde_ells (S, N),
    Ys (S, N, D), corrs (S, N, D, D))."""
    dev = model.device_
    x = torch.as_tensor(x).reshape(-1, 1).to(F64).to(dev).contiguous()
    st = _sampling_setup(model, x)
    per = _noise_layout(st, True)[0]
    sd_err = (st["s2_err"] + JIT) ** 0.5
    Ts, Ys, Cs = [], [], []
    for _, _, zc in _chunks(_Draws(dev, noise_tape), n_sample, _chunk_size(n_sample, st["N"], st["M"]), per):
        T, Lfull, G, z_f = _sample_chunk(st, zc, fy=True)
        Ln = Lfull.permute(0, 3, 1, 2)                                   # (S, N, D, D)
        F = torch.matmul(Ln, G.transpose(1, 2).unsqueeze(3))[..., 0]     # (S, N, D)
        cov = torch.matmul(Ln, Ln.transpose(2, 3))
        invstd = torch.sqrt(torch.diag_embed(1.0 / torch.diagonal(cov, dim1=-2, dim2=-1)))
        Ts.append(T), Ys.append(F + sd_err * z_f), Cs.append(torch.matmul(torch.matmul(invstd, cov), invstd))
    return torch.cat(Ts), torch.cat(Ys), torch.cat(Cs)


def _quantiles_dim0(t, qs):
    """np.quantile(t, qs, axis=0) (linear interpolation between the order statistics) by a sort along dim 0:
    torch.quantile refuses inputs above 16 M elements."""
    S = t.shape[0]
    srt = torch.sort(t, dim=0).values
    out = []
    for q in qs:
        pos = float(q) * (S - 1)
        lo = min(max(int(np.floor(pos)), 0), S - 1)
        hi = min(lo + 1, S - 1)
        out.append(torch.lerp(srt[lo], srt[hi], pos - lo))
    return torch.stack(out)


def _parse_corr_pairs(corr_pairs, D):
    """corr_pairs of summarize_FY -> (P, 2) int64 CPU tensor: "all" is every (i, j < i) in row order, else a
    sequence of (i, j) with 0 <= i, j < D, order and duplicates kept."""
    if isinstance(corr_pairs, str):
        if corr_pairs != "all":
            raise ValueError('corr_pairs: the only string accepted is "all"')
        lst = [(i, j) for i in range(D) for j in range(i)]
    else:
        try:
            lst = [tuple(int(v) for v in p) for p in corr_pairs]
        except (TypeError, ValueError):
            raise ValueError('corr_pairs must be None, "all" or a sequence of (i, j) pairs') from None
        if any(len(p) != 2 for p in lst):
            raise ValueError("corr_pairs: every entry must be an (i, j) pair")
        if any(not (0 <= i < D and 0 <= j < D) for i, j in lst):
            raise ValueError(f"corr_pairs: output indices must lie in 0..{D - 1}")
    return torch.tensor(lst, dtype=torch.long).reshape(len(lst), 2)


def _parse_corr_groups(corr_groups, D):
    """corr_groups of summarize_FY -> list of K >= 1 non-empty lists of (i, j) with 0 <= i, j < D, order and
    duplicates kept; ValueError for anything else (an empty outer sequence, an empty group, an entry that is not a
    pair, an index out of range, a string)."""
    if isinstance(corr_groups, (str, bytes)):
        raise ValueError("corr_groups must be None or a sequence of groups of (i, j) pairs, not a string")
    try:
        groups = [list(g) for g in corr_groups]
        if any(isinstance(p, (str, bytes)) for g in groups for p in g):
            raise TypeError
        lst = [[tuple(int(v) for v in p) for p in g] for g in groups]
        if any(float(v) != int(v) for g in groups for p in g for v in p):
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError("corr_groups must be None or a sequence of groups of (i, j) pairs") from None
    if len(lst) == 0:
        raise ValueError("corr_groups: at least one group")
    if any(len(g) == 0 for g in lst):
        raise ValueError("corr_groups: a group may not be empty")
    if any(len(p) != 2 for g in lst for p in g):
        raise ValueError("corr_groups: every entry must be an (i, j) pair")
    if any(not (0 <= i < D and 0 <= j < D) for g in lst for i, j in g):
        raise ValueError(f"corr_groups: output indices must lie in 0..{D - 1}")
    return lst


def _parse_spectrum(spectrum, D):
    """spectrum of summarize_FY -> k: "all" is D, else a plain int with 1 <= k <= D (a bool is refused); ValueError
    for anything else."""
    if isinstance(spectrum, str):
        if spectrum != "all":
            raise ValueError('spectrum: the only string accepted is "all"')
        return D
    if isinstance(spectrum, bool) or not isinstance(spectrum, (int, np.integer)):
        raise ValueError('spectrum must be None, "all" or an int k with 1 <= k <= D')
    if not 1 <= int(spectrum) <= D:
        raise ValueError(f"spectrum: k must lie in 1..{D}")
    return int(spectrum)


def groups_from_labels(labels, between=True):
    """Within- and between-network groups for summarize_FY(corr_groups=...) from one hashable label per output ->
    (groups, names).  For every label a with at least two members, in order of first appearance: the group of all
    (i, j < i) with both outputs in a, named (a, a).  With between=True then, for every unordered pair of labels
    a != b in the same order: the group of all (i, j < i) with one output in a and the other in b, named (a, b).
    A label with a single member gets no within group.  When no label is a singleton and between=True, the groups
    partition the D (D - 1) / 2 pairs."""
    labels = list(labels)
    order, members = [], {}
    for i, a in enumerate(labels):
        if a not in members:
            members[a] = []
            order.append(a)
        members[a].append(i)
    groups, names = [], []
    for a in order:
        if len(members[a]) >= 2:
            groups.append([(i, j) for i in members[a] for j in members[a] if j < i])
            names.append((a, a))
    if between:
        for x, a in enumerate(order):
            for b in order[x + 1:]:
                groups.append(sorted((max(i, j), min(i, j)) for i in members[a] for j in members[b]))
                names.append((a, b))
    return groups, names


def _pop_sd(sq_mean, mean):
    return torch.sqrt(torch.clamp(sq_mean - mean * mean, min=0.0))


def _lpd(lse_max, lse_sum, ok, n_sample):
    """log mean_s exp(ll_s) from the log-sum-exp state of the n_sample log densities; NaN where not ok (unscored)."""
    nan = torch.full((), float("nan"), dtype=F64, device=ok.device)
    return torch.where(ok, lse_max + torch.log(lse_sum) - float(np.log(n_sample)), nan)


def _group_stats(Gb, qs):
    """Mean, population sd and quantiles over the samples of the collected group means Gb (groups, N, S) ->
    (N, groups), (N, groups), (len(qs), N, groups).  Mean and sd are taken group by group on (N, S) blocks, so
    that their bits do not depend on how many groups share the buffer; a NaN sample makes its (n, k) NaN."""
    means, sds = [], []
    for k in range(Gb.shape[0]):
        m = Gb[k].mean(1)
        means.append(m)
        sds.append(torch.sqrt(((Gb[k] - m.unsqueeze(1)) ** 2).mean(1)))
    return torch.stack(means, 1), torch.stack(sds, 1), _band_quantiles(Gb, qs)


def _band_quantiles(C, qs):
    """Quantiles along the last axis of the collected correlations C (pairs, N, S) -> (len(qs), N, pairs): the
    LDS sort of csrc/corrq.hip, or, for more samples than one workgroup sorts, torch.sort and the same
    interpolation (a row with a NaN is NaN, as np.quantile has it)."""
    pb, N, S = C.shape
    if S <= H.quantile_rows_max_S():
        out = H.quantile_rows(C.reshape(pb * N, S), qs)
    else:
        srt = torch.sort(C.reshape(pb * N, S), dim=1).values
        bad = torch.isnan(srt[:, -1])
        rows = []
        for q in qs:
            pos = q * (S - 1)
            lo = min(max(int(np.floor(pos)), 0), S - 1)
            hi = min(lo + 1, S - 1)
            r = srt[:, lo] if pos == lo else torch.lerp(srt[:, lo], srt[:, hi], pos - lo)
            rows.append(torch.where(bad, torch.full_like(r, float("nan")), r))
        out = torch.stack(rows)
    return out.reshape(len(qs), pb, N).permute(0, 2, 1)


def _pair_bands(walk, st, o_p, qs, pi, pj, pb, Cb, Pb):
    """The quantile bands of the P listed pairs, pb pairs at a time -> (cq, pq), each (len(qs), N, P); pq is None
    without Pb.  The main pass has collected the first batch into Cb (pb, N, S) and, with partial, Pb; every further
    batch walks the noise stream again (walk() yields _chunks from position 0) and launches only the collectors."""
    P, N = pi.numel(), Cb.shape[1]
    cq = torch.empty(len(qs), N, P, dtype=F64, device=Cb.device)
    pq = None if Pb is None else torch.empty_like(cq)
    for p0 in range(0, P, pb):
        p1 = min(P, p0 + pb)
        if p0 > 0:
            for done, _, zc in walk():
                H.corr_collect_(st["pair_mu"], st["pair_sd"], zc[:, o_p:], pi[p0:p1], pj[p0:p1], Cb[:p1 - p0],
                                s_off=done)
                if Pb is not None:
                    H.pcorr_accum_(st["pair_mu"], st["pair_sd"], zc[:, o_p:], pi=pi[p0:p1], pj=pj[p0:p1],
                                   C=Pb[:p1 - p0], s_off=done)
                del zc                                                    # freed before the next chunk is drawn
        cq[:, :, p0:p1] = _band_quantiles(Cb[:p1 - p0], qs)
        if Pb is not None:
            pq[:, :, p0:p1] = _band_quantiles(Pb[:p1 - p0], qs)
    return cq, pq


def _group_bands(walk, st, o_p, qs, tabs, Gb, PGb):
    """Mean, sd and quantiles of the group means, one table of tabs at a time -> (stats, pstats), each the list of
    the batches' _group_stats; pstats is empty without PGb.  The main pass has collected the groups of tabs[0] into
    Gb (and, with partial, PGb); every further table walks the noise stream again and launches only the group
    kernels."""
    stats, pstats = [], []
    for b, (goff, gent) in enumerate(tabs):
        kb = goff.numel() - 1
        if b > 0:
            for done, _, zc in walk():
                H.corr_group_(st["pair_mu"], st["pair_sd"], zc[:, o_p:], goff, gent, Gb[:kb], s_off=done)
                if PGb is not None:
                    H.pcorr_accum_(st["pair_mu"], st["pair_sd"], zc[:, o_p:], goff=goff, gent=gent, Cg=PGb[:kb],
                                   sg_off=done)
                del zc                                                    # freed before the next chunk is drawn
        stats.append(_group_stats(Gb[:kb], qs))
        if PGb is not None:
            pstats.append(_group_stats(PGb[:kb], qs))
    return stats, pstats


def _group_keys(prefix, stats):
    """The batches' (mean, sd, quantiles) side by side along the group axis, under the keys of summarize_FY."""
    return {prefix + "_mean": torch.cat([v[0] for v in stats], 1), prefix + "_sd": torch.cat([v[1] for v in stats], 1),
            prefix + "_quantiles": torch.cat([v[2] for v in stats], 2)}


def summarize_FY(model, x, n_sample=1000, quantiles=(0.025, 0.975), noise_tape=None, keep_samples=False,
                 corr_pairs=None, band_bytes=1 << 30, partial=False, corr_groups=None, spectrum=None):
    """What the reference's drivers keep of NMGP.sample_FY (code/nmgp_dsvi.py:492-580; NMGP_ECoG_full.py:329-332):
    means and quantile bands of tilde_ell and Y, mean and population sd of the output correlations, as a dict of
    device tensors.  Same setup, chunking, noise layout and stream as sample_FY; each chunk's tail (pair samples,
    L, Y, L L^T, normalisation, accumulation over the samples) is one fused launch (csrc/fy.hip), so only
    O(S N D + N D^2) is ever stored -- the (S, N, D, D) correlation samples are not.  keep_samples=True adds
    Ys (S, N, D) and tilde_ells (S, N).

    corr_pairs ("all" = every (i, j < i) in row order, or a sequence of (i, j)) adds the credible bands the
    reference plots (code/utils.py:354-366, plot_corrs): "corr_pairs" (P, 2) int64 and "corr_quantiles"
    (len(quantiles), N, P), whose [:, :, p] is np.quantile(corrs[:, :, i, j], quantiles, axis=0) of the very
    samples whose mean is corr_mean.  The pairs are taken in batches of max(1, band_bytes // (8 S N)): a batch's
    samples (pairs, N, S) are collected chunk by chunk (csrc/corrq.hip) and sorted inside LDS.  The first batch
    rides along with the summary's chunks; every further batch walks the same noise stream again (the tape, or
    Philox from position 0 with the same seed) and runs neither the sampling head nor fy.hip.  The result does not
    depend on band_bytes.  With n_sample above hip_ops.quantile_rows_max_S() (16384) the collected batch is sorted
    by torch.sort instead, with the same interpolation; that sort holds a second copy of the batch.

    partial=True adds the partial correlations of the outputs -- the correlation of outputs i and j given all the
    others, -Omega_ij / sqrt(Omega_ii Omega_jj) with Omega = (L L^T)^-1 the sample's precision matrix, diagonal 1 --
    as "pcorr_mean" and "pcorr_sd" (N, D, D; population sd, as corr_sd): the mean of the samples' partial
    correlations, not the partial correlation of corr_mean.  Each chunk is one more fused launch (csrc/pcorr.hip:
    L^-1 and L^-T L^-1 per sample and input inside one workgroup's LDS), again without an (S, N, D, D) tensor.  With
    corr_pairs it also adds "pcorr_quantiles" (len(quantiles), N, P) for the same pair list, collected by the same
    kernel into a second (pairs, N, S) batch buffer of the size band_bytes allows and sorted like the correlation
    bands; the further batches run that kernel in collect-only mode.  A sample whose L has a zero or non-finite
    diagonal entry at an input (an exp that under- or overflowed) is NaN in every partial correlation at that input.
    With partial=False nothing is launched or returned for it.

    corr_groups (a sequence of K >= 1 non-empty groups of (i, j) pairs, e.g. from groups_from_labels) adds what the
    reference's ECoG driver plots (NMGP_ECoG_full.py:456-544): the correlations averaged over groups of pairs.  Per
    sample and input the group value is the plain mean of the group's correlations -- order and duplicates kept (a
    pair listed twice counts twice), (i, j) = (j, i), (i, i) exactly 1 where finite, groups may overlap -- of the
    very samples whose mean is corr_mean.  Keys: "corr_group_sizes" (K,) int64, "corr_group_mean" and
    "corr_group_sd" (N, K; population sd over the samples), "corr_group_quantiles" (len(quantiles), N, K; exact,
    sorted like the pair bands); with partial=True also "pcorr_group_mean" / "pcorr_group_sd" /
    "pcorr_group_quantiles" of the group means of the samples' partial correlations; with keep_samples=True also
    "corr_group_samples" (K, N, S) (and "pcorr_group_samples"), from which any contrast between groups or inputs
    can be formed.  A group that contains a NaN correlation at (s, n) is NaN there, and then so are that (n, k)'s
    mean, sd and quantiles.  The reduction over the pairs happens next to the correlation matrix in LDS
    (csrc/cgroup.hip; for the partial correlations inside csrc/pcorr.hip), one more launch per chunk; only the
    (groups, N, S) group samples are stored.  The groups are taken in batches of max(1, band_bytes // (8 S N)),
    independently of the pair batches: the first rides along with the summary's chunks, every further batch walks
    the noise stream again and launches only the group kernels.  The result does not depend on band_bytes.  With
    keep_samples=True the buffer is the full (K, N, S), whatever band_bytes says.  Anything else than None or such
    a sequence raises ValueError before any device work; with None nothing is launched or returned.

    spectrum (a plain int k with 1 <= k <= D, or "all" for k = D) adds the eigenvalues of every sample's correlation
    matrix at every input: how many independent modes the outputs have at x and how strong the common mode is.  The
    matrix has trace D, so lambda / D is a mode's share.  Keys: "eig_mean" and "eig_sd" (N, k; mean and population
    sd over the samples of the r-th largest eigenvalue), "eig_quantiles" (len(quantiles), N, k; exact, sorted like
    the pair bands), "eff_dim_mean" / "eff_dim_sd" (N,) and "eff_dim_quantiles" (len(quantiles), N) of the effective
    dimension (participation ratio) D^2 / sum_j lambda_j^2 over all D eigenvalues, "eig_loading2_mean" (N, k, D), the
    mean over the samples of the squared loading u_rd^2 of output d on mode r (sign-free, each mode's sums to 1), and
    "spectrum_unconverged", a 0-d int tensor counting the finite (sample, input) whose solve ran out of sweeps (0 on
    everything tested); with keep_samples=True also "eig_samples" (k, N, S) and "eff_dim_samples" (N, S).  The mean
    of the samples' eigenvalues is not the eigenvalues of corr_mean.  Modes are identified by rank, so two modes
    whose eigenvalues cross over x swap labels there (and their loadings with them).  A sample whose L has a zero or
    non-finite diagonal entry at an input (or that did not converge) is NaN in every eigenvalue and the effective
    dimension at that input, and then so are that input's means, sds, quantiles and loadings.  Each chunk is one
    more fused launch (csrc/spectrum.hip: one-sided Jacobi on diag(Is) L inside one workgroup's LDS), no second
    walk of the noise stream and no (S, N, D, D) tensor.  The sample buffer is the full 8 (k + 1) S N bytes and is
    not batched by band_bytes: a further batch would repeat the whole solve.  Anything else raises ValueError before
    any device work; with None nothing is launched or returned."""
    qs, n_sample = _check_sampling_args(quantiles, n_sample)
    pairs_t = None if corr_pairs is None else _parse_corr_pairs(corr_pairs, model.D)
    groups = None if corr_groups is None else _parse_corr_groups(corr_groups, model.D)
    kspec = 0 if spectrum is None else _parse_spectrum(spectrum, model.D)
    dev = model.device_
    x = torch.as_tensor(x).reshape(-1, 1).to(F64).to(dev).contiguous()
    st = _sampling_setup(model, x)
    N, D, M = st["N"], st["D"], st["M"]
    if D > 128:
        raise ValueError("summarize_FY: the fused kernel holds L in one workgroup's LDS, D <= 128")
    per, o_p, _, o_f = _noise_layout(st, True)
    draws = _Draws(dev, noise_tape)
    sd_err = (st["s2_err"] + JIT) ** 0.5
    Ts = torch.empty(n_sample, N, dtype=F64, device=dev)
    Ys = torch.empty(n_sample, N, D, dtype=F64, device=dev)
    csum = torch.zeros(N, D, D, dtype=F64, device=dev)
    csq = torch.zeros(N, D, D, dtype=F64, device=dev)
    chunk = _chunk_size(n_sample, N, M)
    ws = H.fy_workspace(D, N, chunk, dev)
    P = 0 if pairs_t is None else pairs_t.shape[0]
    Pb = PGb = None                                                      # the partial-correlation batch buffers
    if partial:
        psum = torch.zeros(N, D, D, dtype=F64, device=dev)
        psq = torch.zeros(N, D, D, dtype=F64, device=dev)
        pws = H.pcorr_workspace(D, N, chunk, dev)
    if P:
        pb = min(P, max(1, int(band_bytes) // (8 * n_sample * N)))       # pairs per batch
        pij = pairs_t.to(torch.int32).to(dev)
        pi, pj = pij[:, 0].contiguous(), pij[:, 1].contiguous()
        Cb = torch.empty(pb, N, n_sample, dtype=F64, device=dev)
        if partial:
            Pb = torch.empty(pb, N, n_sample, dtype=F64, device=dev)
    K = 0 if groups is None else len(groups)
    if K:
        # groups per batch; the kept samples are one buffer of all the groups
        gb = K if keep_samples else min(K, max(1, int(band_bytes) // (8 * n_sample * N)))
        tabs = [H.group_table(groups[k0:k0 + gb], D, dev) for k0 in range(0, K, gb)]
        Gb = torch.empty(gb, N, n_sample, dtype=F64, device=dev)
        if partial:
            PGb = torch.empty(gb, N, n_sample, dtype=F64, device=dev)
    if kspec:
        Eb = torch.empty(kspec + 1, N, n_sample, dtype=F64, device=dev)  # the top k eigenvalues, then eff_dim
        l2sum = torch.zeros(N, kspec, D, dtype=F64, device=dev)
        unconv = torch.zeros(1, dtype=torch.int32, device=dev)
        sws = H.spectrum_workspace(D, N, chunk, kspec, dev)
    # ---- the main pass: the sampling head and the fused tails of every chunk, the first batches riding along
    for done, S, zc in _chunks(draws, n_sample, chunk, per):
        T, G, _, _ = _sample_TG(st, zc)
        Ts[done:done + S] = T
        H.fy_accum_(st["pair_mu"], st["pair_sd"], G.contiguous(), zc[:, o_p:], zc[:, o_f:], sd_err,
                    Ys[done:done + S], csum, csq, ws=ws)
        if P:
            H.corr_collect_(st["pair_mu"], st["pair_sd"], zc[:, o_p:], pi[:pb], pj[:pb], Cb, s_off=done)
        if K:
            H.corr_group_(st["pair_mu"], st["pair_sd"], zc[:, o_p:], tabs[0][0], tabs[0][1], Gb, s_off=done)
        if partial:
            # one launch: L^-1 and Omega once, for the sums, the pair list and the groups
            kw = {"pi": pi[:pb], "pj": pj[:pb], "C": Pb, "s_off": done} if P else {}
            if K:
                kw.update(goff=tabs[0][0], gent=tabs[0][1], Cg=PGb, sg_off=done)
            H.pcorr_accum_(st["pair_mu"], st["pair_sd"], zc[:, o_p:], psum, psq, ws=pws, **kw)
        if kspec:
            H.corr_spectrum_(st["pair_mu"], st["pair_sd"], zc[:, o_p:], kspec, Eb, unconv, s_off=done,
                             load2_sum=l2sum, ws=sws)
    mean = csum / n_sample
    out = {"tilde_ell_mean": Ts.mean(0), "tilde_ell_quantiles": _quantiles_dim0(Ts, qs),
           "Y_mean": Ys.mean(0), "Y_quantiles": _quantiles_dim0(Ys, qs),
           "corr_mean": mean, "corr_sd": _pop_sd(csq / n_sample, mean)}
    if partial:
        pmean = psum / n_sample
        out["pcorr_mean"], out["pcorr_sd"] = pmean, _pop_sd(psq / n_sample, pmean)
    if keep_samples:
        out["Ys"], out["tilde_ells"] = Ys, Ts
    walk = lambda: _chunks(draws, n_sample, chunk, per, rewind=True)
    # ---- the pair bands: the chunk's G, T and noise are released before the further batches walk the stream again
    if pairs_t is not None:
        if P:
            del G, T, zc
            cq, pq = _pair_bands(walk, st, o_p, qs, pi, pj, pb, Cb, Pb)
        else:
            cq = torch.empty(len(qs), N, 0, dtype=F64, device=dev)
            pq = torch.empty(len(qs), N, 0, dtype=F64, device=dev)
        out["corr_pairs"], out["corr_quantiles"] = pairs_t.to(dev), cq
        if partial:
            out["pcorr_quantiles"] = pq
    # ---- the group bands, likewise
    if K:
        G = T = zc = None
        stats, pstats = _group_bands(walk, st, o_p, qs, tabs, Gb, PGb)
        out["corr_group_sizes"] = torch.tensor([len(g) for g in groups], dtype=torch.long, device=dev)
        out.update(_group_keys("corr_group", stats))
        if partial:
            out.update(_group_keys("pcorr_group", pstats))
        if keep_samples:
            out["corr_group_samples"] = Gb
            if partial:
                out["pcorr_group_samples"] = PGb
    # ---- the eigenvalue bands: rows 0..k-1 of the buffer are the eigenvalues, row k the effective dimension
    if kspec:
        G = T = zc = None
        em, es, eq = _group_stats(Eb, qs)
        out["eig_mean"], out["eig_sd"], out["eig_quantiles"] = em[:, :kspec], es[:, :kspec], eq[:, :, :kspec]
        out["eff_dim_mean"], out["eff_dim_sd"], out["eff_dim_quantiles"] = em[:, kspec], es[:, kspec], eq[:, :, kspec]
        out["eig_loading2_mean"] = l2sum / n_sample
        out["spectrum_unconverged"] = unconv[0]
        if keep_samples:
            out["eig_samples"], out["eff_dim_samples"] = Eb[:kspec], Eb[kspec]
    return out


def score_mixture(Mu, Var, y=None, quantiles=(), crps=True):
    """Exact scores of E predictives that are equal-weight mixtures of S Gaussians -- what summarize_Y (components
    N(F_sn, s2)) and impute_Y (components N(mu_se, v_se)) end in -- from the component buffers, e.g. the
    keep_samples outputs: Mu (S, E) float64 device tensor, Var the same shape or one positive number.  One fused
    pass (csrc/mixscore.hip), closed forms throughout, no Monte-Carlo noise.  A dict of device tensors:
    with crps=True "crps_spread" (E,), the term (1 / 2 S^2) sum_s sum_t A(mu_s - mu_t, v_s + v_t) of the CRPS that
    needs no truth; with y (E,) "pit" (E,), the mixture CDF at the truth, and with crps=True also "crps" (E,) and
    "mean_crps" over the entries with a finite y (0 / 0 = NaN, like mean_lpd); with quantiles (probabilities
    strictly inside (0, 1)) "quantiles" (len(quantiles), E), the exact roots of the mixture CDF, bisected down to
    adjacent doubles, and "unconverged" (1,) int32, the number of quantiles that did not get there (NaN; 0 in every
    case tried).  An entry with a non-finite mean or a variance that is not finite and positive is NaN throughout;
    a non-finite y[e] makes pit[e] and crps[e] NaN only.  Argument errors raise ValueError before any device
    work."""
    got = H.mix_score_(Mu, Var, y=y, qs=quantiles, crps=crps)
    out = {}
    if "pit" in got:
        out["pit"] = got["pit"]
    if "crps" in got:
        c, ok = got["crps"], torch.isfinite(y)
        out["crps"] = c
        out["mean_crps"] = torch.where(ok, c, torch.zeros_like(c)).sum() / ok.sum()
    if "spread" in got:
        out["crps_spread"] = got["spread"]
    if "quantiles" in got:
        out["quantiles"], out["unconverged"] = got["quantiles"], got["unconverged"]
    return out


def _mixture_coverage(Mq, qs, y):
    """1 where y lies inside the outermost pair of the exact quantiles Mq (len(qs), E), else 0, as float64."""
    lo, hi = Mq[int(np.argmin(qs))], Mq[int(np.argmax(qs))]
    return ((y >= lo) & (y <= hi)).to(F64)


def summarize_Y(model, X_list, Y_list=None, n_sample=1000, index=None, quantiles=(0.025, 0.975), noise_tape=None,
                keep_samples=False, mixture=False):
    """What the reference's drivers keep of NMGP.sample_Y on held-out rows (code/nmgp_dsvi.py:406-490;
    NMGP_ECoG_pred.py:277-299): mean, population sd and quantile bands of Y, mean and sd of the noise-free F, of
    row I_n of L and of G, mean and bands of tilde_ell -- and, when the observations Y_list are given, the scores:
    log predictive density lpd (N,) = log mean_s N(y_n | F_sn, sigma2_err + 1e-4) and its mean, RMSE of F_mean,
    coverage of the outermost requested Y band and the number of scored rows, per list entry (rows whose y is
    not finite are left out of every score and keep a NaN lpd).  A dict of device tensors.  Same setup, chunking,
    noise layout and stream as sample_Y; each chunk's tail is one fused call (csrc/ysum.hip) that reads only the
    I_n + 1 pairs of row n, so O(S N + N D) is stored and the (S, D, D, N) tensor of sample_Y is not.
    keep_samples=True adds Ys, Fs and tilde_ells, each (S, N).

    mixture=True adds the exact scores of the rows' predictives, the equal-weight mixtures of N(F_sn, s2) with
    s2 = sigma2_err + 1e-4 (score_mixture on Fs, one launch after the last chunk; the Y bands above are order
    statistics of one noisy draw per sample, these are the mixture's own): "mixture_quantiles" (len(quantiles), N),
    "crps_spread" (N,), "mixture_unconverged" (1,), and with Y_list "pit" and "crps" (N,), "mean_crps",
    "crps_per_entry" and "mixture_coverage" per list entry (the outermost pair of exact quantiles; NaN with fewer
    than two).  Every other key has the bits of the mixture=False run."""
    qs, n_sample = _check_sampling_args(quantiles, n_sample)
    D = model.D
    ids = list(range(len(X_list))) if index is None else [int(j) for j in index]
    if len(ids) != len(X_list):
        raise ValueError("index needs one output id per entry of X_list")
    if any(not 0 <= j < D for j in ids):
        raise ValueError(f"output ids must lie in 0..{D - 1}")
    xs = [torch.as_tensor(x).reshape(-1).to(F64) for x in X_list]
    sizes = [int(x.shape[0]) for x in xs]
    ys = None
    if Y_list is not None:
        ys = [torch.as_tensor(y).reshape(-1).to(F64) for y in Y_list]
        if len(ys) != len(xs) or any(y.shape[0] != n for y, n in zip(ys, sizes)):
            raise ValueError("Y_list must match X_list entry by entry")
    dev = model.device_
    x, I = prepare_inputs(model, xs, ids)
    st = _sampling_setup(model, x)
    N, M = st["N"], st["M"]
    per, o_p, _, o_f = _noise_layout(st, False)
    sd_err = (st["s2_err"] + JIT) ** 0.5
    z = lambda *shape: torch.zeros(*shape, dtype=F64, device=dev)
    Ts, Ys, Fs = (torch.empty(n_sample, N, dtype=F64, device=dev) for _ in range(3))
    F_sum, F_sq, L_sum, L_sq, G_sum, G_sq = z(N), z(N), z(N, D), z(N, D), z(D, N), z(D, N)
    y = lse_max = lse_sum = None
    if ys is not None:
        y = torch.cat(ys).to(dev)
        lse_max, lse_sum = torch.full((N,), float("-inf"), dtype=F64, device=dev), z(N)
    chunk = _chunk_size(n_sample, N, M)
    ws = H.y_workspace(D, N, chunk, dev)
    for done, S, zc in _chunks(_Draws(dev, noise_tape), n_sample, chunk, per):
        T, G, _, _ = _sample_TG(st, zc)
        Ts[done:done + S] = T
        H.y_accum_(st["pair_mu"], st["pair_sd"], G.contiguous(), zc[:, o_p:], zc[:, o_f:], I, sd_err,
                   Ys[done:done + S], Fs[done:done + S], F_sum, F_sq, L_sum, L_sq, G_sum, G_sq, y=y,
                   lse_max=lse_max, lse_sum=lse_sum, ws=ws)
    Y_mean, F_mean, L_mean, G_mean = Ys.mean(0), F_sum / n_sample, L_sum / n_sample, G_sum / n_sample
    Yq = _quantiles_dim0(Ys, qs)
    out = {"Y_mean": Y_mean, "Y_sd": _pop_sd((Ys * Ys).mean(0), Y_mean), "Y_quantiles": Yq,
           "F_mean": F_mean, "F_sd": _pop_sd(F_sq / n_sample, F_mean),
           "tilde_ell_mean": Ts.mean(0), "tilde_ell_quantiles": _quantiles_dim0(Ts, qs),
           "L_mean": L_mean, "L_sd": _pop_sd(L_sq / n_sample, L_mean),
           "G_mean": G_mean, "G_sd": _pop_sd(G_sq / n_sample, G_mean)}
    if y is not None:
        ok = torch.isfinite(y)
        lpd = _lpd(lse_max, lse_sum, ok, n_sample)

        def mean_of(v, mask):
            return torch.where(mask, v, torch.zeros_like(v)).sum() / mask.sum()          # 0 / 0 = NaN: none scored

        err2 = (F_mean - y) ** 2
        out["lpd"], out["mean_lpd"] = lpd, mean_of(lpd, ok)
        out["rmse_all"] = torch.sqrt(mean_of(err2, ok))
        bounds = np.cumsum([0] + sizes)
        parts = [slice(int(a), int(b)) for a, b in zip(bounds[:-1], bounds[1:])]
        out["rmse"] = torch.stack([torch.sqrt(mean_of(err2[p], ok[p])) for p in parts])
        out["n_scored"] = torch.stack([ok[p].sum() for p in parts])
        if len(qs) >= 2:
            lo, hi = Yq[int(np.argmin(qs))], Yq[int(np.argmax(qs))]
            inside = ((y >= lo) & (y <= hi)).to(F64)
            out["coverage"] = torch.stack([mean_of(inside[p], ok[p]) for p in parts])
    if mixture:
        mx = score_mixture(Fs, float(st["s2_err"] + JIT), y=y, quantiles=qs, crps=True)
        Mq = mx.get("quantiles", torch.empty(0, N, dtype=F64, device=dev))
        out["mixture_quantiles"], out["crps_spread"] = Mq, mx["crps_spread"]
        out["mixture_unconverged"] = mx.get("unconverged", torch.zeros(1, dtype=torch.int32, device=dev))
        if y is not None:
            out["pit"], out["crps"], out["mean_crps"] = mx["pit"], mx["crps"], mx["mean_crps"]
            out["crps_per_entry"] = torch.stack([mean_of(mx["crps"][p], ok[p]) for p in parts])
            inside = _mixture_coverage(Mq, qs, y) if len(qs) >= 2 else torch.full_like(y, float("nan"))
            out["mixture_coverage"] = torch.stack([mean_of(inside[p], ok[p]) for p in parts])
    if keep_samples:
        out["Ys"], out["Fs"], out["tilde_ells"] = Ys, Fs, Ts
    return out


def observed_grid(X_list, Y_list, x):
    """The bridge from the reference's per-output lists to the grid that impute_Y conditions on: Y_obs (N, D)
    float64 numpy, entry (n, d) the y of output d where X_list[d] contains x[n] exactly (the first hit wins), else
    NaN.  Host logic; X_list[d] need not be sorted and may hold duplicates."""
    if len(X_list) != len(Y_list):
        raise ValueError("Y_list must match X_list entry by entry")
    x = np.asarray(x, np.float64).reshape(-1)
    out = np.full((x.shape[0], len(X_list)), np.nan)
    for d, (xd, yd) in enumerate(zip(X_list, Y_list)):
        xd, yd = np.asarray(xd, np.float64).reshape(-1), np.asarray(yd, np.float64).reshape(-1)
        if xd.shape != yd.shape:
            raise ValueError("Y_list must match X_list entry by entry")
        if xd.size == 0:
            continue
        order = np.argsort(xd, kind="stable")                            # stable: the first of equal inputs first
        xs = xd[order]
        pos = np.minimum(np.searchsorted(xs, x, side="left"), xs.size - 1)
        hit = xs[pos] == x
        out[hit, d] = yd[order[pos[hit]]]
    return out


def _impute_args(D, Y_obs, Y_true, n_sample, quantiles, N=None):
    """Validation of impute_Y that needs no device -> (Y_obs, Y_true as float64 numpy, n_sample, quantiles)."""
    qs, n_sample = _check_sampling_args(quantiles, n_sample)
    Y_obs = np.asarray(Y_obs.detach().cpu() if torch.is_tensor(Y_obs) else Y_obs, np.float64)
    if Y_obs.ndim != 2 or Y_obs.shape[1] != D or (N is not None and Y_obs.shape[0] != N):
        raise ValueError(f"Y_obs must be (N, D) = ({'N' if N is None else N}, {D}), got {Y_obs.shape}")
    if Y_true is not None:
        Y_true = np.asarray(Y_true.detach().cpu() if torch.is_tensor(Y_true) else Y_true, np.float64)
        if Y_true.shape != Y_obs.shape:
            raise ValueError(f"Y_true must have the shape of Y_obs {Y_obs.shape}, got {Y_true.shape}")
    return Y_obs, Y_true, n_sample, qs


def impute_Y(model, x, Y_obs, Y_true=None, n_sample=1000, quantiles=(0.025, 0.975), noise_tape=None,
             keep_samples=False, mixture=False):
    """Predict the missing outputs at the inputs x (N,) from the outputs observed at the SAME inputs: Y_obs (N, D)
    holds the observations, NaN where an output is missing (observed_grid builds it from per-output lists).  This
    is what makes the model collaborative at prediction time: the outputs share the latent g through L(x), so an
    output observed at x_n informs the others there.  Per posterior sample s (tilde_ell, L and the MGP_d marginals
    mu_g, var_g of the latent, drawn exactly as sample_FY draws them: same setup, chunking, noise layout
    [z_v M][z_t N][z_p Q N][z_g D N][z_f N D] and stream, so the same seed or tape gives the same tilde_ell and L
    samples) the latent G is integrated out, y(x_n) ~ N(L mu_g, L V L^T + s2 I) with V = diag(var_g + 1e-4) and
    s2 = sigma2_err + 1e-4 (z_g is consumed, not used), and every missing entry gets its conditional mean mu_s and
    variance v_s given the row's observed entries.  The predictive of an entry is the equal-weight mixture of
    N(mu_s, v_s) over the samples.  Each chunk is one fused launch (csrc/ycond.hip) that never stores an
    (S, N, D, D) tensor.

    Returns a dict of device tensors over the E missing entries in (n, d) row-major order: "missing" (E, 2) their
    (n, d); "mean" and "sd" (mixture mean and population sd of y); "F_mean" and "F_sd" (noise-free: v_s - s2);
    "Y_filled" (N, D), Y_obs with the means written into the gaps; "tilde_ell_mean" (N,); with non-empty quantiles
    "quantiles" (len(quantiles), E), the sample quantiles of the draws mu_s + sqrt(v_s) z_f with z_f the entry's
    noise of the sample_FY slot (one draw per sample, not the exact mixture quantile: mixture=True gives that).
    mu_s and v_s are collected as (S, E) only when quantiles, keep_samples or mixture ask for them: 16 S E bytes,
    not batched.  keep_samples=True adds "Mu", "Var" (S, E) and "tilde_ells" (S, N).

    mixture=True scores the collected mixtures exactly, once after the last chunk (score_mixture, csrc/mixscore.hip):
    "mixture_quantiles" (len(quantiles), E), the roots of the mixture CDF, "crps_spread" (E,), the CRPS term that
    needs no truth, and "mixture_unconverged" (1,); every other key keeps the bits of the mixture=False run.

    With Y_true (N, D) the missing entries whose truth is finite are scored: "lpd" (E,) the log of the mixture
    density at the truth (NaN where not scored) and "mean_lpd"; "rmse" (D,) per output and "rmse_all", of "mean";
    "coverage" (D,) of the outermost quantile band (needs two quantiles); "n_scored" (D,).  With mixture=True also
    "pit" (E,), the mixture CDF at the truth, "crps" (E,) and "mean_crps", "crps_per_output" (D,) and
    "mixture_coverage" (D,) of the outermost pair of exact quantiles (NaN with fewer than two).

    A row with no missing entry costs nothing; with no missing entry at all every result has E = 0.  An all-NaN
    Y_obs conditions on nothing: the result is the unconditional predictive of sample_FY's Y, Rao-Blackwellised
    over G and the observation noise.

    What this is not: the conditioning is pointwise in x -- an observed output informs the others at the same
    input only, not at neighbouring inputs.  And observations that were already in the training set are used
    twice, once through the variational posterior and once here; the clean protocol holds the test inputs out of
    training for every output."""
    Y_obs, Y_true, n_sample, qs = _impute_args(model.D, Y_obs, Y_true, n_sample, quantiles)
    dev = model.device_
    x = torch.as_tensor(x).reshape(-1, 1).to(F64).to(dev).contiguous()
    if Y_obs.shape[0] != x.shape[0]:
        raise ValueError(f"Y_obs must be (N, D) = ({x.shape[0]}, {model.D}), got {Y_obs.shape}")
    st = _sampling_setup(model, x)
    N, D, M = st["N"], st["D"], st["M"]
    per = _noise_layout(st, True)[0]
    s2 = st["s2_err"] + JIT
    Yo = torch.from_numpy(np.ascontiguousarray(Y_obs)).to(dev)
    e_off, missing = H.missing_table(Yo)
    E = int(missing.shape[0])
    flat = missing[:, 0] * D + missing[:, 1]
    z = lambda *shape: torch.zeros(*shape, dtype=F64, device=dev)
    mu_sum, y2_sum, f2_sum, T_sum = z(E), z(E), z(E), z(N)
    collect = bool(qs) or keep_samples or mixture
    Mu = Var = Yd = None
    if collect:
        Mu, Var = torch.empty(n_sample, E, dtype=F64, device=dev), torch.empty(n_sample, E, dtype=F64, device=dev)
    if qs:
        Yd = torch.empty(n_sample, E, dtype=F64, device=dev)
    Ts = torch.empty(n_sample, N, dtype=F64, device=dev) if keep_samples else None
    y = lse_max = lse_sum = None
    if Y_true is not None:
        y = torch.from_numpy(np.ascontiguousarray(Y_true)).to(dev).reshape(-1)[flat].contiguous()
        lse_max, lse_sum = torch.full((E,), float("-inf"), dtype=F64, device=dev), z(E)
    chunk = _chunk_size(n_sample, N, M)
    ws = H.ycond_workspace(D, N, chunk, dev) if E > 0 else None
    for done, S, zc in _chunks(_Draws(dev, noise_tape), n_sample, chunk, per):
        T, mu_g, var_g, o_p, o_g, o_f = _sample_T_moments(st, zc)
        T_sum += T.sum(0)
        if Ts is not None:
            Ts[done:done + S] = T
        if E > 0:
            H.ycond_accum_(st["pair_mu"], st["pair_sd"], zc[:, o_p:], mu_g.contiguous(),
                           var_g.transpose(1, 2).contiguous(), Yo, s2, e_off, mu_sum, y2_sum, f2_sum, y_true=y,
                           lse_max=lse_max, lse_sum=lse_sum, Mu=Mu, Var=Var, s_off=done, ws=ws)
            if qs:
                z_f = zc[:, o_f:].index_select(1, flat)
                Yd[done:done + S] = Mu[done:done + S] + torch.sqrt(Var[done:done + S]) * z_f
    mean = mu_sum / n_sample
    filled = Yo.clone()
    filled.reshape(-1)[flat] = mean
    out = {"missing": missing, "mean": mean, "sd": _pop_sd(y2_sum / n_sample, mean),
           "F_mean": mean.clone(), "F_sd": _pop_sd(f2_sum / n_sample, mean), "Y_filled": filled,
           "tilde_ell_mean": T_sum / n_sample}
    Yq = None
    if qs:
        Yq = _quantiles_dim0(Yd, qs)
        out["quantiles"] = Yq
    if y is not None:
        ok = torch.isfinite(y)
        lpd = _lpd(lse_max, lse_sum, ok, n_sample)
        okf = ok.to(F64)
        d_of = missing[:, 1]

        def per_output(v):                                               # sum over the scored entries of each output
            return z(D).index_add_(0, d_of, torch.where(ok, v, torch.zeros_like(v)))

        n_sc = per_output(okf)                                           # 0 / 0 = NaN: none scored
        err2 = (mean - y) ** 2
        out["lpd"] = lpd
        out["mean_lpd"] = torch.where(ok, lpd, torch.zeros_like(lpd)).sum() / okf.sum()
        out["rmse"] = torch.sqrt(per_output(err2) / n_sc)
        out["rmse_all"] = torch.sqrt(per_output(err2).sum() / okf.sum())
        out["n_scored"] = n_sc.to(torch.long)
        if len(qs) >= 2:
            lo, hi = Yq[int(np.argmin(qs))], Yq[int(np.argmax(qs))]
            out["coverage"] = per_output(((y >= lo) & (y <= hi)).to(F64)) / n_sc
    if mixture:
        mx = score_mixture(Mu, Var, y=y, quantiles=qs, crps=True)
        Mq = mx.get("quantiles", torch.empty(0, E, dtype=F64, device=dev))
        out["mixture_quantiles"], out["crps_spread"] = Mq, mx["crps_spread"]
        out["mixture_unconverged"] = mx.get("unconverged", torch.zeros(1, dtype=torch.int32, device=dev))
        if y is not None:
            out["pit"], out["crps"], out["mean_crps"] = mx["pit"], mx["crps"], mx["mean_crps"]
            out["crps_per_output"] = per_output(mx["crps"]) / n_sc
            inside = _mixture_coverage(Mq, qs, y) if len(qs) >= 2 else torch.full_like(y, float("nan"))
            out["mixture_coverage"] = per_output(inside) / n_sc
    if keep_samples:
        out["Mu"], out["Var"], out["tilde_ells"] = Mu, Var, Ts
    return out
