"""One chunk of the conditional prediction of missing outputs, timed with HIP events after warm-up: the fused launch
of predict.impute_Y (csrc/ycond.hip) against the materialised route at the same shapes -- the pair loop of
sample_FY -> L (S, N, D, D), the dense A = V^-1 + L^T diag(w) L and b through torch, torch.linalg.cholesky and two
triangular solves (every row of L as a right-hand side, then the missing entries gathered).

  python tools/impute_probe.py [--fused-only] [--out profiles/impute_probe.json]

Shapes (D, N, S) = (50, 64, 256) and (128, 64, 64), each with one missing output per row and with half of every
row missing.  The off-diagonal pair rows are scaled by 1 / sqrt(D) so that L is well conditioned
(tests/_pcorr_ref.py); the kernel's time does not depend on the values.  The peak memory of each route is the
growth of torch's peak allocation over the inputs both share.  No speed is fixed in advance."""
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import provenance  # noqa: E402
from collaborative_nonstationary_multivariate_gaussian_process_amd import hip_ops as H  # noqa: E402

F64 = torch.float64
SHAPES = [(50, 64, 256), (128, 64, 64)]
S2 = math.exp(-5.0) + 1e-4
dev = torch.device("cuda", 0)


def timed(fn, min_ms=300.0, max_reps=50):
    """ms per call: one warm-up call, one call to size the window, then at least 3 calls and about min_ms of work."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    reps = int(min(max_reps, max(3, math.ceil(min_ms / max(e0.elapsed_time(e1), 1e-3)))))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, reps


def peak_of(fn):
    """Growth of the peak allocation over what is allocated now, in MB."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    del out
    return round(grown / 1e6, 1)


def main():
    fused_only = "--fused-only" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
        ROOT, "profiles", "impute_probe.json")
    rows = []
    for D, N, S in SHAPES:
        Q = D * (D + 1) // 2
        g = torch.Generator(device=dev).manual_seed(D)
        pairs = [(i, j) for i in range(D) for j in range(i + 1)]
        scale = torch.tensor([1.0 if i == j else D ** -0.5 for i, j in pairs], dtype=F64, device=dev).reshape(Q, 1)
        pair_mu = 0.5 * torch.randn(Q, N, dtype=F64, device=dev, generator=g) * scale
        pair_sd = (0.05 + 0.45 * torch.rand(Q, N, dtype=F64, device=dev, generator=g)) * scale
        zc = torch.randn(S, Q * N, dtype=F64, device=dev, generator=g)
        mu_g = torch.randn(S, N, D, dtype=F64, device=dev, generator=g)
        var_g = 0.01 + 0.99 * torch.rand(S, N, D, dtype=F64, device=dev, generator=g)
        Y = torch.randn(N, D, dtype=F64, device=dev, generator=g)
        for mask in ("one_missing", "half_missing"):
            miss = torch.zeros(N, D, dtype=torch.bool, device=dev)
            if mask == "one_missing":
                miss[torch.arange(N, device=dev), torch.randint(0, D, (N,), device=dev, generator=g)] = True
            else:
                order = torch.rand(N, D, device=dev, generator=g).argsort(1)
                miss.scatter_(1, order[:, :D // 2], True)
            Y_obs = torch.where(miss, torch.full_like(Y, float("nan")), Y)
            e_off, missing = H.missing_table(Y_obs)
            E = int(missing.shape[0])
            ws = H.ycond_workspace(D, N, S, dev)
            sums = [torch.zeros(E, dtype=F64, device=dev) for _ in range(3)]
            Mu, Var = torch.empty(S, E, dtype=F64, device=dev), torch.empty(S, E, dtype=F64, device=dev)

            def fused():
                for t in sums:
                    t.zero_()
                H.ycond_accum_(pair_mu, pair_sd, zc, mu_g, var_g, Y_obs, S2, e_off, *sums, Mu=Mu, Var=Var, ws=ws)
                return Mu

            def materialised():
                Ls = pair_mu.unsqueeze(0) + pair_sd.unsqueeze(0) * zc.reshape(S, Q, N)
                Lfull = torch.zeros(S, D, D, N, dtype=F64, device=dev)
                for q, (i, j) in enumerate(pairs):
                    Lfull[:, i, j] = torch.exp(Ls[:, q]) if i == j else Ls[:, q]
                Ln = Lfull.permute(0, 3, 1, 2).contiguous()                              # (S, N, D, D)
                del Lfull, Ls
                w = (~miss).to(F64) / S2                                                 # (N, D)
                A = torch.matmul(Ln.transpose(2, 3) * w.unsqueeze(0).unsqueeze(2), Ln)
                vinv = 1.0 / (var_g + 1e-4)
                A.diagonal(dim1=-2, dim2=-1).add_(vinv)
                wy = torch.where(miss, torch.zeros_like(Y), Y) * w
                b = vinv * mu_g + torch.matmul(Ln.transpose(2, 3), wy.unsqueeze(0).unsqueeze(3))[..., 0]
                R = torch.linalg.cholesky(A)
                del A
                c = torch.linalg.solve_triangular(R, b.unsqueeze(3), upper=False)[..., 0]
                W = torch.linalg.solve_triangular(R, Ln.transpose(2, 3), upper=False)     # column h = R^-1 l_h
                mu = torch.einsum("snjh,snj->snh", W, c)[:, miss]
                v = (W * W).sum(2)[:, miss] + S2
                return mu, v

            row = {"D": D, "N": N, "S": S, "mask": mask, "E": E, "sliced": ws is not None,
                   "samples_tensor_MB": round(S * N * D * D * 8 / 1e6, 1), "collected_MB": round(2 * S * E * 8 / 1e6, 1)}
            ms, reps = timed(fused)
            row["fused_ms"], row["fused_reps"] = round(ms, 3), reps
            row["fused_us_per_sample_input"] = round(ms * 1e3 / (S * N), 3)
            row["fused_peak_MB"] = peak_of(fused)
            if not fused_only:
                mu, v = materialised()
                fused()
                torch.cuda.synchronize()
                row["max_abs_mu_diff"] = float((Mu - mu).abs().max())
                row["max_abs_v_diff"] = float((Var - v).abs().max())
                del mu, v
                ms, reps = timed(materialised, max_reps=5)
                row["materialised_ms"], row["materialised_reps"] = round(ms, 3), reps
                row["materialised_peak_MB"] = peak_of(materialised)
                row["materialised_over_fused"] = round(ms / row["fused_ms"], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del pair_mu, pair_sd, zc, mu_g, var_g
        torch.cuda.empty_cache()
    if not fused_only:
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        json.dump({"device": torch.cuda.get_device_name(0), "code_hash": provenance.code_hash(),
                   "timing": "HIP events; 1 warm-up call, 1 sizing call, then the mean of max(3, 300 ms of) calls "
                             "(at most 50; at most 5 on the materialised side)",
                   "peak": "growth of torch's peak allocation during one call over the shared inputs",
                   "rows": rows}, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
