"""One chunk of correlation spectra, timed with HIP events after warm-up: the fused kernel of
predict.summarize_FY(spectrum=...) (csrc/spectrum.hip) for k = 4 with loadings and for k = D, next to fy_accum_
(csrc/fy.hip) on the same inputs in the same process, and next to the route a user has without the kernel: the
chunk's correlation samples materialised as predict.sample_FY does, then torch.linalg.eigvalsh.

  python tools/spectrum_probe.py [--out profiles/spectrum_probe.json]

Shapes: HCP (D = 50, M = 512) and ECoG (D = 128, M = 1024), N = 800; S is one chunk of predict._chunk_size at
n_sample = 1000.  The materialised route runs on the first samples of the chunk only -- as many as hold the
(S', N, D, D) tensor under 2 GB and, for eigvalsh, as an estimate from a first call on 64 matrices puts under a few
seconds -- and is scaled linearly to the chunk; the JSON records the matrices it ran and the factor.  The fused
kernel's eigenvalues are compared with eigvalsh of the materialised matrices on those samples (largest difference
recorded), and its counter of unconverged solves is recorded.  No speed is fixed in advance: the kernel exists for
the memory, a chunk's time is recorded as it is."""
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from provenance import code_hash  # noqa: E402
from collaborative_nonstationary_multivariate_gaussian_process_amd import hip_ops as H  # noqa: E402
from collaborative_nonstationary_multivariate_gaussian_process_amd import predict  # noqa: E402

F64 = torch.float64
SHAPES = [("hcp", 50, 800, 512), ("ecog", 128, 800, 1024)]
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


def corr_samples(pair_mu, pair_sd, z_p, D):
    """The materialised correlations of predict.sample_FY for the samples of z_p (S', Q N) -> (S', N, D, D)."""
    Sx, N = z_p.shape[0], pair_mu.shape[1]
    Q = D * (D + 1) // 2
    l = pair_mu.unsqueeze(0) + pair_sd.unsqueeze(0) * z_p[:, :Q * N].reshape(Sx, Q, N)
    i, j = torch.tril_indices(D, D, device=dev)
    Ln = torch.zeros(Sx, N, D, D, dtype=F64, device=dev)
    Ln[:, :, i, j] = torch.where((i == j)[None, :, None], torch.exp(l), l).transpose(1, 2)
    cov = torch.matmul(Ln, Ln.transpose(2, 3))
    invstd = torch.sqrt(torch.diag_embed(1.0 / torch.diagonal(cov, dim1=-2, dim2=-1)))
    return torch.matmul(torch.matmul(invstd, cov), invstd)


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
        ROOT, "profiles", "spectrum_probe.json")
    rows = []
    for name, D, N, M in SHAPES:
        S = predict._chunk_size(1000, N, M)
        Q = D * (D + 1) // 2
        g = torch.Generator(device=dev).manual_seed(D)
        pair_mu = 0.5 * torch.randn(Q, N, dtype=F64, device=dev, generator=g)
        pair_sd = 0.05 + 0.45 * torch.rand(Q, N, dtype=F64, device=dev, generator=g)
        zc = torch.randn(S, Q * N + N * D, dtype=F64, device=dev, generator=g)
        Gm = torch.randn(S, D, N, dtype=F64, device=dev, generator=g)
        Y = torch.empty(S, N, D, dtype=F64, device=dev)
        csum = torch.zeros(N, D, D, dtype=F64, device=dev)
        csq = torch.zeros(N, D, D, dtype=F64, device=dev)
        ws = H.fy_workspace(D, N, S, dev)

        def fy():
            H.fy_accum_(pair_mu, pair_sd, Gm, zc, zc[:, Q * N:], 0.1, Y, csum, csq, ws=ws)

        row = {"shape": name, "D": D, "N": N, "M": M, "S_chunk": S, "matrices": S * N,
               "corr_samples_chunk_MB": round(S * N * D * D * 8 / 1e6, 1),
               "corr_samples_n_sample_1000_GB": round(1000 * N * D * D * 8 / 1e9, 1)}
        ms, reps = timed(fy)
        row["fy_accum_ms"], row["fy_accum_reps"] = round(ms, 3), reps
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        E_all = None
        for label, k, load in (("top4_loadings", 4, True), ("all_no_loadings", D, False), ("all_loadings", D, True)):
            E = torch.empty(k + 1, N, S, dtype=F64, device=dev)
            l2 = torch.zeros(N, k, D, dtype=F64, device=dev) if load else None
            sws = H.spectrum_workspace(D, N, S, k, dev) if load else None
            ms, reps = timed(lambda: H.corr_spectrum_(pair_mu, pair_sd, zc, k, E, cnt, load2_sum=l2, ws=sws),
                             max_reps=10)
            row[label] = {"k": k, "ms": round(ms, 3), "reps": reps, "us_per_matrix_per_cu":
                          round(ms * 1e3 / math.ceil(S * N / 256), 2), "over_fy_accum": round(ms / row["fy_accum_ms"], 1),
                          "E_MB": round(E.numel() * 8 / 1e6, 1)}
            if k == D and E_all is None:
                E_all = E
        row["unconverged"] = int(cnt.item())
        # ---- the materialised route on the first samples of the chunk
        s_fit = max(1, min(S, int(2e9 // (N * D * D * 8))))
        corr_ms, _ = timed(lambda: corr_samples(pair_mu, pair_sd, zc[:s_fit], D), max_reps=5)
        cs = corr_samples(pair_mu, pair_sd, zc[:s_fit], D)
        small = cs.reshape(-1, D, D)[:64]
        ms64, _ = timed(lambda: torch.linalg.eigvalsh(small), min_ms=0.0, max_reps=3)
        n_eig = int(max(64, min(s_fit * N, 5000.0 / max(ms64 / 64, 1e-6))))
        mats = cs.reshape(-1, D, D)[:n_eig]                                                    # (s, n) order
        eig_ms, eig_reps = timed(lambda: torch.linalg.eigvalsh(mats), min_ms=0.0, max_reps=3)
        lam = torch.linalg.eigvalsh(mats).flip(-1)                                             # descending
        n_m = mats.shape[0]
        got = E_all[:D].permute(2, 1, 0).reshape(-1, D)[:n_m]                                  # (s, n) order
        row["materialised"] = {
            "corr_samples": {"samples": s_fit, "ms": round(corr_ms, 3),
                             "scaled_to_chunk_ms": round(corr_ms * S / s_fit, 1)},
            "eigvalsh": {"matrices": n_m, "first_call_64_matrices_ms": round(ms64, 3), "ms": round(eig_ms, 3),
                         "reps": eig_reps, "scale": round(S * N / n_m, 2),
                         "scaled_to_chunk_ms": round(eig_ms * S * N / n_m, 1)},
            "max_abs_diff_fused_vs_eigvalsh": float((got - lam).abs().max())}
        total = row["materialised"]["corr_samples"]["scaled_to_chunk_ms"] + \
            row["materialised"]["eigvalsh"]["scaled_to_chunk_ms"]
        row["materialised"]["scaled_to_chunk_ms"] = round(total, 1)
        row["fused_all_over_materialised"] = round(row["all_no_loadings"]["ms"] / total, 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del pair_mu, pair_sd, zc, Gm, Y, csum, csq, ws, cs, mats, small, lam, E_all
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump({"code_hash": code_hash(), "device": torch.cuda.get_device_name(0),
               "timing": "HIP events; 1 warm-up call, 1 sizing call, then the mean of max(3, 300 ms of) calls (at "
                         "most 10 for the spectrum kernel, 3 for eigvalsh); all in the same process on the same "
                         "inputs; the materialised route on a part of the chunk, scaled linearly",
               "rows": rows}, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
