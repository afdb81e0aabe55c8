"""One chunk of partial correlations, timed with HIP events after warm-up: the fused kernel of
predict.summarize_FY(partial=True) (csrc/pcorr.hip) alone, with and without the collection of every pair, against the
materialised route -- sample_FY's tail (pair loop -> Lfull (S, D, D, N), cov, corr (S, N, D, D)) followed by
torch.linalg.inv, the normalisation and the mean / second moment over the samples.

  python tools/pcorr_probe.py [--fused-only] [--out profiles/pcorr_probe.json]

Shapes: D in {50, 128} x N in {64, 1000}; S is one chunk of predict._chunk_size at n_sample = 1000 with M = 512
(D = 50) or 1024 (D = 128), which only sets how many samples a chunk holds.  The off-diagonal pair rows are scaled
by 1 / sqrt(D) so that L is well conditioned (tests/_pcorr_ref.py); the kernel's time does not depend on the values.
GF/s counts 2 D^3 / 3 fp64 flops per (sample, input) -- the flops of the triangular inverse and of the lower
triangle of W^T W that the algorithm needs, not the padded-tile MFMA rate.  No speed is fixed in advance."""
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from collaborative_nonstationary_multivariate_gaussian_process_amd import hip_ops as H  # noqa: E402
from collaborative_nonstationary_multivariate_gaussian_process_amd import predict  # noqa: E402

F64 = torch.float64
SHAPES = [(50, 64, 512), (50, 1000, 512), (128, 64, 1024), (128, 1000, 1024)]
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


def main():
    fused_only = "--fused-only" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
        ROOT, "profiles", "pcorr_probe.json")
    rows = []
    for D, N, M in SHAPES:
        S = predict._chunk_size(1000, N, M)
        Q = D * (D + 1) // 2
        g = torch.Generator(device=dev).manual_seed(D)
        pairs = [(i, j) for i in range(D) for j in range(i + 1)]
        scale = torch.tensor([1.0 if i == j else D ** -0.5 for i, j in pairs], dtype=F64, device=dev).reshape(Q, 1)
        pair_mu = 0.5 * torch.randn(Q, N, dtype=F64, device=dev, generator=g) * scale
        pair_sd = (0.05 + 0.45 * torch.rand(Q, N, dtype=F64, device=dev, generator=g)) * scale
        zc = torch.randn(S, Q * N, dtype=F64, device=dev, generator=g)
        psum = torch.zeros(N, D, D, dtype=F64, device=dev)
        psq = torch.zeros(N, D, D, dtype=F64, device=dev)
        pij = torch.tensor([(i, j) for i in range(D) for j in range(i)], dtype=torch.int32, device=dev)
        pi, pj = pij[:, 0].contiguous(), pij[:, 1].contiguous()
        C = torch.empty(pi.numel(), N, S, dtype=F64, device=dev)
        ws = H.pcorr_workspace(D, N, S, dev)

        def sums():
            psum.zero_(), psq.zero_()
            H.pcorr_accum_(pair_mu, pair_sd, zc, psum, psq, ws=ws)

        def sums_and_all_pairs():
            psum.zero_(), psq.zero_()
            H.pcorr_accum_(pair_mu, pair_sd, zc, psum, psq, pi, pj, C, ws=ws)

        def collect_only():
            H.pcorr_accum_(pair_mu, pair_sd, zc, pi=pi, pj=pj, C=C)

        def materialised():
            Ls = pair_mu.unsqueeze(0) + pair_sd.unsqueeze(0) * zc.reshape(S, Q, N)
            Lfull = torch.zeros(S, D, D, N, dtype=F64, device=dev)
            for q, (i, j) in enumerate(pairs):
                Lfull[:, i, j] = torch.exp(Ls[:, q]) if i == j else Ls[:, q]
            Ln = Lfull.permute(0, 3, 1, 2)
            cov = torch.matmul(Ln, Ln.transpose(2, 3))
            invstd = torch.sqrt(torch.diag_embed(1.0 / torch.diagonal(cov, dim1=-2, dim2=-1)))
            corr = torch.matmul(torch.matmul(invstd, cov), invstd)
            del cov, invstd, Lfull, Ln, Ls
            Om = torch.linalg.inv(corr)
            isd = torch.sqrt(1.0 / torch.diagonal(Om, dim1=-2, dim2=-1))
            pc = -Om * isd.unsqueeze(-1) * isd.unsqueeze(-2)
            idx = torch.arange(D, device=dev)
            pc[..., idx, idx] = 1.0
            return pc.mean(0), (pc * pc).mean(0)

        flops = 2.0 * D ** 3 / 3.0 * S * N
        row = {"D": D, "N": N, "M": M, "S_chunk": S, "noise_block_MB": round(zc.numel() * 8 / 1e6, 1),
               "pcorr_samples_MB": round(S * N * D * D * 8 / 1e6, 1), "all_pairs": int(pi.numel()),
               "C_MB": round(C.numel() * 8 / 1e6, 1), "sliced": ws is not None}
        for name, fn in (("sums", sums), ("sums_and_all_pairs", sums_and_all_pairs), ("collect_only", collect_only)):
            ms, reps = timed(fn)
            row[name + "_ms"], row[name + "_reps"] = round(ms, 3), reps
            row[name + "_fp64_GFLOPs"] = round(flops / ms / 1e6, 1)
        row["us_per_sample_input"] = round(row["sums_ms"] * 1e3 / (S * N), 3)
        if not fused_only:
            torch.cuda.reset_peak_memory_stats()
            try:
                pm, pq2 = materialised()
                sums()
                torch.cuda.synchronize()
                row["max_abs_pcorr_mean_diff"] = float((psum / S - pm).abs().max())
                row["max_abs_pcorr_sq_diff"] = float((psq / S - pq2).abs().max())
                del pm, pq2
                ms, reps = timed(materialised, max_reps=3)
                row["materialised_ms"], row["materialised_reps"] = round(ms, 3), reps
                row["materialised_over_fused"] = round(ms / row["sums_ms"], 2)
            except torch.OutOfMemoryError as e:
                row["materialised_ms"] = None
                row["materialised_skipped"] = "did not fit: " + str(e)[:120]
            row["materialised_peak_MB"] = round(torch.cuda.max_memory_allocated() / 1e6, 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del pair_mu, pair_sd, zc, psum, psq, C, ws
        torch.cuda.empty_cache()
    if not fused_only:
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        json.dump({"device": torch.cuda.get_device_name(0),
                   "timing": "HIP events; 1 warm-up call, 1 sizing call, then the mean of max(3, 300 ms of) calls "
                             "(at most 50; at most 3 on the materialised side)",
                   "flops": "2 D^3 / 3 per (sample, input)", "rows": rows}, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
