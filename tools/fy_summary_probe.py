"""One chunk's sample_FY tail, timed with HIP events after warm-up: the materialised path of predict.sample_FY
(pair loop -> Lfull (S, D, D, N), three batched matmuls -> corrs (S, N, D, D), then the mean over samples the
drivers take) against the fused kernel of predict.summarize_FY (csrc/fy.hip).

  python tools/fy_summary_probe.py [--fused-only] [--out profiles/fy_summary_probe.json]

Shapes (D, N, M, S_chunk): (50, 1000, 512, 64) and (128, 1000, 1024, 32); M only sets how many samples a chunk
holds (predict._chunk_size gives 65 and 32 at n_sample = 1000) -- the tail does not read it.  --fused-only
skips the materialised side (for a counter pass: rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES GRBM_GUI_ACTIVE, summarised by tools/mfma_summary.py).
The yardstick is the materialised tail at the same shape; no speed is fixed in advance."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from collaborative_nonstationary_multivariate_gaussian_process_amd import hip_ops as H  # noqa: E402

F64 = torch.float64
SHAPES = [(50, 1000, 512, 64), (128, 1000, 1024, 32)]
dev = torch.device("cuda", 0)


def timed(fn, reps):
    """ms per call.  The fused side's timed region includes zeroing corr_sum / corr_sq (two memsets of N D D
    doubles, as summarize_FY does once per call); the materialised side's includes its allocations."""
    fn()                                                  # warm-up: code objects, allocator pool, library heuristics
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def mfma_count(D):
    """v_mfma_f64_16x16x4_f64 per (sample, input): cov tile (ti, tj <= ti) sums tj + 1 k-tiles of 4 steps."""
    nt = (D + 15) // 16
    return 4 * sum((tj + 1) for ti in range(nt) for tj in range(ti + 1))


def main():
    fused_only = "--fused-only" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
        ROOT, "profiles", "fy_summary_probe.json")
    rows = []
    for D, N, M, S in SHAPES:
        Q = D * (D + 1) // 2
        per = Q * N + N * D
        g = torch.Generator(device=dev).manual_seed(D)
        pair_mu = 0.5 * torch.randn(Q, N, dtype=F64, device=dev, generator=g)
        pair_sd = 0.05 + 0.45 * torch.rand(Q, N, dtype=F64, device=dev, generator=g)
        G = torch.randn(S, D, N, dtype=F64, device=dev, generator=g)
        zc = torch.randn(S, per, dtype=F64, device=dev, generator=g)
        sd_err = 0.3
        pairs = [(i, j) for i in range(D) for j in range(i + 1)]
        Y = torch.empty(S, N, D, dtype=F64, device=dev)
        csum = torch.zeros(N, D, D, dtype=F64, device=dev)
        csq = torch.zeros(N, D, D, dtype=F64, device=dev)

        def fused():
            csum.zero_(), csq.zero_()
            H.fy_accum_(pair_mu, pair_sd, G, zc, zc[:, Q * N:], sd_err, Y, csum, csq)

        def materialised():
            z_p = zc[:, :Q * N].reshape(S, Q, N)
            z_f = zc[:, Q * N:].reshape(S, N, D)
            Ls = pair_mu.unsqueeze(0) + pair_sd.unsqueeze(0) * z_p
            Lfull = torch.zeros(S, D, D, N, dtype=F64, device=dev)
            for q, (i, j) in enumerate(pairs):
                Lfull[:, i, j] = torch.exp(Ls[:, q]) if i == j else Ls[:, q]
            Ln = Lfull.permute(0, 3, 1, 2)
            F = torch.matmul(Ln, G.transpose(1, 2).unsqueeze(3))[..., 0]
            cov = torch.matmul(Ln, Ln.transpose(2, 3))
            invstd = torch.sqrt(torch.diag_embed(1.0 / torch.diagonal(cov, dim1=-2, dim2=-1)))
            corr = torch.matmul(torch.matmul(invstd, cov), invstd)
            return F + sd_err * z_f, corr.mean(0)

        row = {"D": D, "N": N, "M": M, "S_chunk": S, "noise_block_MB": round(zc.numel() * 8 / 1e6, 1),
               "corr_samples_MB": round(S * N * D * D * 8 / 1e6, 1)}
        ms = timed(fused, 5)
        n_mfma = mfma_count(D) * S * N
        row["fused_ms"] = round(ms, 3)
        row["fused_read_GBs"] = round((zc.numel() + G.numel() + 2 * Q * N) * 8 / ms / 1e6, 1)
        row["fused_cov_mfma_GFLOPs"] = round(n_mfma * 2 * 16 * 16 * 4 / ms / 1e6, 1)      # padded-tile rate
        if not fused_only:
            try:
                Ym, cm = materialised()
                fused()
                torch.cuda.synchronize()
                row["max_abs_corr_mean_diff"] = float((csum / S - cm).abs().max())
                row["max_abs_Y_diff"] = float((Y - Ym).abs().max())
                del Ym, cm
                row["materialised_ms"] = round(timed(materialised, 2), 3)
                row["materialised_over_fused"] = round(row["materialised_ms"] / row["fused_ms"], 2)
            except torch.OutOfMemoryError as e:
                row["materialised_ms"] = None
                row["materialised_skipped"] = "did not fit: " + str(e)[:120]
            row["materialised_peak_MB"] = round(torch.cuda.max_memory_allocated() / 1e6, 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del pair_mu, pair_sd, G, zc, Y, csum, csq
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
    if not fused_only:
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        json.dump({"device": torch.cuda.get_device_name(0), "timing": "HIP events, 1 warm-up call, mean of 5 (fused) / "
                   "2 (materialised) calls", "rows": rows}, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
