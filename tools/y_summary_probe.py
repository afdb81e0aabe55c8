"""One chunk's sample_Y tail, timed with HIP events after warm-up: the materialised path of predict.sample_Y
(_sample_chunk's loop over the Q pairs into Lfull (S, D, D, N), then the gather of row I_n, F, Y and the means over
the samples that callers take) against the fused call of predict.summarize_Y (csrc/ysum.hip), with observations.

  python tools/y_summary_probe.py [--fused-only] [--out profiles/y_summary_probe.json]

Shapes (D, N, M, S_chunk): (50, 1000, 512, 64) and (128, 1000, 1024, 32); M only sets how many samples a chunk
holds (predict._chunk_size gives 65 and 32 at n_sample = 1000) -- the tail does not read it.  The ids are D equal
blocks of inputs, as the list-per-output API builds them.  The two sides are timed alternately, three rounds each;
the yardstick is the materialised tail at the same shape; no speed is fixed in advance.  fused_ms is what a chunk of
summarize_Y pays (allocations, zeroing, the call); fused_call_ms is the call alone on buffers made before, which on
an idle stream is still bound by the host's launches -- the kernels' own time comes from a separate pass,
rocprofv3 --kernel-trace --stats -- python tools/y_summary_probe.py --fused-only (the kernel_us fields, added by hand
from its statistics)."""
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
    """ms per call: HIP events around `reps` calls, after one warm-up call."""
    fn()                                                  # warm-up: code objects, allocator pool
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def peak_of(fn):
    """Peak allocation of one call above what is allocated before it, in bytes."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    fused_only = "--fused-only" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
        ROOT, "profiles", "y_summary_probe.json")
    rows = []
    for D, N, M, S in SHAPES:
        Q = D * (D + 1) // 2
        per = Q * N + N
        g = torch.Generator(device=dev).manual_seed(D)
        pair_mu = 0.5 * torch.randn(Q, N, dtype=F64, device=dev, generator=g)
        pair_sd = 0.05 + 0.45 * torch.rand(Q, N, dtype=F64, device=dev, generator=g)
        G = torch.randn(S, D, N, dtype=F64, device=dev, generator=g)
        zc = torch.randn(S, per, dtype=F64, device=dev, generator=g)
        y = torch.randn(N, dtype=F64, device=dev, generator=g)
        I = (torch.arange(N, device=dev) * D) // N
        sd_err = 0.3
        pairs = [(i, j) for i in range(D) for j in range(i + 1)]
        rows_idx = torch.arange(N, device=dev)
        z = lambda *shape: torch.zeros(*shape, dtype=F64, device=dev)
        ws = H.y_workspace(D, N, S, dev)

        def fused():
            """Allocations and initialisation of the sums included, as summarize_Y does once per call."""
            Y, F = torch.empty(S, N, dtype=F64, device=dev), torch.empty(S, N, dtype=F64, device=dev)
            st = [z(N), z(N), z(N, D), z(N, D), z(D, N), z(D, N)]
            lse = torch.full((N,), float("-inf"), dtype=F64, device=dev), z(N)
            H.y_accum_(pair_mu, pair_sd, G, zc, zc[:, Q * N:], I, sd_err, Y, F, *st, y=y, lse_max=lse[0],
                       lse_sum=lse[1], ws=ws)
            return Y, st[2] / S, st[4] / S

        def materialised():
            z_p = zc[:, :Q * N].reshape(S, Q, N)
            z_f = zc[:, Q * N:Q * N + N]
            Ls = pair_mu.unsqueeze(0) + pair_sd.unsqueeze(0) * z_p
            Lfull = torch.zeros(S, D, D, N, dtype=F64, device=dev)
            for q, (i, j) in enumerate(pairs):
                Lfull[:, i, j] = torch.exp(Ls[:, q]) if i == j else Ls[:, q]
            l = Lfull.permute(0, 3, 1, 2)[:, rows_idx, I]
            F = (l * G.transpose(1, 2)).sum(2)
            return F + sd_err * z_f, l.mean(0), G.mean(0)

        n_pairs = int((I + 1).sum())                                # pairs the rows need, summed over the inputs
        fused_read = 8 * (S * (3 * n_pairs + D * N + N) + 4 * n_pairs)   # z_p twice, G once per pass, F, mu / sd
        row = {"D": D, "N": N, "M": M, "S_chunk": S, "noise_block_MB": round(zc.numel() * 8 / 1e6, 1),
               "pair_tensor_MB": round(S * D * D * N * 8 / 1e6, 1), "fused_slices": 0 if ws is None else int(
                   ws.numel() // (4 * (D + 1) * N * 8)), "fused_read_MB": round(fused_read / 1e6, 1)}
        Yb, Fb = torch.empty(S, N, dtype=F64, device=dev), torch.empty(S, N, dtype=F64, device=dev)
        stb = [z(N), z(N), z(N, D), z(N, D), z(D, N), z(D, N), torch.full((N,), float("-inf"), dtype=F64, device=dev),
               z(N)]

        def fused_call():
            H.y_accum_(pair_mu, pair_sd, G, zc, zc[:, Q * N:], I, sd_err, Yb, Fb, *stb[:6], y=y, lse_max=stb[6],
                       lse_sum=stb[7], ws=ws)

        if fused_only:
            print(json.dumps({"D": D, "fused_call_ms": round(timed(fused_call, 50), 4)}), flush=True)
            continue
        Ym, lm, gm = materialised()
        Yf, lf, gf = fused()
        torch.cuda.synchronize()
        row["max_abs_Y_diff"] = float((Yf - Ym).abs().max())
        row["max_abs_L_mean_diff"] = float((lf - lm).abs().max())
        row["max_abs_G_mean_diff"] = float((gf - gm).abs().max())
        del Ym, lm, gm, Yf, lf, gf
        row["fused_peak_MB"] = round(peak_of(fused) / 1e6, 1)
        row["materialised_peak_MB"] = round(peak_of(materialised) / 1e6, 1)
        t_f, t_m = [], []
        for _ in range(3):                                          # alternate the two sides
            t_f.append(timed(fused, 2000))
            t_m.append(timed(materialised, 3))
        row["fused_call_ms"] = round(timed(fused_call, 2000), 4)
        row["fused_ms"], row["materialised_ms"] = [round(t, 4) for t in t_f], [round(t, 2) for t in t_m]
        row["fused_ms_median"] = sorted(row["fused_ms"])[1]
        row["materialised_ms_median"] = sorted(row["materialised_ms"])[1]
        row["materialised_over_fused"] = round(row["materialised_ms_median"] / row["fused_ms_median"], 1)
        row["fused_read_GBs"] = round(fused_read / row["fused_ms_median"] / 1e6, 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del pair_mu, pair_sd, G, zc
        torch.cuda.empty_cache()
    if fused_only:
        return
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump({"device": torch.cuda.get_device_name(0),
               "timing": "HIP events, 1 warm-up call per window, windows of 2000 (fused: allocations, zeroing and "
                         "the call) / 3 (materialised) calls, three alternating rounds, medians",
               "rows": rows}, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
