"""What the correlation bands add to predict.summarize_FY, timed with HIP events after a warm-up call, and the two
kernels of csrc/corrq.hip alone.

  python tools/corr_band_probe.py [--shape K] [--kernels-only] [--out profiles/corr_band_probe.json]

Shapes (D, N, M, S): (50, 1000, 512, 1000) and (128, 1000, 1024, 1000); --shape K runs only shape K.  Per shape:
  * kernels alone, on synthetic pair marginals and noise: nmgp_corr_collect_f64 for 256 pairs (and for every pair at
    D = 50) over all S samples in chunks of predict._chunk_size samples, and nmgp_quantile_rows_f64 on the collected
    (pairs * N, S) rows;
  * summarize_FY on a default-initialised model (fp32 parameters at D = 128: the packed sqrt_U is 35 GB; the
    summary itself runs in fp64 either way): one warm-up call with 256 pairs, then one timed call each with
    corr_pairs=None, 256 pairs and, at D = 50, "all"; the peak allocation of each call.
Nothing is fixed in advance: the numbers are the share the band passes add over the corr_pairs=None run of the
same build."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from collaborative_nonstationary_multivariate_gaussian_process_amd import hip_ops as H  # noqa: E402
from collaborative_nonstationary_multivariate_gaussian_process_amd import predict  # noqa: E402
from collaborative_nonstationary_multivariate_gaussian_process_amd.nmgp_dsvi import NMGP  # noqa: E402

F64 = torch.float64
SHAPES = [(50, 1000, 512, 1000), (128, 1000, 1024, 1000)]
QS = (0.025, 0.975)
dev = torch.device("cuda", 0)


def events(fn, reps=1):
    """ms per call of fn, between two HIP events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def pairs_256(D):
    """256 pairs spread over the rows of the lower triangle, in row order."""
    allp = [(i, j) for i in range(D) for j in range(i)]
    idx = np.linspace(0, len(allp) - 1, 256).round().astype(int)
    return [allp[k] for k in idx]


def kernel_rows(D, N, M, S):
    Q = D * (D + 1) // 2
    chunk = predict._chunk_size(S, N, M)
    g = torch.Generator(device=dev).manual_seed(D)
    pair_mu = 0.5 * torch.randn(Q, N, dtype=F64, device=dev, generator=g)
    pair_sd = 0.05 + 0.45 * torch.rand(Q, N, dtype=F64, device=dev, generator=g)
    zc = torch.randn(chunk, Q * N, dtype=F64, device=dev, generator=g)
    rows = []
    lists = [("256", pairs_256(D))] + ([("all", [(i, j) for i in range(D) for j in range(i)])] if D <= 50 else [])
    for name, pl in lists:
        P = len(pl)
        pij = torch.tensor(pl, dtype=torch.int32, device=dev)
        pi, pj = pij[:, 0].contiguous(), pij[:, 1].contiguous()
        C = torch.empty(P, N, S, dtype=F64, device=dev)

        def collect():
            for s0 in range(0, S, chunk):
                n = min(chunk, S - s0)
                H.corr_collect_(pair_mu, pair_sd, zc[:n], pi, pj, C, s_off=s0)

        def quant():
            return H.quantile_rows(C.reshape(P * N, S), QS)

        collect(), quant()                                   # warm-up: code objects, allocator pool
        t_c, t_q = events(collect, 3), events(quant, 3)
        terms = sum(max(i, j) + 1 + 2 * (min(i, j) + 1) for i, j in pl)      # upper bound: no row is held
        rows.append({"D": D, "N": N, "S": S, "S_chunk": chunk, "pairs": name, "P": P,
                     "collect_ms": round(t_c, 3), "quantile_ms": round(t_q, 3),
                     "collect_loaded_GBs": round(3 * 8 * terms * N * S / t_c / 1e6, 1),
                     "collect_stored_GBs": round(8 * P * N * S / t_c / 1e6, 1),
                     "quantile_rows_per_ms": round(P * N / t_q, 1), "C_MB": round(C.numel() * 8 / 1e6, 1)})
        print(json.dumps(rows[-1]), flush=True)
        del C
    return rows


def summary_rows(D, N, M, S):
    m = NMGP(N, D, np.linspace(0.0, 1.0, M), dtype=torch.float32 if D > 64 else F64, pair_layout="packed")
    xf = torch.linspace(0.0, 1.0, N, dtype=F64)
    p256 = pairs_256(D)
    runs = [("none", None), ("256", p256)] + ([("all", "all")] if D <= 50 else [])
    torch.manual_seed(1)
    predict.summarize_FY(m, xf, S, quantiles=QS, corr_pairs=p256)            # warm-up
    rows, base_ms = [], None
    for name, cp in runs:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        torch.manual_seed(1)
        ms = events(lambda: predict.summarize_FY(m, xf, S, quantiles=QS, corr_pairs=cp))
        base_ms = ms if cp is None else base_ms
        rows.append({"D": D, "N": N, "M": M, "S": S, "corr_pairs": name, "summarize_FY_ms": round(ms, 1),
                     "added_over_none_pct": None if cp is None else round(100.0 * (ms - base_ms) / base_ms, 2),
                     "peak_grown_MB": round((torch.cuda.max_memory_allocated() - base) / 1e6, 1)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
        ROOT, "profiles", "corr_band_probe.json")
    shapes = [SHAPES[int(sys.argv[sys.argv.index("--shape") + 1])]] if "--shape" in sys.argv else SHAPES
    res = {"device": torch.cuda.get_device_name(0), "kernels": [], "summarize_FY": [],
           "timing": "HIP events; kernels: 1 warm-up call, mean of 3; summarize_FY: 1 warm-up call (256 pairs), 1 "
                     "timed call per run"}
    for shp in shapes:
        res["kernels"] += kernel_rows(*shp)
        if "--kernels-only" not in sys.argv:
            res["summarize_FY"] += summary_rows(*shp)
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        json.dump(res, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
