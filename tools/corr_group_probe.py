"""One chunk of group-mean correlations, timed with HIP events after warm-up: the fused kernel of
predict.summarize_FY(corr_groups=...) (csrc/cgroup.hip) alone for three group tables, next to fy_accum_ (csrc/fy.hip)
on the same inputs in the same process -- the yardstick: the group kernel does the same MFMA work plus one LDS write of
the normalised triangle and one pass over the table.

  python tools/corr_group_probe.py [--out profiles/corr_group_probe.json]

Shapes: HCP (D = 50, M = 512) and ECoG (D = 128, M = 1024), N = 800; S is one chunk of predict._chunk_size at
n_sample = 1000.  Tables: "all" (one group of every pair), "networks7" (the within / between groups of 7 networks of
predict.groups_from_labels: 28 groups that read each pair once) and "grid5x5" (the ECoG driver's neighbour groups
left / top / right / bottom and its distance groups 1, 2, 3 on a 5 x 5 electrode grid, reference
NMGP_ECoG_full.py:456-544).  The expectation to confirm or refute, from the operation count: within 1.5x of fy_accum_
for "networks7".  No speed is fixed in advance."""
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


def grid_groups(D, n=5):
    """The direction groups (each electrode with its left, top, right, bottom neighbour) and the distance groups
    (all pairs 1, 2, 3 steps apart along a grid axis) of an n x n grid of electrodes spread over the D outputs."""
    at = lambda i, j: (i * n + j) * (D // (n * n))
    left, top, right, bottom = [], [], [], []
    for i in range(n):
        for j in range(n):
            if i >= 1:
                left.append((at(i, j), at(i - 1, j)))
            if j + 1 < n:
                top.append((at(i, j), at(i, j + 1)))
            if i + 1 < n:
                right.append((at(i, j), at(i + 1, j)))
            if j >= 1:
                bottom.append((at(i, j), at(i, j - 1)))
    dist = []
    for d in (1, 2, 3):
        g = []
        for i in range(n - d):
            for j in range(n - d):
                g += [(at(i, j), at(i + d, j)), (at(i, j), at(i, j + d))]
        dist.append(g)
    return [left, top, right, bottom] + dist


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
        ROOT, "profiles", "corr_group_probe.json")
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

        row = {"shape": name, "D": D, "N": N, "M": M, "S_chunk": S, "noise_block_MB": round(zc.numel() * 8 / 1e6, 1)}
        ms, reps = timed(fy)
        row["fy_accum_ms"], row["fy_accum_reps"] = round(ms, 3), reps
        tables = {"all": [[(i, j) for i in range(D) for j in range(i)]],
                  "networks7": predict.groups_from_labels([d % 7 for d in range(D)])[0],
                  "grid5x5": grid_groups(D)}
        for tname, groups in tables.items():
            goff, gent = H.group_table(groups, D, dev)
            C = torch.empty(len(groups), N, S, dtype=F64, device=dev)
            ms, reps = timed(lambda: H.corr_group_(pair_mu, pair_sd, zc, goff, gent, C))
            row[tname] = {"groups": len(groups), "entries": int(gent.numel()),
                          "largest_group": max(len(x) for x in groups), "ms": round(ms, 3), "reps": reps,
                          "over_fy_accum": round(ms / row["fy_accum_ms"], 3), "C_MB": round(C.numel() * 8 / 1e6, 1)}
            del C
        rows.append(row)
        print(json.dumps(row), flush=True)
        del pair_mu, pair_sd, zc, Gm, Y, csum, csq, ws
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump({"code_hash": code_hash(), "device": torch.cuda.get_device_name(0),
               "timing": "HIP events; 1 warm-up call, 1 sizing call, then the mean of max(3, 300 ms of) calls (at "
                         "most 50); fy_accum_ and the group kernel in the same process on the same inputs",
               "rows": rows}, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
