"""The local pre-estimation (csrc/prelocal.hip, the window form of csrc/preest.hip, pre_nmgp.pre_estimate(cov_rows=...))
timed with HIP events after warm-up, medians of repeated calls: the factor launch, the eigen and rotation step
(hip_ops.syevj of the M local matrices and hip_ops.bmm of the fit rows), and the search on the windows.  Beside each
shape: the global pre_estimate launch at the same (x, Y, z, P), and the numpy host statement of the factor step
(gather, Y_w^T Y_w, Cholesky per window) on the CPU of the same box.

  python tools/pre_local_probe.py [--out profiles/pre_local_probe.json]

Shapes (D, M, Pc, P, N): PM2.5-like (5, 256, 64, 10, 10000), HCP-like (50, 512, 200, 10, 4096), ECoG-like
(128, 1024, 512, 10, 4096).  The factor kernel's share of the fp64 matrix peak is stated from the measured time and
2 Pc D^2 / 2 flops per window (the lower triangle of Y_w^T Y_w; the tiles the kernel computes hold a little more).
hip_ops.syevj runs matrices above 64 x 64 one after another (block Jacobi, csrc/eig.hip), so at D > 64 the eigen step is
timed once, not nine times, and the whole call from numpy is not repeated.  No time is fixed in advance."""
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import provenance  # noqa: E402
from collaborative_nonstationary_multivariate_gaussian_process_amd import hip_ops as H  # noqa: E402
from collaborative_nonstationary_multivariate_gaussian_process_amd import pre_nmgp as PN  # noqa: E402

SHAPES = [("PM2.5-like", 5, 256, 64, 10, 10000), ("HCP-like", 50, 512, 200, 10, 4096),
          ("ECoG-like", 128, 1024, 512, 10, 4096)]
FP64_MFMA_PEAK_TFLOPS = 78.6
dev = torch.device("cuda", 0)


def timed(fn, reps=9, warm=2):
    """Median ms of `reps` calls, each between its own pair of events, after `warm` calls."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def synth(N, D, seed):
    """Outputs whose mixing matrix changes half-way along the input, plus noise."""
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(0.0, 1.0, N))
    warp = x + 1.5 * x * x
    K = 3 if D < 16 else D + 8
    lat = np.stack([np.sin(2 * np.pi * (0.5 * k + 1.5) * warp + rng.uniform(0, 2 * np.pi)) for k in range(K)], axis=1)
    A0, A1 = rng.standard_normal((K, D)), rng.standard_normal((K, D))
    w = 1.0 / (1.0 + np.exp(-20.0 * (x - 0.5)))
    Y = ((lat * (1 - w)[:, None]).dot(A0) + (lat * w[:, None]).dot(A1)) / math.sqrt(K) + 0.3 * rng.standard_normal((N, D))
    return x, Y


def host_factor(x, Y, B, z, P, Pc, w, alpha):
    """The factor step in numpy: the hold-out covariance window, B_m and its Cholesky factor, window by window."""
    out = np.empty((len(z),) + B.shape)
    for m, zm in enumerate(z):
        o = np.argsort(np.abs(x - zm), kind="stable")[P:P + Pc]
        Yw = Y[np.sort(o)]
        out[m] = np.linalg.cholesky(w * Yw.T.dot(Yw) + alpha * B)
    return out


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
        ROOT, "profiles", "pre_local_probe.json")
    rows = []
    for name, D, M, Pc, P, N in SHAPES:
        x, Y = synth(N, D, D + M)
        z = np.linspace(0.02, 0.98, M)
        Pc_, w, alpha, holdout = PN._local_plan(N, D, P, Pc, None, True)
        serial_eig = D > 64
        glob = PN.pre_estimate(x, Y, z, P=P, device=dev)
        xd, zd, Yd = torch.from_numpy(x).to(dev), torch.from_numpy(z).to(dev), torch.from_numpy(Y).to(dev)
        B = torch.from_numpy(glob["B"]).to(dev)
        fac = H.pre_local_factor_(xd, Yd, B, zd, P, Pc, w, alpha, holdout)
        eig = {}

        def eigen_rotate():
            eig["mu"], V = H.syevj(fac["B_local"])
            eig["Yr"] = H.bmm(fac["Yloc"], V)

        row = {"shape": name, "D": D, "M": M, "Pc": Pc, "P": P, "N": N, "alpha": round(alpha, 6)}
        med, lo, hi = timed(eigen_rotate, reps=1, warm=0) if serial_eig else timed(eigen_rotate)
        row["eigen_rotate_ms"] = {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3),
                                  "calls": 1 if serial_eig else 9}
        mu, Yr = eig["mu"], eig["Yr"]
        res = H.pre_estimate_windows_(fac["xs"], Yr, mu)
        mug, VB = H.syevj(B)
        Yrot = H.matmul(Yd, VB)
        gout = H.pre_estimate_(xd, Yrot, mug, zd, P)
        for key, fn in (("factor_ms", lambda: H.pre_local_factor_(xd, Yd, B, zd, P, Pc, w, alpha, holdout, out=fac)),
                        ("search_windows_ms", lambda: H.pre_estimate_windows_(fac["xs"], Yr, mu, out=res)),
                        ("global_search_ms", lambda: H.pre_estimate_(xd, Yrot, mug, zd, P, out=gout))):
            med, lo, hi = timed(fn)
            row[key] = {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3)}
        if not serial_eig:
            med, lo, hi = timed(lambda: PN.pre_estimate(x, Y, z, P=P, device=dev, cov_rows=Pc), reps=5, warm=1)
            row["whole_local_call_ms"] = {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3)}
        med, lo, hi = timed(lambda: PN.pre_estimate(x, Y, z, P=P, device=dev), reps=5, warm=1)
        row["whole_global_call_ms"] = {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3)}
        flops = M * 2.0 * Pc * D * D / 2.0
        tf = flops / (row["factor_ms"]["median"] * 1e-3) / 1e12
        row["factor_syrk_flops"] = flops
        row["factor_tflops"] = round(tf, 4)
        row["factor_share_of_fp64_mfma_peak"] = round(tf / FP64_MFMA_PEAK_TFLOPS, 5)
        host_factor(x, Y, glob["B"], z[:8], P, Pc, w, alpha)
        t0 = time.perf_counter()
        Lh = host_factor(x, Y, glob["B"], z, P, Pc, w, alpha)
        row["cpu_numpy_factor_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        row["max_rel_L_diff_vs_numpy"] = float(np.max(np.linalg.norm(fac["L"].cpu().numpy() - Lh, axis=(1, 2))
                                                      / np.linalg.norm(Lh, axis=(1, 2))))
        lflags = (res["flags"] | fac["flags"]).cpu().numpy()
        for tag, fl in (("local", lflags), ("global", glob["flags"])):
            row[tag + "_flag_counts"] = {str(b): int((fl & b != 0).sum()) for b in (1, 2, 4, 8, 16, 32, 64)}
        row["mean_nll_local"], row["mean_nll_global"] = float(res["nll"].mean().item()), float(glob["nll"].mean())
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump({"device": torch.cuda.get_device_name(0), "code_hash": provenance.code_hash(),
               "timing": "HIP events around each call; 2 warm-up calls, then the median (min, max) of 9 calls (1 and 5 "
                         "for the whole calls from numpy); the CPU side by perf_counter after a short warm-up",
               "fp64_mfma_peak_tflops": FP64_MFMA_PEAK_TFLOPS, "cpu_threads": torch.get_num_threads(), "rows": rows},
              open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
