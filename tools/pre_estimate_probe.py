"""The pre-estimation (csrc/preest.hip, pre_nmgp.py), timed with HIP events after warm-up: the launch alone
(hip_ops.pre_estimate_ on prepared device inputs) and the whole call (pre_nmgp.pre_estimate from numpy: upload, B,
its Cholesky factor and eigendecomposition, the rotation GEMM, the launch, the download), against the cost of the
reference's objective on the CPU of the same box.

  python tools/pre_estimate_probe.py [--out profiles/pre_estimate_probe.json]

Shapes (D, M, P, N) = (5, 256, 10, 10000) and (128, 1024, 10, 4096).  The reference's objective
(code/pre_nmgp.py:48-62) is restated here as it is there -- kron(K, B) + s I of size P D x P D handed to a dense
Gaussian log-density -- and timed on three windows; its BFGS needs some tens of evaluations per window (a
two-parameter finite-difference gradient costs 3 evaluations per iteration), so the reference's time for M windows
is EXTRAPOLATED as M x EVALS_PER_WINDOW x the measured time of one evaluation, and marked so.  No speed is fixed in
advance."""
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

SHAPES = [(5, 256, 10, 10000), (128, 1024, 10, 4096)]
EVALS_PER_WINDOW = 60
dev = torch.device("cuda", 0)


def timed(fn, min_ms=300.0, max_reps=20):
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


def synth(N, D, seed):
    rng = np.random.default_rng(seed)
    x = np.sort(rng.uniform(0.0, 1.0, N))
    warp = x + 1.5 * x * x
    K = 3 if D < 16 else D + 8
    lat = np.stack([np.sin(2 * np.pi * (0.5 * k + 1.5) * warp + rng.uniform(0, 2 * np.pi)) for k in range(K)], axis=1)
    return x, lat.dot(rng.standard_normal((K, D))) / math.sqrt(K) + 0.3 * rng.standard_normal((N, D))


def dense_objective(xs, Y_loc, B, log_s, log_ell):
    """The reference's objective: the dense P D x P D Gaussian negative log-density."""
    P, D = Y_loc.shape
    u = xs / max(math.exp(log_ell), 1e-8)
    K = np.exp(-0.5 * (u[:, None] - u[None, :]) ** 2)
    C = np.kron(K, B) + np.eye(P * D) * math.exp(log_s)
    Lc = np.linalg.cholesky(C)
    a = np.linalg.solve(Lc, Y_loc.reshape(-1))
    return 0.5 * float(a.dot(a)) + float(np.log(np.diag(Lc)).sum()) + 0.5 * P * D * math.log(2 * math.pi)


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
        ROOT, "profiles", "pre_estimate_probe.json")
    rows = []
    for D, M, P, N in SHAPES:
        x, Y = synth(N, D, D + M)
        z = np.linspace(0.02, 0.98, M)
        full = PN.pre_estimate(x, Y, z, P=P, device=dev)
        Yd = torch.from_numpy(Y).to(dev)
        B = torch.from_numpy(full["B"]).to(dev)
        mu, VB = H.syevj(B)
        Yrot = H.matmul(Yd, VB)
        xd, zd = torch.from_numpy(x).to(dev), torch.from_numpy(z).to(dev)
        out = H.pre_estimate_(xd, Yrot, mu, zd, P)
        row = {"D": D, "M": M, "P": P, "N": N}
        ms, reps = timed(lambda: H.pre_estimate_(xd, Yrot, mu, zd, P, out=out))
        row["launch_ms"], row["launch_reps"] = round(ms, 3), reps
        ms, reps = timed(lambda: PN.pre_estimate(x, Y, z, P=P, device=dev), max_reps=5)
        row["whole_call_ms"], row["whole_call_reps"] = round(ms, 3), reps
        fl = full["flags"]
        row["windows_on_an_edge"] = int((fl & 15 != 0).sum())
        row["flag_counts"] = {str(b): int((fl & b != 0).sum()) for b in (1, 2, 4, 8, 16, 32)}
        ts = []
        for m in (0, M // 2, M - 1):
            idx = full["neighbours"][m]
            ls, le = full["sigma2_err_log_array"][m], full["v_array"][m]
            dense_objective(x[idx], Y[idx], full["B"], ls, le)
            t0 = time.perf_counter()
            v = dense_objective(x[idx], Y[idx], full["B"], ls, le)
            ts.append(time.perf_counter() - t0)
            row.setdefault("dense_minus_kernel_nll", []).append(float(v - full["nll"][m]))
        row["cpu_dense_eval_ms"] = round(1e3 * float(np.mean(ts)), 3)
        row["cpu_reference_EXTRAPOLATED_s"] = round(M * EVALS_PER_WINDOW * float(np.mean(ts)), 1)
        row["extrapolation"] = f"{M} windows x {EVALS_PER_WINDOW} evaluations x the mean of 3 timed evaluations"
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump({"device": torch.cuda.get_device_name(0), "code_hash": provenance.code_hash(),
               "timing": "HIP events; 1 warm-up call, 1 sizing call, then the mean of max(3, 300 ms of) calls (at "
                         "most 20; at most 5 for the whole call); the CPU side by perf_counter, second call",
               "cpu_threads": torch.get_num_threads(), "rows": rows}, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
