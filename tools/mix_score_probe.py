"""The exact mixture scores (csrc/mixscore.hip), timed with HIP events after warm-up: one hip_ops.mix_score_ call
(CRPS, its spread term and PIT) against the torch route on the same box -- the same closed form through elementwise
torch passes over an (S, S, e-block) temporary, in entry blocks sized to a fixed budget for the temporaries.

  python tools/mix_score_probe.py [--fused-only] [--out profiles/mix_score_probe.json]

Shapes (S, E) = (1000, 4096) with a variance per component (the impute_Y case) and (1000, 4096) with one scalar
variance (the summarize_Y case).  Reported per shape: ms, pair terms per second (E S (S - 1) / 2 useful terms per
call on either side; the torch route evaluates all S^2), the growth of torch's peak allocation, the largest
difference between the two routes, and the kernel's time for two exact quantiles on top.  The kernel's time does
not depend on the values.  No speed is fixed in advance."""
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
SHAPES = [(1000, 4096, True), (1000, 4096, False)]
BUDGET = 2 << 30                  # bytes of (S, S, e-block) temporaries the torch route may hold at once
LIVE = 6                          # such temporaries alive at the peak of one block (m, v, s, z, two summands)
QS = (0.025, 0.975)
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


def A(m, v):
    s = torch.sqrt(v)
    z = m / s
    return m * torch.erf(z * math.sqrt(0.5)) + s * (math.sqrt(2.0 / math.pi) * torch.exp(-0.5 * z * z))


def torch_route(Mu, Var, y):
    """crps, spread, pit by the closed form, the pair terms in blocks of entries."""
    S, E = Mu.shape
    het = torch.is_tensor(Var)
    eb = max(1, BUDGET // (S * S * 8 * LIVE))
    spread = torch.empty(E, dtype=F64, device=Mu.device)
    for e0 in range(0, E, eb):
        m = Mu[:, e0:e0 + eb]
        v = Var[:, e0:e0 + eb] if het else torch.full_like(m, Var)
        spread[e0:e0 + eb] = A(m[:, None] - m[None], v[:, None] + v[None]).sum((0, 1)) / (2.0 * S * S)
    v = Var if het else torch.full_like(Mu, Var)
    t1 = A(y[None] - Mu, v).mean(0)
    pit = (0.5 * torch.erfc(-(y[None] - Mu) / torch.sqrt(2.0 * v))).mean(0)
    return t1 - spread, spread, pit


def main():
    fused_only = "--fused-only" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
        ROOT, "profiles", "mix_score_probe.json")
    rows = []
    for S, E, het in SHAPES:
        g = torch.Generator(device=dev).manual_seed(S + E + het)
        Mu = torch.randn(S, E, dtype=F64, device=dev, generator=g) + torch.randn(E, dtype=F64, device=dev, generator=g)
        Var = 0.2 + 1.3 * torch.rand(S, E, dtype=F64, device=dev, generator=g) if het else 0.37
        y = 1.5 * torch.randn(E, dtype=F64, device=dev, generator=g)
        ws = H.mix_score_workspace(S, E, dev)
        out = {k: torch.empty(E, dtype=F64, device=dev) for k in ("pit", "crps", "spread")}
        outq = dict(out, quantiles=torch.empty(len(QS), E, dtype=F64, device=dev),
                    unconverged=torch.zeros(1, dtype=torch.int32, device=dev))

        def fused():
            return H.mix_score_(Mu, Var, y=y, ws=ws, out=out)

        def fused_q():
            return H.mix_score_(Mu, Var, y=y, qs=QS, ws=ws, out=outq)

        pairs = E * S * (S - 1) // 2
        row = {"S": S, "E": E, "variance": "per component" if het else "scalar", "pair_terms": pairs,
               "workspace_MB": round(ws.numel() / 1e6, 2)}
        ms, reps = timed(fused)
        row["fused_ms"], row["fused_reps"] = round(ms, 3), reps
        row["fused_pair_terms_per_s"] = float(f"{pairs / (ms * 1e-3):.4g}")
        row["fused_peak_MB"] = peak_of(fused)
        msq, _ = timed(fused_q)
        row["fused_with_2_quantiles_ms"] = round(msq, 3)
        row["unconverged"] = int(outq["unconverged"])
        if not fused_only:
            crps, spread, pit = torch_route(Mu, Var, y)
            fused()
            torch.cuda.synchronize()
            row["max_abs_crps_diff"] = float((out["crps"] - crps).abs().max())
            row["max_abs_spread_diff"] = float((out["spread"] - spread).abs().max())
            row["max_abs_pit_diff"] = float((out["pit"] - pit).abs().max())
            del crps, spread, pit
            ms, reps = timed(lambda: torch_route(Mu, Var, y), max_reps=3)
            row["torch_ms"], row["torch_reps"] = round(ms, 3), reps
            row["torch_pair_terms_per_s"] = float(f"{pairs / (ms * 1e-3):.4g}")
            row["torch_peak_MB"] = peak_of(lambda: torch_route(Mu, Var, y))
            row["torch_entry_block"] = max(1, BUDGET // (S * S * 8 * LIVE))
            row["torch_over_fused"] = round(ms / row["fused_ms"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del Mu, Var, y
        torch.cuda.empty_cache()
    if not fused_only:
        os.makedirs(os.path.dirname(out_path), exist_ok=True)
        json.dump({"device": torch.cuda.get_device_name(0), "code_hash": provenance.code_hash(),
                   "timing": "HIP events; 1 warm-up call, 1 sizing call, then the mean of max(3, 300 ms of) calls "
                             "(at most 50; at most 3 on the torch side)",
                   "peak": "growth of torch's peak allocation during one call over the shared inputs",
                   "torch_route": f"the same closed form, pair terms in entry blocks under {BUDGET >> 20} MiB of "
                                  f"temporaries ({LIVE} live (S, S, block) tensors)",
                   "rows": rows}, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
