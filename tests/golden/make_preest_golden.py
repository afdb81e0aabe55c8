"""Record what the reference's pre-estimation does on small synthetic nonstationary data:
tests/golden/preest_cases.npz.

    NMGP_REFERENCE_DIR=<reference checkout> python tests/golden/make_preest_golden.py

Imports the real `code/pre_nmgp.py` of the reference and runs its BFGS (pre_estimation_partial's loop, one window at
a time so that scipy's `success` can be kept).  Per case: x (N,), Y (N, D), z (M,); per window BFGS's
(log s, log ell), the dense-logpdf nll at that point, scipy's success, and same_basin =
|nll_BFGS - nll_host| <= 1e-6 max(1, |nll|) against the host reference's optimum (tests/_preest_ref.py).  The
reference takes 10 neighbours whatever P says (code/pre_nmgp.py:11), so every case is P = 10.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = os.environ.get("NMGP_REFERENCE_DIR")
if not REF:
    sys.exit("set NMGP_REFERENCE_DIR to the reference checkout")
sys.path.insert(0, os.path.join(REF, "code"))

import pre_nmgp as ref                      # noqa: E402  (the real reference)
from scipy.optimize import minimize         # noqa: E402

from tests import _preest_ref as PR         # noqa: E402

P = 10
# (name, N, D, M, input scale, seed)
CASES = [("unit_a", 100, 2, 6, 1.0, 11), ("unit_b", 200, 5, 8, 1.0, 22), ("unit_c", 120, 12, 5, 1.0, 13),
         ("hour", 300, 5, 6, 300.0, 14)]


def synth(N, D, M, scale, seed):
    """Outputs that share K = 3 latent waves whose frequency grows along the input, plus noise."""
    rng = np.random.default_rng(seed)
    u = np.sort(rng.uniform(0.0, 1.0, N))
    warp = u + 1.5 * u * u
    lat = np.stack([np.sin(2 * np.pi * (k + 1.5) * warp + rng.uniform(0, 2 * np.pi)) for k in range(3)], axis=1)
    A = rng.standard_normal((3, D))
    Y = lat.dot(A) + 0.15 * rng.standard_normal((N, D))
    z = np.linspace(0.05, 0.95, M)
    return u * scale, Y, z * scale


def main():
    out = {"names": np.array([c[0] for c in CASES]), "P": np.int64(P)}
    for name, N, D, M, scale, seed in CASES:
        x, Y, z = synth(N, D, M, scale, seed)
        pre = PR.prepare(x, Y)
        L = np.linalg.cholesky(Y.T.dot(Y) / (N - 1))
        rec = {k: [] for k in ("bfgs_log_s", "bfgs_log_ell", "bfgs_nll", "bfgs_success", "same_basin", "host_nll")}
        for zm in z:
            x_loc, Y_loc = ref.search_nearest_neighhood(x, Y, zm, P=P)
            res = minimize(ref.objective_part, np.array([-6, -6]), args=(x_loc, Y_loc, L))
            nll_b = float(ref.objective_part(res.x, x_loc, Y_loc, L))
            idx = PR.neighbours(x, zm, P)
            assert set(idx.tolist()) == set(np.argsort(np.abs(x - zm))[:P].tolist())
            xs, Yr = pre["x"][idx], pre["Yrot"][idx]
            host = PR.search(xs, Yr, pre["mu"])
            gate = PR.eval_gate(xs, Yr, pre["mu"], host["log_s"], host["log_ell"])
            assert host["nll"] <= nll_b + gate, (name, zm, host["nll"], nll_b, gate)
            rec["bfgs_log_s"].append(res.x[0])
            rec["bfgs_log_ell"].append(res.x[1])
            rec["bfgs_nll"].append(nll_b)
            rec["bfgs_success"].append(bool(res.success))
            rec["host_nll"].append(host["nll"])
            rec["same_basin"].append(abs(nll_b - host["nll"]) <= 1e-6 * max(1.0, abs(nll_b)))
            print(name, f"z={zm:.4g} bfgs=({res.x[0]:.4f}, {res.x[1]:.4f}) nll={nll_b:.6f} "
                        f"host=({host['log_s']:.4f}, {host['log_ell']:.4f}) nll={host['nll']:.6f} "
                        f"flags={host['flags']} success={res.success}")
        out[name + "/x"], out[name + "/Y"], out[name + "/z"] = x, Y, z
        for k, v in rec.items():
            if k != "host_nll":
                out[name + "/" + k] = np.asarray(v)
    unit = np.concatenate([out[c[0] + "/same_basin"] for c in CASES if c[4] == 1.0])
    print(f"same_basin on the unit-scale windows: {int(unit.sum())} of {unit.size}")
    assert 2 * int(unit.sum()) >= unit.size, "fewer than half of the unit-scale windows share BFGS's basin: new seed"
    np.savez_compressed(os.path.join(HERE, "preest_cases.npz"), **out)


if __name__ == "__main__":
    main()
