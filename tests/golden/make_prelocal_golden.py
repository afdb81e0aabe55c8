"""Record the reference's objective on windows with a local coefficient factor: tests/golden/prelocal_cases.npz.

    NMGP_REFERENCE_DIR=<reference checkout> python tests/golden/make_prelocal_golden.py

The reference's pre_estimation_all (code/pre_nmgp.py:64-100) never returns, so there is no run of it to record.  What
is recorded is its real objective_part (code/pre_nmgp.py:58-62) minimised by scipy's BFGS from (-6, -6), window by
window, with the HOST's local factor L_m (tests/_prelocal_ref.py) in place of the global one.  Per case: x (N,),
Y (N, D), z (M,); per window BFGS's (log s, log ell), the dense-logpdf nll at that point, scipy's success, and
same_basin = |nll_BFGS - nll_host| <= 1e-6 max(1, |nll|) against the host optimum.  P = 10 (the reference takes 10
neighbours whatever P says, code/pre_nmgp.py:11), Pc = 40, hold-out, default shrink.
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
from tests import _prelocal_ref as PL       # noqa: E402

P, PC = 10, 40
# (name, N, D, M, seed)
CASES = [("local_a", 120, 2, 5, 34), ("local_b", 150, 5, 6, 35)]


def main():
    out = {"names": np.array([c[0] for c in CASES]), "P": np.int64(P), "Pc": np.int64(PC)}
    same_all = []
    for name, N, D, M, seed in CASES:
        x, Y, z = PL.synth_local(N, D, M, seed)
        est = PL.estimate_local(x, Y, z, P, PC, holdout=True)
        rec = {k: [] for k in ("bfgs_log_s", "bfgs_log_ell", "bfgs_nll", "bfgs_success", "same_basin")}
        for m, zm in enumerate(z):
            x_loc, Y_loc = ref.search_nearest_neighhood(x, Y, zm, P=P)
            idx = est["neighbours"][m]
            assert set(idx.tolist()) == set(np.argsort(np.abs(x - zm))[:P].tolist())
            res = minimize(ref.objective_part, np.array([-6, -6]), args=(x_loc, Y_loc, est["L"][m]))
            nll_b = float(ref.objective_part(res.x, x_loc, Y_loc, est["L"][m]))
            host = float(est["nll"][m])
            gate = PR.eval_gate(est["xs"][m], est["Yrot_loc"][m], est["mu"][m], est["log_s"][m], est["log_ell"][m])
            assert host <= nll_b + gate, (name, zm, host, nll_b, gate)
            rec["bfgs_log_s"].append(res.x[0])
            rec["bfgs_log_ell"].append(res.x[1])
            rec["bfgs_nll"].append(nll_b)
            rec["bfgs_success"].append(bool(res.success))
            rec["same_basin"].append(abs(nll_b - host) <= 1e-6 * max(1.0, abs(nll_b)))
            print(name, f"z={zm:.4g} bfgs=({res.x[0]:.4f}, {res.x[1]:.4f}) nll={nll_b:.6f} "
                        f"host=({est['log_s'][m]:.4f}, {est['log_ell'][m]:.4f}) nll={host:.6f} "
                        f"flags={est['flags'][m]} success={res.success}")
        out[name + "/x"], out[name + "/Y"], out[name + "/z"] = x, Y, z
        for k, v in rec.items():
            out[name + "/" + k] = np.asarray(v)
        same_all.append(out[name + "/same_basin"])
    same = np.concatenate(same_all)
    print(f"same_basin: {int(same.sum())} of {same.size}")
    assert 2 * int(same.sum()) >= same.size, "fewer than half of the windows share BFGS's basin: new seed"
    np.savez_compressed(os.path.join(HERE, "prelocal_cases.npz"), **out)


if __name__ == "__main__":
    main()
