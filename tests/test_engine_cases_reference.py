"""The generated step inputs of tests/_engine_cases.py leave the fp64 gates to the kernels (CPU).

The oracle (LU solves, autograd) and the closed-form mirror (Cholesky, explicit inverses) are two independent
float64 evaluations of the same step; where they agree to a tenth of the project's fp64 gates (loss 1e-10,
gradient rel-norm 1e-8), an engine outside those gates on the same inputs is wrong, not unlucky.  A condition on
the inputs, not a measurement of the engine.
"""
import pytest
import torch

from oracle import nmgp_oracle as O
from tests import _engine_cases as EC

LOSS_TOL, GRAD_TOL = 1e-11, 1e-9

ALL = {EC.case_id(c): c for c in EC.FP64_CASES + EC.FP32_CASES}


def test_case_tables_are_well_formed():
    for table in (EC.FP64_CASES, EC.FP32_CASES):
        assert len({EC.case_id(c) for c in table}) == len(table)     # (the ids name the parametrised tests)
        for D, M, sizes, flags in table:
            assert len(sizes) == D and D >= 2 and len(flags) == len(EC.Flags)
    for c in EC.ELBO_CASES:
        assert any(tuple(c) == k[:3] for k in EC.FP64_CASES)


def test_make_case_is_deterministic():
    a, b = EC.make_case(3, 65, [9, 0, 22]), EC.make_case(3, 65, [9, 0, 22])
    assert all(torch.equal(a["p"][k], b["p"][k]) for k in O.PARAM_NAMES)
    assert (a["noise"] == b["noise"]).all() and all((u == v).all() for u, v in zip(a["xl"] + a["yl"], b["xl"] + b["yl"]))
    assert a["noise"].shape == (65 + 31 + 6 * 31,) and a["noise"].dtype.name == "float64"
    assert [len(x) for x in a["xl"]] == [9, 0, 22] and all((x[1:] >= x[:-1]).all() for x in a["xl"])
    assert EC.make_case(3, 65, [9, 0, 22], n_sample=3)["noise"].shape == (3 * a["noise"].shape[0],)
    assert not (EC.make_case(3, 65, [9, 0, 22], seed=1)["noise"] == a["noise"]).all()


@pytest.mark.parametrize("cid", list(ALL))
def test_oracle_and_mirror_agree_on_the_case(cid):
    D, M, sizes, _ = ALL[cid]
    c = EC.make_case(D, M, sizes)
    loss, inter, ref = EC.oracle_step(c)             # (asserts tape.done())
    eye = 1e-4 * torch.eye(M, dtype=O.DT)
    conds = {k: float(torch.linalg.cond(inter[k].detach() + eye)) for k in ("K_t22", "K_L0_22", "K_L1_22", "K_G22")}
    l2, gr, _ = EC.mirror_step(c)
    lerr = abs(float(l2) - loss) / abs(loss)
    whole, errs = EC.grad_errs(gr, ref)
    print(f"INPUTS {cid}: loss rel {lerr:.2e} (gate {LOSS_TOL:.0e}: {LOSS_TOL / max(lerr, 1e-300):.0f}x)  "
          f"whole-gradient rel-norm {whole:.2e}  worst parameter {max(errs, key=errs.get)} {max(errs.values()):.2e} "
          f"(gate {GRAD_TOL:.0e}: {GRAD_TOL / max(max(errs.values()), 1e-300):.0f}x)  cond(K22 + 1e-4 I) "
          + "  ".join(f"{k} {v:.2e}" for k, v in conds.items()))
    assert lerr <= LOSS_TOL, lerr
    assert whole <= GRAD_TOL, whole
    bad = {k: e for k, e in errs.items() if e > GRAD_TOL}
    assert not bad, bad
    for k in O.PARAM_NAMES:                          # the same parameters carry a gradient in both
        assert (float(ref[k].norm()) == 0) == (float(gr[k].norm()) == 0), k
