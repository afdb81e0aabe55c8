"""The fused start of the captured training step, nmgp_step_head_* (step_begin, the RBF K22 builders and Sigma_v as
workgroups of one grid), against the three launches it replaces (NMGP_FUSE_HEAD=0 keeps them): bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

DEV = "cuda"
F64 = torch.float64


def _setup(M, B, head=True):
    """A D = 3 fp64 model on nb = 2 bound minibatches (rows sorted by output), its trainer and its engine."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd.nmgp_dsvi import NMGP, DsviTrainer
    D, nb = 3, 2
    mp = pytest.MonkeyPatch()
    if not head:
        mp.setenv("NMGP_FUSE_HEAD", "0")
    model = NMGP(number_observations=D * 400, dim_outputs=D, Z=np.linspace(0, 1, M), minibatch_size=B, seed=9,
                 device=DEV, noise="device", dtype=F64)
    tr = DsviTrainer(model, 0.01)
    eng = model.engine(B)
    g = np.random.default_rng(4)
    Xb = torch.tensor(g.uniform(0, 1, (nb, B)), dtype=F64, device=DEV)
    Yb = torch.tensor(g.standard_normal((nb, B)), dtype=F64, device=DEV)
    ids = np.sort(g.integers(0, D, (nb, B)), axis=1)
    Ib = torch.tensor(ids, dtype=torch.int32, device=DEV)
    Sb = torch.tensor(np.stack([np.concatenate([[0], np.cumsum(np.bincount(r, minlength=D))]) for r in ids]),
                      dtype=torch.int32, device=DEV)
    eng.bind_dataset(Xb, Yb, Ib, Sb)
    return mp, model, tr, eng


# M = 144: masked 32-wide tiles and the 16-column tail of both tile bodies; B = 63: an odd row count
HEAD_SHAPES = [(256, 240), (144, 63), (128, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("M,B,aligned", [s + (True,) for s in HEAD_SHAPES] + [(144, 63, False)])
def test_head_launch_matches_its_three_launches(M, B, aligned):
    """nmgp_step_head_* against begin_step + p["build_k22"] + p["syrk"] on the same engine, two calls each: minibatch,
    segment table, noise, the zeroed gradient (once through a pointer that is not 16-byte aligned), the three
    K22 + lam I, the lower triangle of Sigma_v + lam I, both counters."""
    mp, model, tr, eng = _setup(M, B)
    try:
        assert eng.head_groups() is not None
        g = torch.Generator().manual_seed(M + B)
        with torch.no_grad():
            model._theta.add_(0.05 * torch.randn(model._theta.numel(), generator=g, dtype=F64).to(DEV))
        p = eng._plan(0)
        NF, FV, MM = eng.NF, eng.NF - 1, M * M
        nctr, bctr = model._noise_counter, eng._dataset[4]
        grad0 = eng._grad
        if not aligned:
            eng._grad = torch.empty(grad0.numel() + 1, dtype=F64, device=DEV)[1:]
            assert eng._grad.data_ptr() % 16 == 8
        outs = []
        for head in (False, True):
            bctr.fill_(1)
            nctr.fill_(5)
            eng._grad.fill_(7.0)
            eng.Afac.fill_(3.0)
            for t in (eng.x, eng.y, eng.noise):
                t.fill_(-1.0)
            for _ in range(2):
                if head:
                    eng.head_step(model._noise_seed, nctr)
                else:
                    eng.begin_step(model._noise_seed, nctr)
                    p["build_k22"](eng.dt)
                    p["syrk"]()
            torch.cuda.synchronize()
            A = eng.Afac.reshape(-1)
            k22 = [A[(NF + k) * MM:(NF + k + 1) * MM].clone() for k in range(3)]
            sv = torch.tril(A[FV * MM:(FV + 1) * MM].reshape(M, M)).clone()
            outs.append([t.clone() for t in (eng.x, eng.y, eng.row_out, eng.seg, eng.noise, eng._grad, bctr, nctr)]
                        + k22 + [sv])
        eng._grad = grad0
        for a, b in zip(*outs):
            assert torch.equal(a, b)
        assert not bool((outs[1][8] == 3.0).any()) and bool(torch.isfinite(outs[1][11]).all())
        assert int(outs[1][6]) == 3 and int(outs[1][7]) == 7 and int(eng._begin_done.item()) == 0
        assert float(outs[1][5].abs().max()) == 0.0
    finally:
        mp.undo()


def _steps(M, B, head):
    """out[0:5] and the gradient after two eager steps, then after three replays of the captured step"""
    mp, model, tr, eng = _setup(M, B, head=head)
    try:
        assert (eng.head_groups() is not None) == head
        for _ in range(2):
            tr.grad_step(eng)
        torch.cuda.synchronize()
        res = [eng.out[0:5].cpu().clone(), model._grad.detach().cpu().clone()]
        graph = tr.capture(eng, include_update=True)
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
        return res + [eng.out[0:5].cpu().clone(), model._grad.detach().cpu().clone(),
                      model._theta.detach().cpu().clone()]
    finally:
        mp.undo()


@pytest.mark.gpu
@pytest.mark.parametrize("M,B", HEAD_SHAPES)
def test_step_with_head_launch_matches_step_without(M, B):
    for a, b in zip(_steps(M, B, True), _steps(M, B, False)):
        assert torch.equal(a, b)
        assert bool(torch.isfinite(a).all())


def test_head_entry_points_reject_missing_groups():
    """nmgp_step_head_* return their error codes before anything is launched (no GPU needed): a NULL dataset pointer as
    nmgp_step_begin_*, a missing pairwise group, a missing grouped GEMM."""
    from collaborative_nonstationary_multivariate_gaussian_process_amd import _lib as L
    lib = L.lib()
    vp = ctypes.c_void_p
    ok = 0x10000
    for sfx in ("f64", "f32"):
        h = getattr(lib, "nmgp_step_head_" + sfx)
        beg = [vp(ok)] * 4 + [8, 3, 2] + [vp(ok)] * 6 + [64, ctypes.c_uint64(1), vp(ok), vp(ok), vp(ok), 128]
        assert h(*beg, None, 1, 4, vp(ok), 1, 8, None, None) == -20
        assert h(*beg, vp(ok), 1, 0, vp(ok), 1, 8, None, None) == -20
        assert h(*beg, vp(ok), 1, 4, None, 1, 8, None, None) == -23
        assert h(*([None] + beg[1:]), vp(ok), 1, 4, vp(ok), 1, 8, None, None) == -1
