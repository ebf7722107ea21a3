"""Fused Adam off the GPU: the float64 reference itself, the CPU (_foreach)
path, operand validation, and the discriminating power of the comparison the
GPU tests use (tests/test_adam_gpu.py).

``reference_adam_step`` is anchored to ``torch.optim.Adam`` in float64; every
other Adam test is then a comparison with it.
"""

import pytest
import torch

from deeprest_amd.ops import reference_adam_step
from deeprest_amd.ops.adam import (FusedAdam, adam_error_bound, adam_step_errors,
                                   check_adam_operands, fused_adam_step,
                                   reference_adam_run)

HYPERS = [  # (lr, beta1, beta2, eps, weight_decay)
    (1e-2, 0.9, 0.999, 1e-8, 0.0),
    (1e-2, 0.9, 0.999, 1e-8, 0.01),
    (3e-3, 0.8, 0.99, 1e-3, 0.1),
    (1e-2, 0.0, 0.9, 1e-8, 0.0),
]
HYPER_NUMELS = [4096, 1, 300]
# (gradient scale, eps) where the placement of eps shows in the result
EPS_SENSITIVE = [(1e-3, 1e-3), (1e-6, 1e-8)]


def _inputs(numels, steps, scale=1.0, seed=0, dtype=torch.float64):
    gen = torch.Generator().manual_seed(seed)
    params = [torch.randn(n, generator=gen, dtype=dtype) for n in numels]
    grads = [[torch.randn(n, generator=gen, dtype=dtype) * scale for n in numels]
             for _ in range(steps)]
    return params, grads


def _late(grads, tensor, first_step):
    """No gradient for ``tensor`` before step ``first_step`` (1-based)."""
    return [[None if (i == tensor and s + 1 < first_step) else g
             for i, g in enumerate(gs)] for s, gs in enumerate(grads)]


# ------------------------------------------------------------- the reference
@pytest.mark.parametrize("hyper", HYPERS)
@pytest.mark.parametrize("late", [None, 0, 1])
def test_reference_matches_torch_adam_in_float64(hyper, late):
    lr, b1, b2, eps, wd = hyper
    params, grads = _inputs([37, 5], steps=5)
    if late is not None:
        grads = _late(grads, late, first_step=4)
    torch_p = [p.clone().requires_grad_(True) for p in params]
    opt = torch.optim.Adam(torch_p, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for gs in grads:
        for p, g in zip(torch_p, gs):
            p.grad = None if g is None else g.clone()
        opt.step()
    ref_p, ref_m, ref_v, steps = reference_adam_run(params, grads, lr, b1, b2, eps, wd)
    assert steps == [int(opt.state[p]["step"]) for p in torch_p]
    for p, rp, rm, rv in zip(torch_p, ref_p, ref_m, ref_v):
        assert (p.detach() - rp).abs().max() <= 1e-12
        assert (opt.state[p]["exp_avg"] - rm).abs().max() <= 1e-12
        assert (opt.state[p]["exp_avg_sq"] - rv).abs().max() <= 1e-12


def test_reference_is_out_of_place_and_float32_mode_stays_float32():
    params, grads = _inputs([9], steps=1, dtype=torch.float32)
    m, v = [torch.zeros(9)], [torch.zeros(9)]
    keep = [t.clone() for t in params + grads[0] + m + v]
    out = reference_adam_step(params, grads[0], m, v, [1], 1e-2, 0.9, 0.999, 1e-8,
                              0.01, dtype=torch.float32)
    assert all(t.dtype == torch.float32 for lst in out for t in lst)
    assert all(torch.equal(a, b) for a, b in zip(keep, params + grads[0] + m + v))
    ref = reference_adam_step(params, grads[0], m, v, [1], 1e-2, 0.9, 0.999, 1e-8, 0.01)
    assert all(t.dtype == torch.float64 for lst in ref for t in lst)


# ------------------------------------------------------ the CPU _foreach path
@pytest.mark.parametrize("late", [1, 0])
def test_late_gradient_cpu_path(late):
    """A parameter whose first gradient arrives at step 4 of 5 starts its bias
    correction at 1 then, whichever position it has in the group."""
    lr, b1, b2, eps, wd = 1e-2, 0.9, 0.999, 1e-8, 0.0
    params, grads = _inputs([37, 5], steps=5)
    grads = _late(grads, late, first_step=4)
    ours = [p.clone().requires_grad_(True) for p in params]
    opt = FusedAdam(ours, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for gs in grads:
        for p, g in zip(ours, gs):
            p.grad = None if g is None else g.clone()
        opt.step()
    ref_p, ref_m, ref_v, steps = reference_adam_run(params, grads, lr, b1, b2, eps, wd)
    assert steps[late] == 2 and steps[1 - late] == 5
    sd = opt.state_dict()["state"]
    assert [sd[i]["step"] for i in range(2)] == steps
    for p, rp, rm, rv in zip(ours, ref_p, ref_m, ref_v):
        assert (p.detach() - rp).abs().max() <= 1e-12
        assert (opt.state[p]["exp_avg"] - rm).abs().max() <= 1e-12
        assert (opt.state[p]["exp_avg_sq"] - rv).abs().max() <= 1e-12


def test_fused_adam_step_groups_tensors_by_step():
    lr, b1, b2, eps, wd = 3e-3, 0.8, 0.99, 1e-3, 0.1
    numels = [3, 1, 8, 5]
    steps = [7, 1, 7, 120]
    params, grads = _inputs(numels, steps=1, seed=3)
    gen = torch.Generator().manual_seed(4)
    m = [torch.randn(n, generator=gen, dtype=torch.float64) * 0.1 for n in numels]
    v = [torch.rand(n, generator=gen, dtype=torch.float64) * 0.1 for n in numels]
    ref = reference_adam_step(params, grads[0], m, v, steps, lr, b1, b2, eps, wd)
    p2, g2, m2, v2 = ([t.clone() for t in lst] for lst in (params, grads[0], m, v))
    fused_adam_step(p2, g2, m2, v2, steps, lr, b1, b2, eps, wd)
    for got, want in zip((p2, m2, v2), ref):
        for a, b in zip(got, want):
            assert (a - b).abs().max() <= 1e-12
    with pytest.raises(ValueError, match="steps"):
        fused_adam_step(p2, g2, m2, v2, [1, 2], lr)


def test_resume_keeps_per_parameter_steps_cpu():
    params, grads = _inputs([6, 4], steps=6)
    grads = _late(grads, 1, first_step=3)

    def make():
        ps = [p.clone().requires_grad_(True) for p in params]
        return ps, FusedAdam(ps, lr=1e-2)

    def run(ps, opt, gss):
        for gs in gss:
            for p, g in zip(ps, gs):
                p.grad = None if g is None else g.clone()
            opt.step()

    straight, opt_s = make()
    run(straight, opt_s, grads)
    first, opt_a = make()
    run(first, opt_a, grads[:3])
    second = [p.detach().clone().requires_grad_(True) for p in first]
    opt_b = FusedAdam(second, lr=1e-2)
    opt_b.load_state_dict(opt_a.state_dict())
    run(second, opt_b, grads[3:])
    assert [opt_b.state[p]["step"] for p in second] == [6, 4]
    for a, b in zip(straight, second):
        assert torch.equal(a, b)


# --------------------------------------------------------- operand validation
def _quad(n=3):
    mk = lambda: [torch.zeros(4, 6) for _ in range(n)]
    return mk(), mk(), mk(), mk()


def test_check_adam_operands_accepts_what_the_kernel_takes():
    p, g, m, v = _quad()
    p.append(torch.zeros(0)); g.append(torch.zeros(0))
    m.append(torch.zeros(0)); v.append(torch.zeros(0))
    check_adam_operands(p, g, m, v)


def test_check_adam_operands_transposed_param():
    p, g, m, v = _quad()
    p[1] = torch.zeros(6, 4).t()
    with pytest.raises(ValueError, match=r"param of tensor 1 is not contiguous"):
        check_adam_operands(p, g, m, v)


def test_check_adam_operands_bf16_grad():
    p, g, m, v = _quad()
    g[2] = g[2].to(torch.bfloat16)
    with pytest.raises(ValueError, match=r"grad of tensor 2 is torch\.bfloat16"):
        check_adam_operands(p, g, m, v)


def test_check_adam_operands_short_exp_avg():
    p, g, m, v = _quad()
    m[0] = torch.zeros(23)
    with pytest.raises(ValueError, match=r"exp_avg of tensor 0 has 23 elements"):
        check_adam_operands(p, g, m, v)
    p, g, m, v = _quad()
    with pytest.raises(ValueError, match=r"2 exp_avg_sq tensors for 3 params"):
        check_adam_operands(p, g, m, v[:2])


# --------------------------------- what the GPU comparison can tell apart
def _mutant_run(kind, params, grads, lr, b1, b2, eps, wd):
    """The reference's formula in float64 with one deliberate mistake:
    ``eps_in_sqrt``: sqrt(v / c2 + eps); ``eps_over_bias``: eps / sqrt(c2);
    ``frozen_bias``: bias correction stuck at step 1.  ``None``: no mistake."""
    p = [t.clone() for t in params]
    m = [torch.zeros_like(t) for t in p]
    v = [torch.zeros_like(t) for t in p]
    for s, gs in enumerate(grads):
        k = 1 if kind == "frozen_bias" else s + 1
        c1, c2 = 1.0 - b1 ** k, 1.0 - b2 ** k
        for i, g in enumerate(gs):
            if wd != 0.0:
                g = g + wd * p[i]
            m[i] = b1 * m[i] + (1.0 - b1) * g
            v[i] = b2 * v[i] + (1.0 - b2) * g * g
            if kind == "eps_in_sqrt":
                denom = torch.sqrt(v[i] / c2 + eps)
            elif kind == "eps_over_bias":
                denom = torch.sqrt(v[i] / c2) + eps / c2 ** 0.5
            else:
                denom = torch.sqrt(v[i] / c2) + eps
            p[i] = p[i] - (lr / c1) * m[i] / denom
    return p, m, v


def _eps_sensitive_case(scale, eps):
    lr, b1, b2, wd = 1e-2, 0.9, 0.999, 0.0
    params, grads = _inputs(HYPER_NUMELS, steps=8, scale=scale, seed=11,
                            dtype=torch.float32)
    ref = reference_adam_run(params, grads, lr, b1, b2, eps, wd)[:3]
    emu = reference_adam_run(params, grads, lr, b1, b2, eps, wd,
                             dtype=torch.float32)[:3]
    return params, grads, (lr, b1, b2, eps, wd), ref, emu


@pytest.mark.parametrize("scale,eps", EPS_SENSITIVE)
def test_unmutated_formula_is_the_reference(scale, eps):
    params, grads, hyper, ref, _ = _eps_sensitive_case(scale, eps)
    same = _mutant_run(None, [p.double() for p in params],
                       [[g.double() for g in gs] for gs in grads], *hyper)
    err = adam_step_errors(same, ref, hyper[0] * 8)
    assert max(err.values()) <= 1e-12, err


@pytest.mark.parametrize("kind", ["eps_in_sqrt", "eps_over_bias", "frozen_bias"])
def test_reference_mutants_fail_the_comparison(kind):
    """Each mutant must land outside the bound the GPU tests grant a kernel on
    at least one eps-sensitive input, by the margin the bound was chosen for:
    the nearest mutant moves p by >= 5.6e-4 lr*steps, several times 4x the
    f32 emulation's own error."""
    worst = 0.0
    for scale, eps in EPS_SENSITIVE:
        params, grads, hyper, ref, emu = _eps_sensitive_case(scale, eps)
        emu_err = adam_step_errors(emu, ref, hyper[0] * 8)
        bound = adam_error_bound(emu_err["p"])
        mut = _mutant_run(kind, [p.double() for p in params],
                          [[g.double() for g in gs] for gs in grads], *hyper)
        mut_err = adam_step_errors(mut, ref, hyper[0] * 8)
        print(f"{kind} scale={scale:g} eps={eps:g}: emulation p={emu_err['p']:.3g} "
              f"bound={bound:.3g} mutant p={mut_err['p']:.3g} "
              f"margin={mut_err['p'] / bound:.1f}x")
        # the emulation itself passes its own comparison
        assert all(emu_err[k] <= adam_error_bound(emu_err[k]) for k in emu_err)
        worst = max(worst, mut_err["p"] / bound)
        if mut_err["p"] > bound:
            assert mut_err["p"] >= 5.6e-4
    assert worst >= 5.0, f"{kind}: only {worst:.2f}x the bound"


@pytest.mark.parametrize("hyper", HYPERS)
def test_emulation_error_is_what_f32_commits(hyper):
    """The f32 emulation's distance from float64 over the hyperparameter cases
    stays where it was measured when the bound was chosen (p <= 2.0e-5, m <=
    3e-7, v <= 1.3e-5): the 4x bound derived from it cannot silently grow."""
    lr, b1, b2, eps, wd = hyper
    params, grads = _inputs(HYPER_NUMELS, steps=8, seed=11, dtype=torch.float32)
    ref = reference_adam_run(params, grads, lr, b1, b2, eps, wd)[:3]
    emu = reference_adam_run(params, grads, lr, b1, b2, eps, wd,
                             dtype=torch.float32)[:3]
    err = adam_step_errors(emu, ref, lr * 8)
    print(hyper, err)
    assert err["p"] <= 4e-5 and err["m"] <= 6e-7 and err["v"] <= 2.6e-5, err


def test_adam_step_errors_flags_nan_and_zero_scale():
    ref = ([torch.zeros(3, dtype=torch.float64)],) * 3
    nan = ([torch.tensor([0.0, float("nan"), 0.0])],) * 3
    assert all(e == float("inf") for e in adam_step_errors(nan, ref, 1e-2).values())
    assert all(e == 0.0 for e in adam_step_errors(ref, ref, 0.0).values())
    off = ([torch.full((3,), 1e-3)],) * 3
    assert adam_step_errors(off, ref, 0.0)["p"] == float("inf")
