"""Fused Adam on the GPU: both kernels against the float64 reference.

Every numeric case runs ``FusedAdam(capturable=False)`` (host-step kernel) and
``FusedAdam(capturable=True)`` (device-step kernel) and compares ``p``,
``exp_avg`` and ``exp_avg_sq`` of every tensor with ``reference_adam_step`` in
float64.

Tolerance: no figure picked in advance.  For each case the test computes the
error of the reference's float32 emulation (every scalar and operation rounded
to f32, exact pow) against float64 on the same inputs; the kernel must stay
within 4x that error (floor 1e-6), in units of ``max|dp| / sum(lr)`` for the
parameters and ``max|d| / max|ref|`` for the moments
(``ops.adam.adam_step_errors`` / ``adam_error_bound``).
tests/test_adam_cpu.py shows that three plausible mistakes in the formula fall
outside this bound by four orders of magnitude.  Each comparison prints an
``ADAM-RATIO`` line (kernel error / emulation error); docs/KERNELS.md records
the largest per path.

Layout cases carve every p, g, m and v out of the middle of a larger buffer
with an odd guard of 33 elements on each side: a one-off at a tensor boundary
shows in a guard, and every pointer is only 4-byte aligned.
"""

import copy
import functools

import pytest
import torch

from deeprest_amd.ops.adam import (FusedAdam, adam_error_bound, adam_step_errors,
                                   fused_adam_step, reference_adam_run)

pytestmark = pytest.mark.gpu

GUARD = 33
FILL = -7.25  # exact in f32; nothing the steps compute lands on it
PATHS = [pytest.param(False, id="host-step"), pytest.param(True, id="device-step")]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deeprest_amd.ops import native_available

    if not native_available():
        pytest.fail("HIP extension not built — GPU tests must not fall back")
    return torch.device("cuda:0")


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


@functools.lru_cache(maxsize=None)
def _inputs(shapes, steps, scale=1.0, seed=0):
    """Seeded f32 parameters and per-step gradients on the host, built once per
    case and shared by both paths; never modified."""
    gen = torch.Generator().manual_seed(seed)
    params = tuple(torch.randn(s, generator=gen) for s in shapes)
    grads = tuple(tuple(torch.randn(s, generator=gen) * scale for s in shapes)
                  for _ in range(steps))
    return params, grads


_REFERENCES = {}


def _reference(key, params, grads, lrs, hyper, state=None):
    """(float64 reference, f32 emulation) of one case, computed once."""
    if key not in _REFERENCES:
        _, b1, b2, eps, wd = hyper
        _REFERENCES[key] = tuple(
            reference_adam_run(params, grads, lrs, b1, b2, eps, wd, state=state,
                               dtype=dt)
            for dt in (torch.float64, torch.float32))
    return _REFERENCES[key]


def _carve(t, dev):
    """``t`` as the middle of a guarded buffer on the device: (buffer, view)."""
    buf = torch.full((t.numel() + 2 * GUARD,), FILL, device=dev)
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _guards_intact(buf):
    fill = torch.full((GUARD,), FILL, device=buf.device)
    return torch.equal(buf[:GUARD], fill) and torch.equal(buf[-GUARD:], fill)


class _Run:
    """One optimizer over device copies of ``params``; gradients are copied
    into fixed buffers, so the capturable path keeps its table across steps
    unless the set of tensors with a gradient changes."""

    def __init__(self, dev, capturable, params, hyper, carve=False):
        lr, b1, b2, eps, wd = hyper
        self.bufs = []
        self.keep = []
        self.p, self.g = [], []
        m, v = [], []
        for t in params:
            views = []
            for src in (t, torch.zeros_like(t), torch.zeros_like(t), torch.zeros_like(t)):
                if carve:
                    buf, view = _carve(src, dev)
                    self.bufs.append(buf)
                else:
                    view = src.to(dev).clone()
                views.append(view)
            self.p.append(views[0].requires_grad_(True))
            self.g.append(views[1])
            m.append(views[2])
            v.append(views[3])
        self.opt = FusedAdam(self.p, lr=lr, betas=(b1, b2), eps=eps,
                             weight_decay=wd, capturable=capturable)
        if carve:  # moments inside guarded buffers too
            for p, mi, vi in zip(self.p, m, v):
                self.opt.state[p] = {"step": 0, "exp_avg": mi, "exp_avg_sq": vi}

    def step(self, grads, new_addresses=False):
        for p, buf, g in zip(self.p, self.g, grads):
            if g is None:
                p.grad = None
            elif new_addresses:
                self.keep.append(p.grad)  # kept alive: the next one is elsewhere
                p.grad = g.to(buf.device)
            else:
                buf.copy_(g)
                p.grad = buf
        self.opt.step()

    def result(self):
        torch.cuda.synchronize()
        st = self.opt.state
        return ([p.detach().cpu() for p in self.p],
                [st[p]["exp_avg"].cpu() if p in st else torch.zeros(p.shape) for p in self.p],
                [st[p]["exp_avg_sq"].cpu() if p in st else torch.zeros(p.shape) for p in self.p])

    def steps(self):
        sd = self.opt.state_dict()["state"]
        return [sd[i]["step"] if i in sd else 0 for i in range(len(self.p))]


def _assert_within_bound(label, capturable, got, ref, emu, lr_steps):
    kernel = adam_step_errors(got, ref[:3], lr_steps)
    emulation = adam_step_errors(emu[:3], ref[:3], lr_steps)
    path = "device-step" if capturable else "host-step"
    ratios = " ".join(
        f"{k}={kernel[k]:.3g}/{emulation[k]:.3g}"
        f"({kernel[k] / emulation[k] if emulation[k] > 0 else float(kernel[k] > 0):.2f}x)"
        for k in "pmv")
    print(f"ADAM-RATIO {path} {label}: {ratios}")
    for k in "pmv":
        assert kernel[k] <= adam_error_bound(emulation[k]), \
            f"{label} {path} {k}: kernel {kernel[k]:.3g}, emulation {emulation[k]:.3g}"


# ------------------------------------------------------------------- layouts
_CYCLE = tuple({12: (3, 4), 16: (2, 2, 4)}.get(n, (n,))
               for n in (i % 17 + 1 for i in range(131)))
LAYOUTS = {
    "one-element": ((1,),),
    "three-single-elements": ((1,), (1, 1), (1, 1, 1)),
    "empty-tensors": ((0,), (5,), (0, 3), (0,), (7,), (2, 0, 4)),
    "wave-and-block-edges": ((255,), (1,), (257,), (7, 9), (5, 13), (4, 4, 4)),
    "131-tensors": _CYCLE,
    # 4096 blocks x 256 threads = 1 048 576 elements per grid pass
    "small-tensors-in-second-pass": ((1_048_576 + 300,), (3,), (7, 111)),
    "boundary-in-second-pass": ((700_000,), (700, 1000)),
}
LAYOUT_HYPER = (1e-3, 0.9, 0.999, 1e-8, 0.01)


def test_layout_cases_are_the_sizes_meant():
    numels = {k: [_numel(s) for s in v] for k, v in LAYOUTS.items()}
    assert numels["empty-tensors"] == [0, 5, 0, 0, 7, 0]
    assert numels["wave-and-block-edges"] == [255, 1, 257, 63, 65, 64]
    assert numels["131-tensors"] == [i % 17 + 1 for i in range(131)]
    assert numels["small-tensors-in-second-pass"] == [1_048_876, 3, 777]
    assert numels["boundary-in-second-pass"] == [700_000, 700_000]


@pytest.mark.parametrize("capturable", PATHS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_layouts(dev, layout, capturable):
    shapes = LAYOUTS[layout]
    params, grads = _inputs(shapes, 3, seed=1)
    ref, emu = _reference(("layout", layout), params, grads, LAYOUT_HYPER[0], LAYOUT_HYPER)
    run = _Run(dev, capturable, params, LAYOUT_HYPER, carve=True)
    for gs in grads:
        run.step(gs)
    got = run.result()
    assert all(_guards_intact(b) for b in run.bufs), "a guard element changed"
    assert run.steps() == [3] * len(shapes)
    _assert_within_bound(layout, capturable, got, ref, emu, 3 * LAYOUT_HYPER[0])


# ----------------------------------------------------------- hyperparameters
HYPER_SHAPES = ((4096,), (1,), (300,))
HYPERS = {  # (lr, beta1, beta2, eps, weight_decay), gradient scale
    "default": ((1e-2, 0.9, 0.999, 1e-8, 0.0), 1.0),
    "weight-decay": ((1e-2, 0.9, 0.999, 1e-8, 0.01), 1.0),
    "all-non-default": ((3e-3, 0.8, 0.99, 1e-3, 0.1), 1.0),
    "beta1-zero": ((1e-2, 0.0, 0.9, 1e-8, 0.0), 1.0),
    # |g| ~ eps: eps inside the sqrt or divided by the bias factor shows here
    "small-grads-eps-1e-3": ((1e-2, 0.9, 0.999, 1e-3, 0.0), 1e-3),
    "tiny-grads-eps-1e-8": ((1e-2, 0.9, 0.999, 1e-8, 0.0), 1e-6),
}


@pytest.mark.parametrize("capturable", PATHS)
@pytest.mark.parametrize("case", list(HYPERS))
def test_hyperparameters(dev, case, capturable):
    hyper, scale = HYPERS[case]
    params, grads = _inputs(HYPER_SHAPES, 8, scale=scale, seed=11)
    ref, emu = _reference(("hyper", case), params, grads, hyper[0], hyper)
    run = _Run(dev, capturable, params, hyper)
    for gs in grads:
        run.step(gs)
    _assert_within_bound(case, capturable, run.result(), ref, emu, 8 * hyper[0])


@pytest.mark.parametrize("capturable", PATHS)
def test_lr_zero_leaves_p_and_updates_moments(dev, capturable):
    hyper = (0.0, 0.9, 0.999, 1e-8, 0.01)
    params, grads = _inputs(HYPER_SHAPES, 8, seed=11)
    ref, emu = _reference("lr-zero", params, grads, 0.0, hyper)
    run = _Run(dev, capturable, params, hyper)
    for gs in grads:
        run.step(gs)
    got = run.result()
    for p, start in zip(got[0], params):
        assert torch.equal(p, start)
    assert all(float(r.abs().max()) > 0 for r in ref[1] + ref[2])
    _assert_within_bound("lr-zero", capturable, got, ref, emu, 0.0)


@pytest.mark.parametrize("capturable", PATHS)
def test_zero_gradients_on_the_first_step(dev, capturable):
    hyper = (1e-2, 0.9, 0.999, 1e-8, 0.0)
    params, grads = _inputs(HYPER_SHAPES, 8, seed=11)
    grads = (tuple(torch.zeros_like(g) for g in grads[0]),) + grads[1:]
    ref, emu = _reference("zero-first", params, grads, hyper[0], hyper)
    run = _Run(dev, capturable, params, hyper)
    run.step(grads[0])
    p1, m1, v1 = run.result()
    for p, start in zip(p1, params):
        assert torch.equal(p, start)
    assert all(bool(torch.isfinite(t).all()) for t in p1 + m1 + v1)
    for gs in grads[1:]:
        run.step(gs)
    _assert_within_bound("zero-first", capturable, run.result(), ref, emu, 8 * hyper[0])


# ----------------------------------------------------------------- step count
@functools.lru_cache(maxsize=None)
def _moments(shapes, seed):
    """Moments a run could have left: |m| <= sqrt(v) elementwise."""
    gen = torch.Generator().manual_seed(seed)
    v = tuple(torch.rand(s, generator=gen) + 0.05 for s in shapes)
    m = tuple((torch.rand(s, generator=gen) * 2 - 1) * t.sqrt() for s, t in zip(shapes, v))
    return m, v


def _state_dict(opt, m, v, steps):
    return {"state": {i: {"step": k, "exp_avg": mi.clone(), "exp_avg_sq": vi.clone()}
                      for i, (mi, vi, k) in enumerate(zip(m, v, steps))},
            "param_groups": copy.deepcopy(opt.state_dict()["param_groups"])}


@pytest.mark.parametrize("capturable", PATHS)
@pytest.mark.parametrize("seeded", [0, 1, 9, 999, 9999])
def test_bias_correction_at_step(dev, seeded, capturable):
    """State seeded to ``seeded`` steps through load_state_dict, one step taken:
    the bias factors 1 - beta^k at k = seeded + 1, computed on the device from
    the device counter on the capturable path."""
    hyper = (1e-2, 0.9, 0.999, 1e-8, 0.0)
    params, grads = _inputs(HYPER_SHAPES, 1, seed=12)
    m, v = _moments(HYPER_SHAPES, 13)
    n = len(params)
    ref, emu = _reference(("at-step", seeded), params, grads, hyper[0], hyper,
                          state=(m, v, [seeded] * n))
    run = _Run(dev, capturable, params, hyper)
    run.opt.load_state_dict(_state_dict(run.opt, m, v, [seeded] * n))
    run.step(grads[0])
    assert run.steps() == [seeded + 1] * n
    _assert_within_bound(f"at-step-{seeded + 1}", capturable, run.result(), ref, emu,
                         hyper[0])


# --------------------------------------------------------------------- replay
def test_graph_replay_keeps_bias_correction_and_follows_set_lr(dev):
    """Two eager warm-up steps and the capture on one side stream, six replays
    with fresh gradients copied on the device and no host synchronization in
    between, set_lr between replays 3 and 4: eight Adam steps."""
    hyper = (1e-2, 0.9, 0.999, 1e-8, 0.01)
    params, grads = _inputs(HYPER_SHAPES, 8, seed=14)
    lrs = [1e-2] * 5 + [2.5e-3] * 3
    ref, emu = _reference("replay", params, grads, lrs, hyper)
    run = _Run(dev, True, params, hyper)
    staged = [[g.to(dev) for g in gs] for gs in grads]
    for p, buf in zip(run.p, run.g):
        p.grad = buf

    def load(s):
        for buf, g in zip(run.g, staged[s]):
            buf.copy_(g)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for s in range(2):
            load(s)
            run.opt.step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        run.opt.step()
    for replay in range(6):
        if replay == 3:
            run.opt.set_lr(2.5e-3)
        load(2 + replay)
        graph.replay()
    torch.cuda.synchronize()
    assert run.steps() == [8] * len(params)
    _assert_within_bound("replay", True, run.result(), ref, emu, sum(lrs))


# --------------------------------------------------------------------- resume
RESUME_SHAPES = ((300,), (1,), (7, 11))
RESUME_HYPER = (1e-2, 0.9, 0.999, 1e-8, 0.01)


def _resumed(dev, save_capturable, load_capturable, stepped_before):
    params, grads = _inputs(RESUME_SHAPES, 6, seed=15)
    first = _Run(dev, save_capturable, params, RESUME_HYPER)
    for gs in grads[:3]:
        first.step(gs)
    saved = copy.deepcopy(first.opt.state_dict())
    start = [p.detach().clone() for p in first.p]
    second = _Run(dev, load_capturable, params, RESUME_HYPER)
    if stepped_before:
        other = _inputs(RESUME_SHAPES, 2, seed=16)[1]
        for gs in other:
            second.step(gs)
    with torch.no_grad():
        for p, s in zip(second.p, start):
            p.copy_(s)
    second.opt.load_state_dict(saved)
    for gs in grads[3:]:
        second.step(gs)
    return second


@functools.lru_cache(maxsize=None)
def _uninterrupted(dev, capturable):
    params, grads = _inputs(RESUME_SHAPES, 6, seed=15)
    run = _Run(dev, capturable, params, RESUME_HYPER)
    for gs in grads:
        run.step(gs)
    return run.result()


@pytest.mark.parametrize("stepped_before", [False, True],
                         ids=["fresh-optimizer", "optimizer-stepped-twice"])
@pytest.mark.parametrize("load_capturable", PATHS)
@pytest.mark.parametrize("save_capturable", PATHS)
def test_resume(dev, save_capturable, load_capturable, stepped_before):
    params, grads = _inputs(RESUME_SHAPES, 6, seed=15)
    ref, emu = _reference("resume", params, grads, RESUME_HYPER[0], RESUME_HYPER)
    second = _resumed(dev, save_capturable, load_capturable, stepped_before)
    got = second.result()
    assert second.steps() == [6] * len(params)
    label = f"resume-{'dev' if save_capturable else 'host'}-to-{'dev' if load_capturable else 'host'}"
    _assert_within_bound(label, load_capturable, got, ref, emu, 6 * RESUME_HYPER[0])
    if save_capturable == load_capturable:
        straight = _uninterrupted(dev, load_capturable)
        for a, b in zip(got[0] + got[1] + got[2], straight[0] + straight[1] + straight[2]):
            assert torch.equal(a, b), "resumed run is not bit-equal to an uninterrupted one"


# -------------------------------------------------------------- late gradient
@pytest.mark.parametrize("capturable", PATHS)
@pytest.mark.parametrize("late", [1, 0], ids=["second-is-late", "first-is-late"])
def test_late_gradient(dev, late, capturable):
    """One parameter gets its first gradient at step 4 of 5: its bias
    correction starts at 1 there, as torch.optim.Adam's does."""
    hyper = (1e-2, 0.9, 0.999, 1e-8, 0.0)
    shapes = ((300,), (5,))
    params, grads = _inputs(shapes, 5, seed=17)
    grads = tuple(tuple(None if (i == late and s < 3) else g for i, g in enumerate(gs))
                  for s, gs in enumerate(grads))
    ref, emu = _reference(("late", late), params, grads, hyper[0], hyper)
    run = _Run(dev, capturable, params, hyper)
    for gs in grads:
        run.step(gs)
    want = [5, 5]
    want[late] = 2
    assert ref[3] == want and run.steps() == want
    _assert_within_bound(f"late-{late}", capturable, run.result(), ref, emu, 5 * hyper[0])


@pytest.mark.parametrize("capturable", PATHS)
def test_gradients_at_new_addresses_every_step(dev, capturable):
    """zero_grad(set_to_none=True) training: every step brings gradients at
    other addresses, so the capturable path rebuilds its table each time and
    must carry the late tensor's lag over."""
    hyper = (1e-2, 0.9, 0.999, 1e-8, 0.0)
    shapes = ((300,), (5,))
    params, grads = _inputs(shapes, 5, seed=19)
    grads = tuple(tuple(None if (i == 1 and s < 2) else g for i, g in enumerate(gs))
                  for s, gs in enumerate(grads))
    ref, emu = _reference("new-addresses", params, grads, hyper[0], hyper)
    run = _Run(dev, capturable, params, hyper)
    for gs in grads:
        run.step(gs, new_addresses=True)
    assert run.steps() == [5, 3]
    _assert_within_bound("new-addresses", capturable, run.result(), ref, emu, 5 * hyper[0])


# ------------------------------------------------------------ scheduler idiom
@pytest.mark.parametrize("capturable", PATHS)
def test_param_group_lr_is_followed_between_eager_steps(dev, capturable):
    hyper = (1e-2, 0.9, 0.999, 1e-8, 0.0)
    params, grads = _inputs(HYPER_SHAPES, 6, seed=18)
    lrs = [1e-2, 1e-2, 4e-3, 4e-3, 1e-3, 1e-3]
    ref, emu = _reference("scheduler", params, grads, lrs, hyper)
    run = _Run(dev, capturable, params, hyper)
    for gs, lr in zip(grads, lrs):
        for group in run.opt.param_groups:
            group["lr"] = lr
        run.step(gs)
    _assert_within_bound("scheduler", capturable, run.result(), ref, emu, sum(lrs))


# --------------------------------------------------------- rejected operands
# These raise BEFORE any launch (ops.adam.check_adam_operands); a kernel given
# such operands would read or write past a buffer.
def _bad_transposed_param(dev):
    p = torch.randn(6, 4, device=dev).t().requires_grad_(True)
    p.grad = torch.randn(4, 6, device=dev)
    return p, {}, "param of tensor 0 is not contiguous"


def _bad_bf16_grad(dev):
    p = torch.randn(4, 6, device=dev).requires_grad_(True)
    p.grad_dtype = None  # let the gradient's dtype differ from the parameter's
    p.grad = torch.randn(4, 6, device=dev).to(torch.bfloat16)
    return p, {}, "grad of tensor 0 is torch.bfloat16"


def _bad_short_exp_avg(dev):
    p = torch.randn(4, 6, device=dev).requires_grad_(True)
    p.grad = torch.randn(4, 6, device=dev)
    state = {"step": 3, "exp_avg": torch.zeros(23, device=dev),
             "exp_avg_sq": torch.zeros(4, 6, device=dev)}
    return p, state, "exp_avg of tensor 0 has 23 elements"


@pytest.mark.parametrize("capturable", PATHS)
@pytest.mark.parametrize("bad", [_bad_transposed_param, _bad_bf16_grad,
                                 _bad_short_exp_avg])
def test_step_rejects_operands_the_kernel_cannot_take(dev, bad, capturable):
    p, state, message = bad(dev)
    before = p.detach().clone()
    opt = FusedAdam([p], lr=1e-2, capturable=capturable)
    if state:
        opt.state[p] = state
    with pytest.raises(ValueError, match=message):
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(p.detach(), before)


def test_fused_adam_step_rejects_before_launch(dev):
    p, g, m, v = (torch.zeros(4, 6, device=dev) for _ in range(4))
    with pytest.raises(ValueError, match="exp_avg_sq of tensor 0 has 5 elements"):
        fused_adam_step([p], [g], [m], [v[0, :5].clone()], 1, 1e-2)
    torch.cuda.synchronize()
    assert not p.any()
