"""Fused Adam step.

Replaces torch.optim.Adam's per-tensor eager update loop
(reference: resource-estimation/estimate.py:61,74) with ONE multi-tensor HIP
kernel per step on GPU: all parameter/grad/moment tensors are walked by a
single grid-stride kernel over a packed pointer table, so the optimizer costs
one launch regardless of parameter count.  CPU path uses torch._foreach ops.

Like torch.optim.Adam, every parameter has its own step count: a parameter
that gets its first gradient late starts its bias correction at 1 then.
"""

from __future__ import annotations

from typing import Dict, Iterable, List, Sequence, Union

import torch

from .native import require_native

_OPERANDS = ("param", "grad", "exp_avg", "exp_avg_sq")


def check_adam_operands(params: Sequence[torch.Tensor], grads: Sequence[torch.Tensor],
                        exp_avgs: Sequence[torch.Tensor],
                        exp_avg_sqs: Sequence[torch.Tensor]) -> None:
    """What the kernel assumes of its operands, checked before any launch.

    The kernel walks raw pointers as contiguous f32 of the parameter's numel;
    anything else would be read or written out of bounds.  Raises ValueError
    naming the tensor index and the operand.
    """
    n = len(params)
    for name, lst in zip(_OPERANDS[1:], (grads, exp_avgs, exp_avg_sqs)):
        if len(lst) != n:
            raise ValueError(f"fused adam: {len(lst)} {name} tensors for {n} params")
    for i, quad in enumerate(zip(params, grads, exp_avgs, exp_avg_sqs)):
        for name, t in zip(_OPERANDS, quad):
            if t.dtype != torch.float32:
                raise ValueError(f"fused adam: {name} of tensor {i} is {t.dtype}, "
                                 "expected torch.float32")
            if not t.is_contiguous():
                raise ValueError(f"fused adam: {name} of tensor {i} is not contiguous")
            if t.device != params[0].device:
                raise ValueError(f"fused adam: {name} of tensor {i} is on {t.device}, "
                                 f"expected {params[0].device}")
            if t.numel() != quad[0].numel():
                raise ValueError(f"fused adam: {name} of tensor {i} has {t.numel()} "
                                 f"elements, its param has {quad[0].numel()}")


def reference_adam_step(params, grads, exp_avgs, exp_avg_sqs, steps, lr, beta1,
                        beta2, eps, weight_decay, dtype=torch.float64):
    """One Adam step in plain torch, out of place, one step count per tensor.

    The formula the kernel documents (csrc/adam.hip)::

        g += wd * p;  m = b1 * m + (1 - b1) * g;  v = b2 * v + (1 - b2) * g * g
        p -= lr / (1 - b1^k) * m / (sqrt(v / (1 - b2^k)) + eps)

    ``dtype=torch.float64`` is the reference.  ``dtype=torch.float32`` rounds
    every scalar and tensor to f32 first and every operation once, in the
    kernel's order, with an exactly rounded ``b^k``: an emulation of the
    kernel's arithmetic whose distance from the reference is the error f32
    itself commits on these inputs.

    Returns ``(new_params, new_exp_avgs, new_exp_avg_sqs)`` in ``dtype``.
    """
    def scalar(x):
        return torch.tensor(float(x), dtype=dtype)

    lr_t, b1, b2, eps_t, wd = (scalar(x) for x in (lr, beta1, beta2, eps, weight_decay))
    one = scalar(1.0)
    new_p, new_m, new_v = [], [], []
    for p, g, m, v, k in zip(params, grads, exp_avgs, exp_avg_sqs, steps):
        p, g, m, v = (t.detach().to("cpu", dtype) for t in (p, g, m, v))
        k = int(k)
        # b^k exact for the b this dtype holds, then rounded once
        c1 = one - (b1.double() ** k).to(dtype)
        c2 = one - (b2.double() ** k).to(dtype)
        if float(weight_decay) != 0.0:
            g = g + wd * p
        m = b1 * m + (one - b1) * g
        v = b2 * v + (one - b2) * g * g
        denom = torch.sqrt(v / c2) + eps_t
        new_p.append(p - (lr_t / c1) * m / denom)
        new_m.append(m)
        new_v.append(v)
    return new_p, new_m, new_v


def reference_adam_run(params, grads_per_step, lrs, beta1, beta2, eps, weight_decay,
                       state=None, dtype=torch.float64):
    """Several :func:`reference_adam_step` in a row, as an optimizer would take
    them.  ``grads_per_step[s][i]`` is tensor i's gradient at step s, or None:
    the tensor is then left alone and its own step count does not advance.
    ``lrs``: one lr per step, or one float for all.  ``state``: ``(exp_avgs,
    exp_avg_sqs, steps)`` to continue from (zeros and 0 if None).

    Returns ``(params, exp_avgs, exp_avg_sqs, steps)``.
    """
    n = len(params)
    p = [t.detach().to("cpu", dtype) for t in params]
    if state is None:
        m = [torch.zeros_like(t) for t in p]
        v = [torch.zeros_like(t) for t in p]
        steps = [0] * n
    else:
        m = [t.detach().to("cpu", dtype) for t in state[0]]
        v = [t.detach().to("cpu", dtype) for t in state[1]]
        steps = [int(k) for k in state[2]]
    if isinstance(lrs, (int, float)):
        lrs = [lrs] * len(grads_per_step)
    for grads, lr in zip(grads_per_step, lrs):
        idx = [i for i in range(n) if grads[i] is not None]
        for i in idx:
            steps[i] += 1
        out = reference_adam_step([p[i] for i in idx], [grads[i] for i in idx],
                                  [m[i] for i in idx], [v[i] for i in idx],
                                  [steps[i] for i in idx], lr, beta1, beta2, eps,
                                  weight_decay, dtype=dtype)
        for j, i in enumerate(idx):
            p[i], m[i], v[i] = out[0][j], out[1][j], out[2][j]
    return p, m, v, steps


def adam_step_errors(got, ref, lr_steps: float) -> Dict[str, float]:
    """Distance of ``got = (params, exp_avgs, exp_avg_sqs)`` from the float64
    ``ref`` of the same layout, in the units the Adam tests bound:

    - ``p``: ``max|dp| / lr_steps`` with ``lr_steps`` the sum of lr over the
      steps taken (``lr * steps`` for a constant lr): one Adam step moves a
      parameter by about lr, so this is the error as a share of the distance
      travelled;
    - ``m``, ``v``: ``max|d| / max|ref|`` over all tensors.
    """
    out = {}
    for name, gs, rs in zip(("p", "m", "v"), got, ref):
        err = scale = 0.0
        for g, r in zip(gs, rs):
            if r.numel() == 0:
                continue
            r = r.detach().to("cpu", torch.float64)
            d = (g.detach().to("cpu", torch.float64).reshape(r.shape) - r).abs().max()
            # NaN must not pass as "no error"
            err = float("inf") if not torch.isfinite(d) else max(err, float(d))
            scale = max(scale, float(r.abs().max()))
        unit = lr_steps if name == "p" else scale
        out[name] = err / unit if unit > 0 else (float("inf") if err > 0 else 0.0)
    return out


ADAM_ERROR_FACTOR = 4.0   # FMA contraction, hardware divide / sqrt / pow rounding
ADAM_ERROR_FLOOR = 1e-6


def adam_error_bound(emulation_error: float) -> float:
    """Largest error a kernel may show where the f32 emulation shows
    ``emulation_error``, both against the float64 reference in the units of
    :func:`adam_step_errors`."""
    return max(ADAM_ERROR_FACTOR * emulation_error, ADAM_ERROR_FLOOR)


def _per_tensor_steps(step: Union[int, Sequence[int]], n: int) -> List[int]:
    if isinstance(step, int):
        return [step] * n
    steps = [int(s) for s in step]
    if len(steps) != n:
        raise ValueError(f"fused adam: {len(steps)} steps for {n} params")
    return steps


@torch.no_grad()
def fused_adam_step(
    params: List[torch.Tensor],
    grads: List[torch.Tensor],
    exp_avgs: List[torch.Tensor],
    exp_avg_sqs: List[torch.Tensor],
    step: Union[int, Sequence[int]],
    lr: float,
    beta1: float = 0.9,
    beta2: float = 0.999,
    eps: float = 1e-8,
    weight_decay: float = 0.0,
) -> None:
    """``step``: the step count this update is (1 for the first), one int for
    all tensors or one per tensor."""
    if not params:
        return
    steps = _per_tensor_steps(step, len(params))
    if params[0].is_cuda:
        ext = require_native("fused_adam_step")
        check_adam_operands(params, grads, exp_avgs, exp_avg_sqs)
        ext.fused_adam(params, grads, exp_avgs, exp_avg_sqs, steps,
                       float(lr), float(beta1), float(beta2),
                       float(eps), float(weight_decay))
        return

    if weight_decay != 0.0:
        torch._foreach_add_(grads, params, alpha=weight_decay)
    torch._foreach_mul_(exp_avgs, beta1)
    torch._foreach_add_(exp_avgs, grads, alpha=1.0 - beta1)
    torch._foreach_mul_(exp_avg_sqs, beta2)
    torch._foreach_addcmul_(exp_avg_sqs, grads, grads, value=1.0 - beta2)
    # the bias factors are per step: one _foreach update per group of tensors
    # at the same step (one group unless some parameter's gradients began late)
    by_step: Dict[int, List[int]] = {}
    for i, k in enumerate(steps):
        by_step.setdefault(k, []).append(i)
    for k, idx in by_step.items():
        bias_c1 = 1.0 - beta1 ** k
        bias_c2 = 1.0 - beta2 ** k
        denom = torch._foreach_sqrt(
            torch._foreach_div([exp_avg_sqs[i] for i in idx], bias_c2))
        torch._foreach_add_(denom, eps)
        torch._foreach_addcdiv_([params[i] for i in idx],
                                [exp_avgs[i] for i in idx], denom,
                                value=-(lr / bias_c1))


class FusedAdam(torch.optim.Optimizer):
    """Optimizer wrapper over fused_adam_step (one kernel launch per step on GPU).

    ``capturable=True`` makes ``step()`` hipGraph-safe: the packed pointer
    table is cached on device (rebuilt only if any pointer changes, which can
    only happen outside capture) and the step counter is a device int32
    scalar incremented by a captured add — so a replayed training-step graph
    keeps exact Adam bias correction with zero host work.  The table holds
    each tensor's lag behind that counter (0 unless its gradients began
    later than another's), fixed when the table is built.

    The learning rate of a capturable optimizer lives in a device scalar.  An
    eager ``step()`` refreshes it from ``param_groups[0]["lr"]``, so the usual
    scheduler idiom works; between graph replays only :meth:`set_lr` reaches it.
    """

    def __init__(self, params: Iterable[torch.Tensor], lr: float = 1e-3,
                 betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 capturable: bool = False):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        if capturable and len(self.param_groups) > 1:
            raise ValueError("capturable FusedAdam supports a single param group")
        self.capturable = capturable
        self._step_t: torch.Tensor | None = None   # device int32 scalar
        self._lr_t: torch.Tensor | None = None     # device f32 scalar (lr)
        self._lr_host: float | None = None         # value last written to _lr_t
        self._meta: torch.Tensor | None = None     # device int64 pointer table
        self._meta_key = None                      # pointer tuple behind _meta
        self._meta_total = 0
        self._meta_nt = 0
        # parameters in the table and their lags behind _step_t; empty when
        # the host "step" entries are the authority (fresh, or just loaded)
        self._meta_params: List[torch.Tensor] = []
        self._meta_lags: List[int] = []

    def _sync_host_steps(self) -> None:
        """Graph replays advance only the device counter: bring the host
        ``step`` of every tensor in the table up to date (synchronizes)."""
        if self._step_t is None or not self._meta_params:
            return
        counter = int(self._step_t.item())
        for p, lag in zip(self._meta_params, self._meta_lags):
            self.state[p]["step"] = counter - lag

    def _build_table(self, params, grads, m, v, key, host_steps) -> None:
        """``host_steps``: steps taken by each tensor BEFORE this call, as the
        host knows them (exact for a tensor outside the current table)."""
        check_adam_operands(params, grads, m, v)
        dev = params[0].device
        if len(params) == len(self._meta_params) and all(
                a is b for a, b in zip(params, self._meta_params)):
            # the same tensors at new addresses (gradients reallocated by
            # zero_grad(set_to_none=True)): counter and lags stand, and the
            # eager training loop is spared a device synchronization per step
            counter, lags = None, self._meta_lags
        else:
            in_table = {id(p) for p in self._meta_params}
            self._sync_host_steps()
            done = [int(self.state[p]["step"]) if id(p) in in_table else s
                    for p, s in zip(params, host_steps)]
            counter = max(done)
            lags = [counter - d for d in done]
            for p, d in zip(params, done):
                self.state[p]["step"] = d + 1  # this call's step, as in step()
        ptrs = [t.data_ptr() for lst in (params, grads, m, v) for t in lst]
        cum, total = [], 0
        for p in params:
            total += p.numel()
            cum.append(total)
        self._meta = torch.tensor(ptrs + cum + lags, dtype=torch.int64, device=dev)
        if self._step_t is None:
            self._step_t = torch.full((1,), counter, dtype=torch.int32, device=dev)
        elif counter is not None:
            self._step_t.fill_(counter)
        self._meta_key = key
        self._meta_total = total
        self._meta_nt = len(params)
        self._meta_params = list(params)
        self._meta_lags = lags

    def _capturable_step(self, params, grads, m, v, group, host_steps) -> None:
        ext = require_native("fused_adam_step")
        key = tuple(t.data_ptr() for t in params + grads + m + v)
        if self._meta is None or self._meta_key != key:
            self._build_table(params, grads, m, v, key, host_steps)
        lr = float(group["lr"])
        if self._lr_t is None:
            # device-resident lr: captured replays read it, so LR schedules
            # work under hipGraph (set_lr updates it between replays)
            self._lr_t = torch.full((1,), lr, dtype=torch.float32,
                                    device=params[0].device)
            self._lr_host = lr
        elif lr != self._lr_host and not torch.cuda.is_current_stream_capturing():
            # group["lr"] written by a scheduler; a fill_ under capture would
            # be replayed with the capture-time value, so there set_lr rules
            self._lr_t.fill_(lr)
            self._lr_host = lr
        self._step_t += 1  # device add: captured, so replays keep counting
        beta1, beta2 = group["betas"]
        ext.fused_adam_capturable(self._meta, self._meta_nt, self._meta_total,
                                  self._step_t, self._lr_t, beta1, beta2,
                                  group["eps"], group["weight_decay"])

    def set_lr(self, lr: float) -> None:
        """Schedule-safe lr update: refreshes the host groups AND the
        device scalar a captured (replayed) step reads."""
        for group in self.param_groups:
            group["lr"] = lr
        if self._lr_t is not None:
            self._lr_t.fill_(float(lr))
            self._lr_host = float(lr)

    def state_dict(self):
        # graph replays advance only the device counter; sync the host step
        # bookkeeping before checkpointing
        self._sync_host_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        # the loaded host steps and lr are the authority now.  The device
        # scalars are refreshed IN PLACE (a captured graph holds their
        # addresses); the table is rebuilt, lags included, by the next step.
        self._meta_key = None
        self._meta_params, self._meta_lags = [], []
        if self._step_t is not None:
            steps = [int(st["step"]) for st in self.state.values() if "step" in st]
            self._step_t.fill_(max(steps, default=0))
        if self._lr_t is not None:
            self._lr_host = float(self.param_groups[0]["lr"])
            self._lr_t.fill_(self._lr_host)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            params, grads, m, v, steps = [], [], [], [], []
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = 0
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                state["step"] += 1
                params.append(p)
                grads.append(p.grad)
                m.append(state["exp_avg"])
                v.append(state["exp_avg_sq"])
                steps.append(int(state["step"]))
            if not params:
                continue
            if self.capturable and params[0].is_cuda:
                self._capturable_step(params, grads, m, v, group,
                                      [s - 1 for s in steps])
                continue
            beta1, beta2 = group["betas"]
            fused_adam_step(params, grads, m, v, steps, group["lr"], beta1, beta2,
                            group["eps"], group["weight_decay"])
        return loss
