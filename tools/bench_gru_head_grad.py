#!/usr/bin/env python3
"""Head input gradient fused into the GRU backward: op-level and step-level
measurement.

Op level: one decoder direction, forward+backward, at the flagship shape
(B 2048, T 60, C 64, O 9, bf16).  ``fused`` is ops.fused_gru_heads (the
backward kernel takes the O-wide head gradient); ``unfused`` is
fused_gru_sequence followed by bigk_linear, whose backward writes the
(B, T, C, H) head input gradient for the kernel to read back.  Both run in one
process in alternating blocks, timed with device events after a warm-up.
Prints ms and the bytes of that intermediate the fused form no longer moves
(counted from shapes).

Step level: training windows/s at bench.py's configuration (same dataset,
model seed, TrainStep and FusedAdam) with ``fused_head_grad`` off/on; the two
alternate and each runs ``--repeats`` times so the spread between repeats is
visible next to the difference between variants.

Needs a GPU: there is no CPU timing.

  python tools/bench_gru_head_grad.py [--op-only | --step-only] [--out FILE.md]
"""
import argparse
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (sets the TunableOp environment before torch loads)

import torch  # noqa: E402

from deeprest_amd.engine.step import TrainStep  # noqa: E402
from deeprest_amd.models.net import DeepRestNet, DeepRestNetConfig  # noqa: E402
from deeprest_amd.ops import fused_gru_heads, fused_gru_sequence  # noqa: E402
from deeprest_amd.ops.adam import FusedAdam  # noqa: E402
from deeprest_amd.ops.linear_bigk import bigk_linear  # noqa: E402

H = 128


def bytes_removed(B, T, C, itemsize=2):
    """The (B, T, C, H) head input gradient: written once by the dx GEMM and
    read once by the backward kernel in the unfused form; neither happens in
    the fused form (it reads the (B, T, C, O) head gradient instead, which
    the unfused dx GEMM read as well)."""
    return 2 * B * T * C * H * itemsize


def bench_op(dev, B, T, C, O, iters, blocks, warmup):
    dtype = torch.bfloat16
    torch.manual_seed(0)
    mk = lambda *s: torch.randn(*s, device=dev) * 0.4
    leaves = [
        mk(B, T, 3 * H).to(dtype), (mk(3 * H, H) / H ** 0.5).to(dtype),
        mk(3 * H) * 0.2, mk(B, C, H).to(dtype),
        (1.0 + 0.1 * mk(C, 3 * H)).to(dtype), (0.1 * mk(C, 3 * H)).to(dtype),
        mk(O, H) / H ** 0.5,
    ]
    for t in leaves:
        t.requires_grad_(True)
    grad = torch.randn(B, T, C, O, device=dev).to(dtype)

    def fused():
        fused_gru_heads(*leaves).backward(grad)

    def unfused():
        h_all = fused_gru_sequence(*leaves[:6])
        bigk_linear(h_all, leaves[6]).backward(grad)

    def clear():
        for t in leaves:
            t.grad = None

    variants = {"unfused": unfused, "fused": fused}
    for fn in variants.values():
        for _ in range(warmup):
            clear()
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(blocks):                     # alternate block by block
        for name, fn in variants.items():
            start = torch.cuda.Event(enable_timing=True)
            stop = torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(iters):
                clear()
                fn()
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop) / iters)
    return [{"variant": k, "ms": sum(t) / len(t), "ms_min": min(t),
             "ms_max": max(t), "iters": iters * blocks} for k, t in times.items()]


def bench_step(dev, steps, warmup, repeats):
    args = argparse.Namespace(batch=2048, endpoints=256, components=63, seq_len=60)
    X, y, spec = bench.build_train_tensors(args)
    X = X.to(dev).to(torch.bfloat16)
    y = y.to(dev)
    n, B = X.shape[0], args.batch
    variants = [False, True]
    results = {v: [] for v in variants}
    for _ in range(repeats):
        for fused in variants:                  # alternate the variants
            torch.manual_seed(1234)
            model = DeepRestNet(spec, DeepRestNetConfig(
                dropout=0.0, fused_head_grad=fused)).to(dev)
            opt = FusedAdam(model.parameters(), lr=1e-3, capturable=True)
            step = TrainStep(model, opt, autocast_dtype=torch.bfloat16)

            def run(i):
                s = (i * B) % max(n - B, 1)
                return step(X[s:s + B], y[s:s + B])

            for i in range(warmup):
                run(i)
            torch.cuda.synchronize()
            start = torch.cuda.Event(enable_timing=True)
            stop = torch.cuda.Event(enable_timing=True)
            start.record()
            for i in range(steps):
                loss = run(warmup + i)
            stop.record()
            stop.synchronize()
            assert torch.isfinite(loss).item(), "non-finite loss"
            results[fused].append(B * steps / (start.elapsed_time(stop) * 1e-3))
            del model, opt, step
            torch.cuda.empty_cache()
    return results


def report(op, step, shape):
    B, T, C, O = shape
    lines = []
    if op is not None:
        lines += [
            f"## Op level: one direction forward+backward, (B {B}, T {T}, C {C}, "
            f"O {O}) bf16",
            "",
            f"Intermediate no longer moved by the fused form: "
            f"{bytes_removed(B, T, C) / 1e9:.2f} GB per call (one write + one "
            f"read of the (B, T, C, H) head input gradient; counted from shapes).",
            "",
            "| variant | ms (mean) | ms (min..max over blocks) | iterations |",
            "|---|---|---|---|",
        ]
        for r in op:
            lines.append(f"| {r['variant']} | {r['ms']:.3f} | "
                         f"{r['ms_min']:.3f}..{r['ms_max']:.3f} | {r['iters']} |")
        lines.append("")
    if step is not None:
        lines += [
            "## Step level: training windows/s at the bench.py configuration",
            "",
            "| fused_head_grad | windows/s per repeat | mean | spread |",
            "|---|---|---|---|",
        ]
        for fused, v in step.items():
            lines.append(
                f"| {'on' if fused else 'off'} | "
                f"{', '.join(f'{x:.0f}' for x in v)} | {sum(v) / len(v):.0f} | "
                f"{max(v) - min(v):.0f} |")
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--seq-len", type=int, default=60)
    ap.add_argument("--components", type=int, default=64)
    ap.add_argument("--out-width", type=int, default=9, help="O = resources x quantiles")
    ap.add_argument("--iters", type=int, default=5, help="iterations per block")
    ap.add_argument("--blocks", type=int, default=4, help="alternating blocks per variant")
    ap.add_argument("--op-warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--op-only", action="store_true")
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    args = ap.parse_args()

    if not torch.cuda.is_available():
        raise SystemExit("bench_gru_head_grad.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    shape = (args.batch, args.seq_len, args.components, args.out_width)
    text = ""
    if not args.step_only:
        op = bench_op(dev, *shape, args.iters, args.blocks, args.op_warmup)
        text += report(op, None, shape)
        print(text, flush=True)
    if not args.op_only:
        step = bench_step(dev, args.steps, args.warmup, args.repeats)
        text += report(None, step, shape)
        print(report(None, step, shape), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
