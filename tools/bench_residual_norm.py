#!/usr/bin/env python3
"""Fused dropout+residual+LayerNorm: op-level and step-level measurement.

Op level: at the flagship shape (2048*60 rows x 256, bf16), forward+backward
of the fused op against the eager composition ``layer_norm(x + F.dropout(a))``
(upstream grads on both the residual stream and the normed tensor, as in the
encoder), for p in {0, 0.1}.  Both run in one process in alternating blocks,
timed with device events after a warm-up.  Prints ms, the bytes each variant
has to move (counted from shapes, below) and the achieved bytes/s next to the
6.3 TB/s elementwise ceiling of the MI355X.

Step level: training windows/s at bench.py's configuration (same dataset,
model seed, TrainStep and FusedAdam) for {flag off, flag on} x {dropout 0,
0.1}; the variants alternate and each runs ``--repeats`` times so the spread
between repeats is visible next to the difference between variants.

Needs a GPU: there is no CPU timing.

  python tools/bench_residual_norm.py [--op-only | --step-only] [--out FILE.md]
"""
import argparse
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (sets the TunableOp environment before torch loads)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from deeprest_amd.engine.step import TrainStep  # noqa: E402
from deeprest_amd.models.net import DeepRestNet, DeepRestNetConfig  # noqa: E402
from deeprest_amd.ops import dropout_add_layer_norm, layer_norm  # noqa: E402
from deeprest_amd.ops.adam import FusedAdam  # noqa: E402

HBM_CEILING = 6.3e12   # B/s, elementwise ceiling (guide Appendix B)


def op_bytes_per_element(fused: bool, p: float, itemsize: int = 2) -> dict:
    """Bytes per element each variant must move, from shapes alone.

    fused forward : read branch, residual; write r_out, normed
    fused backward: read d_normed, d_r_out, r_out; write d_residual and, with
                    a mask, d_branch (without one it aliases d_residual)
    eager forward : dropout (read, write, 1 B mask; identity at p == 0),
                    add (2 reads, 1 write), LayerNorm (read, write)
    eager backward: LayerNorm (read dy, x; write dx), grad accumulation on
                    the residual stream (2 reads, 1 write), dropout (read
                    grad and 1 B mask, write; identity at p == 0)
    The f32 per-row statistics and the w/b traffic are left out (< 2%).
    """
    s = itemsize
    if fused:
        fwd = 4 * s
        bwd = 3 * s + s + (s if p > 0 else 0)
    else:
        drop_f = (2 * s + 1) if p > 0 else 0
        drop_b = (2 * s + 1) if p > 0 else 0
        fwd = drop_f + 3 * s + 2 * s
        bwd = 3 * s + 3 * s + drop_b
    return {"fwd": fwd, "bwd": bwd, "total": fwd + bwd}


def bench_op(dev, rows, D, iters, blocks, warmup):
    dtype = torch.bfloat16
    torch.manual_seed(0)
    a = torch.randn(rows, D, device=dev, dtype=dtype, requires_grad=True)
    x = torch.randn(rows, D, device=dev, dtype=dtype, requires_grad=True)
    w = torch.ones(D, device=dev, requires_grad=True)
    b = torch.zeros(D, device=dev, requires_grad=True)
    g_r = torch.randn(rows, D, device=dev, dtype=dtype)
    g_n = torch.randn(rows, D, device=dev, dtype=dtype)

    def fused(p):
        r, n = dropout_add_layer_norm(a, x, w, b, p, True)
        torch.autograd.backward([r, n], [g_r, g_n])

    def eager(p):
        r = x + F.dropout(a, p, True)
        n = layer_norm(r, w, b)
        torch.autograd.backward([r, n], [g_r, g_n])

    def clear():
        for t in (a, x, w, b):
            t.grad = None

    results = []
    for p in (0.0, 0.1):
        variants = {"eager": eager, "fused": fused}
        for fn in variants.values():
            for _ in range(warmup):
                clear()
                fn(p)
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(blocks):                 # alternate block by block
            for name, fn in variants.items():
                start = torch.cuda.Event(enable_timing=True)
                stop = torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(iters):
                    clear()
                    fn(p)
                stop.record()
                stop.synchronize()
                times[name].append(start.elapsed_time(stop) / iters)
        for name in variants:
            t = times[name]
            nbytes = op_bytes_per_element(name == "fused", p)["total"] * rows * D
            mean = sum(t) / len(t)
            results.append({
                "p": p, "variant": name, "ms": mean, "ms_min": min(t),
                "ms_max": max(t), "iters": iters * blocks, "bytes": nbytes,
                "bytes_per_s": nbytes / (mean * 1e-3),
            })
    return results


def bench_step(dev, steps, warmup, repeats):
    args = argparse.Namespace(batch=2048, endpoints=256, components=63, seq_len=60)
    X, y, spec = bench.build_train_tensors(args)
    X = X.to(dev).to(torch.bfloat16)
    y = y.to(dev)
    n, B = X.shape[0], args.batch
    variants = [(fused, p) for p in (0.0, 0.1) for fused in (False, True)]
    results = {v: [] for v in variants}
    for _ in range(repeats):
        for fused, p in variants:               # alternate the variants
            torch.manual_seed(1234)
            model = DeepRestNet(spec, DeepRestNetConfig(
                dropout=p, fused_residual_norm=fused)).to(dev)
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
            results[(fused, p)].append(B * steps / (start.elapsed_time(stop) * 1e-3))
            del model, opt, step
            torch.cuda.empty_cache()
    return results


def report(op, step, rows, D):
    lines = []
    if op is not None:
        lines += [
            f"## Op level: forward+backward, ({rows} x {D}) bf16",
            "",
            f"Ceiling for the last column: {HBM_CEILING / 1e12:.1f} TB/s "
            "(elementwise HBM ceiling). Bytes are counted from shapes.",
            "",
            "| p | variant | ms (mean) | ms (min..max over blocks) | iterations "
            "| MB moved | achieved TB/s | share of ceiling |",
            "|---|---|---|---|---|---|---|---|",
        ]
        for r in op:
            lines.append(
                f"| {r['p']} | {r['variant']} | {r['ms']:.4f} | "
                f"{r['ms_min']:.4f}..{r['ms_max']:.4f} | {r['iters']} | "
                f"{r['bytes'] / 1e6:.1f} | {r['bytes_per_s'] / 1e12:.2f} | "
                f"{100 * r['bytes_per_s'] / HBM_CEILING:.0f}% |")
        lines.append("")
    if step is not None:
        lines += [
            "## Step level: training windows/s at the bench.py configuration",
            "",
            "| dropout | fused_residual_norm | windows/s per repeat | mean | spread |",
            "|---|---|---|---|---|",
        ]
        for (fused, p), v in step.items():
            lines.append(
                f"| {p} | {'on' if fused else 'off'} | "
                f"{', '.join(f'{x:.0f}' for x in v)} | {sum(v) / len(v):.0f} | "
                f"{max(v) - min(v):.0f} |")
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048 * 60)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50, help="iterations per block")
    ap.add_argument("--blocks", type=int, default=4, help="alternating blocks per variant")
    ap.add_argument("--op-warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--op-only", action="store_true")
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    args = ap.parse_args()

    if not torch.cuda.is_available():
        raise SystemExit("bench_residual_norm.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    text = ""
    if not args.step_only:
        op = bench_op(dev, args.rows, args.dim, args.iters, args.blocks, args.op_warmup)
        text += report(op, None, args.rows, args.dim)
        print(text, flush=True)
    if not args.op_only:
        step = bench_step(dev, args.steps, args.warmup, args.repeats)
        text += report(None, step, args.rows, args.dim)
        print(report(None, step, args.rows, args.dim), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
