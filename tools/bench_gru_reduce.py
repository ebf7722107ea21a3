#!/usr/bin/env python3
"""GRU backward reductions over dpre, single pass against the two-kernel form:
op-level and step-level measurement.

Op level: ext.gru_bwd_reduce on a random dpre (B 2048, T 60, C 64, 4H) bf16 in
``split`` mode (gru_dxg_kernel + gru_dgamma_kernel, dpre read twice) and in
``fused`` mode (gru_reduce_fused_kernel, dpre read once).  Both run in one
process in alternating blocks, timed with device events after a warm-up.
Prints ms, the bytes each form has to move (counted from the shapes) and that
byte count over the time as a share of the 6.29 TB/s copy ceiling.

Step level: training windows/s at bench.py's configuration (same dataset, model
seed, TrainStep and FusedAdam) with ops.gru.REDUCE_MODE = split / fused; the
two alternate and each runs ``--repeats`` times so the spread between repeats
is visible next to the difference between variants.

Needs a GPU: there is no CPU timing.

  python tools/bench_gru_reduce.py [--op-only | --step-only] [--out FILE.md]
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
from deeprest_amd.ops import gru as gru_mod  # noqa: E402
from deeprest_amd.ops.adam import FusedAdam  # noqa: E402
from deeprest_amd.ops.native import require_native  # noqa: E402

H = 128
COPY_CEILING = 6.29e12      # measured float4 copy rate of the MI355X, bytes/s
MODES = ["split", "fused"]


def bytes_moved(B, T, C, mode, itemsize=2):
    """Bytes the reductions have to move, from the shapes: dpre once (fused)
    or 1.75 times (split: dgamma reads all four slices, dxg three), the xg
    row once per reader of it plus its pi image written and read, the dxg
    row written.  gamma and the f32 outputs are negligible."""
    bt = B * T
    dpre = bt * C * 4 * H * itemsize
    xg = bt * 3 * H * itemsize
    staging = 2 * xg                       # pi_permute_rows: read xg, write xg_pi
    if mode == "fused":
        return dpre + staging + xg + xg    # + xg_pi read, dxg written
    return dpre + dpre * 3 // 4 + staging + xg + xg


def bench_op(dev, B, T, C, iters, blocks, warmup):
    ext = require_native("bench_gru_reduce")
    dtype = torch.bfloat16
    torch.manual_seed(0)
    dpre = torch.randn(B, T, C, 4 * H, device=dev, dtype=dtype)
    gamma = (1.0 + 0.1 * torch.randn(C, 3 * H, device=dev)).to(dtype)
    xg = torch.randn(B, T, 3 * H, device=dev).to(dtype)
    for mode in MODES:
        for _ in range(warmup):
            ext.gru_bwd_reduce(dpre, gamma, xg, mode)
    torch.cuda.synchronize()
    times = {m: [] for m in MODES}
    for _ in range(blocks):                     # alternate block by block
        for mode in MODES:
            start = torch.cuda.Event(enable_timing=True)
            stop = torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(iters):
                ext.gru_bwd_reduce(dpre, gamma, xg, mode)
            stop.record()
            stop.synchronize()
            times[mode].append(start.elapsed_time(stop) / iters)
    return [{"mode": m, "ms": sum(t) / len(t), "ms_min": min(t), "ms_max": max(t),
             "iters": iters * blocks, "bytes": bytes_moved(B, T, C, m)}
            for m, t in times.items()]


def bench_step(dev, steps, warmup, repeats):
    args = argparse.Namespace(batch=2048, endpoints=256, components=63, seq_len=60)
    X, y, spec = bench.build_train_tensors(args)
    X = X.to(dev).to(torch.bfloat16)
    y = y.to(dev)
    n, B = X.shape[0], args.batch
    results = {m: [] for m in MODES}
    for _ in range(repeats):
        for mode in MODES:                      # alternate the variants
            gru_mod.REDUCE_MODE = mode
            torch.manual_seed(1234)
            model = DeepRestNet(spec, DeepRestNetConfig(dropout=0.0)).to(dev)
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
            results[mode].append(B * steps / (start.elapsed_time(stop) * 1e-3))
            del model, opt, step
            torch.cuda.empty_cache()
    gru_mod.REDUCE_MODE = "auto"
    return results


def report(op, step, shape):
    B, T, C = shape
    lines = []
    if op is not None:
        lines += [
            f"## Op level: gru_bwd_reduce at (B {B}, T {T}, C {C}) bf16",
            "",
            "Bytes are counted from the shapes (dpre read once or 1.75 times, the "
            "xg image, the dxg row); the share is bytes / time over 6.29 TB/s.",
            "",
            "| mode | ms (mean) | ms (min..max over blocks) | iterations | GB | "
            "TB/s | share of 6.29 TB/s |",
            "|---|---|---|---|---|---|---|",
        ]
        for r in op:
            rate = r["bytes"] / (r["ms"] * 1e-3)
            lines.append(
                f"| {r['mode']} | {r['ms']:.3f} | {r['ms_min']:.3f}..{r['ms_max']:.3f} "
                f"| {r['iters']} | {r['bytes'] / 1e9:.2f} | {rate / 1e12:.2f} | "
                f"{100 * rate / COPY_CEILING:.0f} % |")
        lines.append("")
    if step is not None:
        lines += [
            "## Step level: training windows/s at the bench.py configuration",
            "",
            "| reduce mode | windows/s per repeat | mean | spread |",
            "|---|---|---|---|",
        ]
        for mode, v in step.items():
            lines.append(
                f"| {mode} | {', '.join(f'{x:.0f}' for x in v)} | "
                f"{sum(v) / len(v):.0f} | {max(v) - min(v):.0f} |")
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--seq-len", type=int, default=60)
    ap.add_argument("--components", type=int, default=64)
    ap.add_argument("--iters", type=int, default=5, help="iterations per block")
    ap.add_argument("--blocks", type=int, default=4, help="alternating blocks per mode")
    ap.add_argument("--op-warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--op-only", action="store_true")
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    args = ap.parse_args()

    if not torch.cuda.is_available():
        raise SystemExit("bench_gru_reduce.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    shape = (args.batch, args.seq_len, args.components)
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
