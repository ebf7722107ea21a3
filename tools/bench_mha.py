#!/usr/bin/env python3
"""Attention on the packed qkv projection: op-level measurement.

Forward+backward of ``ops.mha_packed`` at the flagship shape (batch 2048,
T 60, 8 heads of 32, bf16) with ``PACKED_MODE`` "off" (three ``.contiguous()``
views, the (B, H, T, D) op, the transposing reshape, and autograd's view
backward that merges dq, dk, dv) against "auto" (the strided kernels on the
packed tensor).  Both run in one process in alternating blocks, timed with
device events after a warm-up.  Prints ms, the bytes the packed op has to move
(counted from shapes) and its achieved bytes/s next to the 6.29 TB/s copy
ceiling of the MI355X.

Needs a GPU: there is no CPU timing.

  python tools/bench_mha.py [--out FILE.md]
"""
import argparse
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from deeprest_amd.ops import attention, mha_packed  # noqa: E402

COPY_CEILING = 6.29e12   # B/s


def packed_bytes(B, T, H, Dh, itemsize=2):
    """Bytes the packed op must move: forward reads qkv, writes o and lse;
    backward reads qkv, o, dO and lse, writes dqkv."""
    part = B * T * H * Dh * itemsize
    lse = B * H * T * 4
    return {"fwd": 3 * part + part + lse, "bwd": 3 * part + 2 * part + lse + 3 * part}


def bench(dev, B, T, H, Dh, iters, blocks, warmup):
    dtype = torch.bfloat16
    torch.manual_seed(0)
    qkv = (0.7 * torch.randn(B, T, 3 * H * Dh, device=dev)).to(dtype).requires_grad_(True)
    g = (0.7 * torch.randn(B, T, H * Dh, device=dev)).to(dtype)

    def run(mode):
        attention.PACKED_MODE = mode
        qkv.grad = None
        mha_packed(qkv, H).backward(g)

    modes = ("off", "auto")
    try:
        for mode in modes:
            for _ in range(warmup):
                run(mode)
        torch.cuda.synchronize()
        times = {m: [] for m in modes}
        for _ in range(blocks):                 # alternate block by block
            for mode in modes:
                start = torch.cuda.Event(enable_timing=True)
                stop = torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(iters):
                    run(mode)
                stop.record()
                stop.synchronize()
                times[mode].append(start.elapsed_time(stop) / iters)
    finally:
        attention.PACKED_MODE = "auto"
    return times


def report(times, shape, iters):
    B, T, H, Dh = shape
    nbytes = sum(packed_bytes(B, T, H, Dh).values())
    lines = [
        f"## Op level: mha_packed forward+backward, (B, T, H, Dh) = {shape} bf16",
        "",
        f"The packed op must move {nbytes / 1e6:.0f} MB per call (from shapes); "
        f"ceiling {COPY_CEILING / 1e12:.2f} TB/s.",
        "",
        "| PACKED_MODE | ms (mean) | ms (min..max over blocks) | iterations "
        "| TB/s of the packed op's bytes | share of ceiling |",
        "|---|---|---|---|---|---|",
    ]
    for mode, t in times.items():
        mean = sum(t) / len(t)
        rate = nbytes / (mean * 1e-3)
        lines.append(f"| {mode} | {mean:.4f} | {min(t):.4f}..{max(t):.4f} | "
                     f"{iters * len(t)} | {rate / 1e12:.2f} | "
                     f"{100 * rate / COPY_CEILING:.0f}% |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--seq-len", type=int, default=60)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--head-dim", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50, help="iterations per block")
    ap.add_argument("--blocks", type=int, default=4, help="alternating blocks per mode")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()

    if not torch.cuda.is_available():
        raise SystemExit("bench_mha.py measures on the GPU; none found")
    shape = (args.batch, args.seq_len, args.heads, args.head_dim)
    times = bench(torch.device("cuda", 0), *shape, args.iters, args.blocks, args.warmup)
    text = report(times, shape, args.iters)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
