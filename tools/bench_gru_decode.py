#!/usr/bin/env python3
"""Quantile-head decode fused into the GRU forward kernel: op-level,
model-level and long-horizon measurement of ``fused_head_decode``.

Op level: one decoder direction without grad at the flagship shape (B 2048,
T 60, C 64, O 9, bf16), forward and reverse.  ``decode`` is
ops.fused_gru_decode (out and h_last, no h_all); ``unfused`` is
fused_gru_sequence (no saves) followed by the head GEMM and the boundary
slice.  Both run in one process in alternating blocks, timed with device
events after a warm-up; the peak allocated memory of one call is taken
separately.  Prints per-block ms, their spread, and the bytes of h_all the
decode form no longer moves (counted from shapes).

Model level: eval windows/s of the flagship model (bench.py's dataset and
model seed, bf16 autocast, no grad) with the flag off/on, alternating,
``--repeats`` times each.

Long horizon: ``forward_long`` steps/s and peak allocated memory over
``--horizon`` steps at batch 1, flag off/on, bf16 and fp8 decode.

"off" is the path of the commit before the flag existed.  Needs a GPU: there
is no CPU timing.

  python tools/bench_gru_decode.py [--only op|model|long] [--out FILE.md]
"""
import argparse
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (sets the TunableOp environment before torch loads)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from deeprest_amd.models.net import DeepRestNet, DeepRestNetConfig  # noqa: E402
from deeprest_amd.ops import fused_gru_decode, fused_gru_sequence  # noqa: E402

H = 128


def h_all_bytes(B, T, C, itemsize=2):
    """The (B, T, C, H) hidden sequence: written once by the GRU kernel and
    read once by the head GEMM in the unfused form; neither in the decode
    form."""
    return 2 * B * T * C * H * itemsize


def _peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del res
    return peak


def bench_op(dev, B, T, C, O, iters, blocks, warmup):
    dtype = torch.bfloat16
    torch.manual_seed(0)
    mk = lambda *s: torch.randn(*s, device=dev) * 0.4
    ins = [
        mk(B, T, 3 * H).to(dtype), (mk(3 * H, H) / H ** 0.5).to(dtype),
        mk(3 * H) * 0.2, mk(B, C, H).to(dtype),
        (1.0 + 0.1 * mk(C, 3 * H)).to(dtype), (0.1 * mk(C, 3 * H)).to(dtype),
        mk(O, H) / H ** 0.5,
    ]
    rows = []
    with torch.no_grad():
        for reverse in (False, True):
            def decode():
                return fused_gru_decode(*ins, reverse=reverse)

            def unfused():
                h_all = fused_gru_sequence(*ins[:6], reverse=reverse)
                out = F.linear(h_all, ins[6].to(h_all.dtype))
                return out, h_all[:, 0 if reverse else -1].contiguous()

            variants = {"unfused": unfused, "decode": decode}
            for fn in variants.values():
                for _ in range(warmup):
                    fn()
            torch.cuda.synchronize()
            # same result, within one bf16 rounding of the output
            a, b = unfused()[0].float(), decode()[0].float()
            max_diff = (a - b).abs().max().item()
            times = {k: [] for k in variants}
            for _ in range(blocks):                 # alternate block by block
                for name, fn in variants.items():
                    start = torch.cuda.Event(enable_timing=True)
                    stop = torch.cuda.Event(enable_timing=True)
                    start.record()
                    for _ in range(iters):
                        fn()
                    stop.record()
                    stop.synchronize()
                    times[name].append(start.elapsed_time(stop) / iters)
            for name, fn in variants.items():
                rows.append({"variant": name, "reverse": reverse,
                             "ms": times[name], "peak": _peak_of(fn),
                             "max_diff": max_diff})
    return rows


def _flagship(dev):
    args = argparse.Namespace(batch=2048, endpoints=256, components=63, seq_len=60)
    X, _, spec = bench.build_train_tensors(args)
    return X[:args.batch].to(dev).to(torch.bfloat16), spec


def _models(spec, dev, fp8=False):
    out = {}
    for flag in (False, True):
        torch.manual_seed(1234)
        out[flag] = DeepRestNet(spec, DeepRestNetConfig(
            dropout=0.0, fused_head_decode=flag, fp8_inference=fp8)).to(dev).eval()
    return out


def bench_model(dev, X, spec, steps, warmup, repeats):
    models = _models(spec, dev)
    results = {flag: [] for flag in models}
    B = X.shape[0]
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        for m in models.values():
            for _ in range(warmup):
                m(X)
        torch.cuda.synchronize()
        for _ in range(repeats):
            for flag, m in models.items():          # alternate the variants
                start = torch.cuda.Event(enable_timing=True)
                stop = torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(steps):
                    out = m(X)
                stop.record()
                stop.synchronize()
                assert torch.isfinite(out).all().item(), "non-finite output"
                results[flag].append(B * steps / (start.elapsed_time(stop) * 1e-3))
    return results


def bench_long(dev, X, spec, horizon, chunk, repeats):
    # one batch-1 horizon built by tiling real windows along time
    T = X.shape[1]
    reps = (horizon + T - 1) // T
    x = X[:reps].reshape(1, reps * T, X.shape[2])[:, :horizon].contiguous()
    rows = []
    for fp8 in (False, True):
        models = _models(spec, dev, fp8=fp8)
        res = {flag: {"steps_s": [], "peak": []} for flag in models}
        with torch.no_grad(), torch.autocast(device_type="cuda",
                                             dtype=torch.bfloat16):
            for m in models.values():               # warm-up: every shape used
                m.forward_long(x[:, :2 * chunk], chunk_size=chunk)
            for _ in range(repeats):
                for flag, m in models.items():
                    torch.cuda.synchronize()
                    torch.cuda.empty_cache()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    t0 = time.perf_counter()
                    out = m.forward_long(x, chunk_size=chunk)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    assert torch.isfinite(out).all().item(), "non-finite output"
                    res[flag]["steps_s"].append(horizon / dt)
                    res[flag]["peak"].append(torch.cuda.max_memory_allocated() - base)
                    del out
        rows.append((fp8, res))
        del models
        torch.cuda.empty_cache()
    return rows


def _spread(v):
    return f"{min(v):.3f}..{max(v):.3f}"


def report_op(rows, shape):
    B, T, C, O = shape
    lines = [
        f"## Op level: one direction, no grad, (B {B}, T {T}, C {C}, O {O}) bf16",
        "",
        f"h_all no longer moved by the decode form: {h_all_bytes(B, T, C) / 1e9:.2f} "
        f"GB per call (one write + one read; counted from shapes).",
        "",
        "| variant | direction | ms per block | mean | min..max | peak allocated MB | max abs diff of out |",
        "|---|---|---|---|---|---|---|",
    ]
    for r in rows:
        ms = r["ms"]
        lines.append(
            f"| {r['variant']} | {'reverse' if r['reverse'] else 'forward'} | "
            f"{', '.join(f'{x:.3f}' for x in ms)} | {sum(ms) / len(ms):.3f} | "
            f"{_spread(ms)} | {r['peak'] / 1e6:.1f} | {r['max_diff']:.3e} |")
    return "\n".join(lines + [""])


def report_model(results):
    lines = [
        "## Model level: eval windows/s, flagship model, bf16 autocast, no grad",
        "",
        "| fused_head_decode | windows/s per repeat | mean | spread |",
        "|---|---|---|---|",
    ]
    for flag, v in results.items():
        lines.append(f"| {'on' if flag else 'off'} | "
                     f"{', '.join(f'{x:.0f}' for x in v)} | {sum(v) / len(v):.0f} | "
                     f"{max(v) - min(v):.0f} |")
    return "\n".join(lines + [""])


def report_long(rows, horizon, chunk):
    lines = [
        f"## Long horizon: forward_long, batch 1, {horizon} steps, chunk {chunk}",
        "",
        "| decode | fused_head_decode | steps/s per repeat | mean | peak allocated MB |",
        "|---|---|---|---|---|",
    ]
    for fp8, res in rows:
        for flag, r in res.items():
            v = r["steps_s"]
            lines.append(
                f"| {'fp8' if fp8 else 'bf16'} | {'on' if flag else 'off'} | "
                f"{', '.join(f'{x:.0f}' for x in v)} | {sum(v) / len(v):.0f} | "
                f"{max(r['peak']) / 1e6:.1f} |")
    return "\n".join(lines + [""])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--seq-len", type=int, default=60)
    ap.add_argument("--components", type=int, default=64)
    ap.add_argument("--out-width", type=int, default=9, help="O = resources x quantiles")
    ap.add_argument("--iters", type=int, default=10, help="iterations per block")
    ap.add_argument("--blocks", type=int, default=5, help="alternating blocks per variant")
    ap.add_argument("--op-warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--horizon", type=int, default=32768)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--only", choices=["op", "model", "long"], default=None)
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    args = ap.parse_args()

    if not torch.cuda.is_available():
        raise SystemExit("bench_gru_decode.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    shape = (args.batch, args.seq_len, args.components, args.out_width)
    parts = []

    def emit(text):
        parts.append(text)
        print(text, flush=True)

    if args.only in (None, "op"):
        emit(report_op(bench_op(dev, *shape, args.iters, args.blocks,
                                args.op_warmup), shape))
    if args.only in (None, "model", "long"):
        X, spec = _flagship(dev)
        if args.only in (None, "model"):
            emit(report_model(bench_model(dev, X, spec, args.steps, args.warmup,
                                          args.repeats)))
        if args.only in (None, "long"):
            emit(report_long(bench_long(dev, X, spec, args.horizon, args.chunk,
                                        args.repeats), args.horizon, args.chunk))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(parts) + "\n")


if __name__ == "__main__":
    main()
