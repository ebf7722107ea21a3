#!/usr/bin/env python3
"""Masked pinball loss (NaN label = not observed): op-level timing against
the dense op, and one accuracy comparison of masked training against dense
training on carried-forward labels.

Op level: forward + backward of ``masked_pinball_loss`` and of
``pinball_loss`` in one process, bf16 outputs of (B, 60, M, 3), f32 labels,
for M = 39, 192 and 12288 (B 2048, reduced for the last M so the tensors
fit), with 0 % and 30 % of the labels missing.  The dense op gets the same
tensors with the holes filled (it cannot take NaN), so both read the same
bytes; the masked op adds its (M,) workspaces and a one-block finalize
launch.  Variants alternate block by block, timed with device events after a
warm-up.  Prints ms per call, the spread, the masked/dense ratio and the
bytes each call moves (counted from shapes).

Accuracy: the 13-endpoint reference config of tools/accuracy_run.py with 30 %
of the labels knocked out in bursts.  Trains twice from the same seed —
masked loss on the NaN labels, dense loss on the same labels carried forward
— and scores both medians against the COMPLETE ground truth on the eval
windows (mean over metrics of the median absolute error, raw units).

Needs a GPU: there is no CPU timing.

  python tools/bench_masked_pinball.py [--only op|accuracy] [--out FILE.md]
"""
import argparse
import copy
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import bench  # noqa: E402,F401  (sets the TunableOp environment before torch loads)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deeprest_amd.ops import masked_pinball_loss, pinball_loss  # noqa: E402

QUANTILES = (0.05, 0.5, 0.95)


def moved_bytes(B, T, M, Q):
    """Per fwd+bwd call: outputs read twice (bf16), labels read twice (f32),
    gradient written once (bf16); the masked op adds its (M,) sums, counts
    and weights."""
    n = B * T * M
    common = 2 * n * Q * 2 + 2 * n * 4 + n * Q * 2
    return common, 4 * M * 4


def bench_op(dev, B, T, M, Q, rate, iters, blocks, warmup):
    gen = torch.Generator().manual_seed(0)
    out = torch.randn(B, T, M, Q, generator=gen).to(torch.bfloat16).to(dev)
    y = torch.rand(B, T, M, generator=gen)
    miss = torch.rand(B, T, M, generator=gen) < rate
    y_dense = y.to(dev)
    y_nan = y.masked_fill(miss, float("nan")).to(dev)
    out.requires_grad_(True)

    def run(fn, labels):
        out.grad = None
        loss = fn(out, labels, QUANTILES)
        loss.backward()
        return loss

    variants = {"dense": lambda: run(pinball_loss, y_dense),
                "masked": lambda: run(masked_pinball_loss, y_nan)}
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    losses = {k: float(fn().detach()) for k, fn in variants.items()}
    times = {k: [] for k in variants}
    for _ in range(blocks):                          # alternate block by block
        for name, fn in variants.items():
            start = torch.cuda.Event(enable_timing=True)
            stop = torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(iters):
                fn()
            stop.record()
            stop.synchronize()
            times[name].append(start.elapsed_time(stop) / iters)
    return times, losses


def report_op(rows):
    lines = [
        "## Op level: forward + backward, bf16 outputs (B, 60, M, 3), f32 labels",
        "",
        "| B | M | missing | dense ms (min..max) | masked ms (min..max) | "
        "masked/dense | MB moved per call | masked extra KB | loss dense / masked |",
        "|---|---|---|---|---|---|---|---|---|",
    ]
    for (B, T, M, Q, rate), (times, losses) in rows:
        d, m = times["dense"], times["masked"]
        common, extra = moved_bytes(B, T, M, Q)
        lines.append(
            f"| {B} | {M} | {int(rate * 100)} % | {np.mean(d):.4f} "
            f"({min(d):.4f}..{max(d):.4f}) | {np.mean(m):.4f} "
            f"({min(m):.4f}..{max(m):.4f}) | {np.mean(m) / np.mean(d):.2f} | "
            f"{common / 1e6:.1f} | {extra / 1e3:.1f} | "
            f"{losses['dense']:.5f} / {losses['masked']:.5f} |")
    return "\n".join(lines + [""])


# ------------------------------------------------------------------ accuracy
def _fill_forward(data):
    from deeprest_amd.data.windows import forward_fill

    for name in data.metric_names:
        data.resources[name] = forward_fill(data.resources[name])
    return data


def _median_error_vs_truth(trainer, truth_raw):
    """Mean over metrics of the median |median-quantile prediction - complete
    ground truth| on the eval windows, raw units."""
    ds = trainer.dataset
    idx = ds.eval_window_indices(trainer.cfg.train.eval_cycles)
    trainer.model.eval()
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16):
        out = trainer.model(ds.X_test[idx].to(trainer.device))
    out = np.maximum(out.float().cpu().numpy(), 1e-6)
    mq = len(trainer.model.cfg.quantiles) // 2
    truth = truth_raw[ds.split:][idx]
    meds = []
    for m in range(len(ds.metric_names)):
        pred = ds.denormalize_metric(out[:, :, m, mq], m)
        meds.append(float(np.median(np.abs(pred - truth[:, :, m]))))
    return float(np.mean(meds))


def accuracy_run(dev, epochs, rate, mean_gap, seed):
    from deeprest_amd.data.synthetic import (SyntheticApp, SyntheticAppConfig,
                                             inject_missing)
    from deeprest_amd.engine.config import DataConfig, EngineConfig, TrainConfig
    from deeprest_amd.engine.dataset import EstimationDataset
    from deeprest_amd.engine.trainer import Trainer
    from deeprest_amd.models.net import DeepRestNetConfig

    app = SyntheticApp(SyntheticAppConfig(
        n_apis=13, n_components=12, windows_per_day=240, n_days=8,
        resource_noise=0.03, seed=77))
    clean = app.generate_featurized()
    truth_raw = EstimationDataset(clean, step_size=60, split_fraction=0.40).y_raw
    gappy = inject_missing(copy.deepcopy(clean), rate, mean_gap, seed)
    share = float(np.mean([np.isnan(gappy.resources[n]).mean()
                           for n in gappy.metric_names]))
    carried = _fill_forward(copy.deepcopy(gappy))

    def cfg():
        return EngineConfig(
            data=DataConfig(step_size=60, split=0.40),
            train=TrainConfig(epochs=epochs, batch_size=32, lr=1e-3, eval_cycles=9,
                              log_every=0, eval_every=epochs, graph_step=True,
                              run_baselines=False),
            model=DeepRestNetConfig(dropout=0.1))

    res = {"missing_share": share, "epochs": epochs}
    for name, data in (("clean (dense loss)", clean), ("masked on NaN labels", gappy),
                       ("dense on carried-forward labels", carried)):
        torch.manual_seed(1234)
        tr = Trainer(data, cfg(), device=dev)
        assert tr.dataset.has_missing == (data is gappy)
        result = tr.train()
        assert np.isfinite(result.train_losses).all(), name
        res[name] = _median_error_vs_truth(tr, truth_raw)
    return res


def report_accuracy(res):
    lines = [
        "## Accuracy: 13 endpoints, 12 components, 8 days, split 0.40, window 60, "
        f"{res['epochs']} epochs",
        "",
        f"Labels missing in bursts: {res['missing_share'] * 100:.1f} % of all samples. "
        "Score: mean over metrics of the median absolute error of the median "
        "quantile against the COMPLETE ground truth on the eval windows.",
        "",
        "| training | mean median abs error |",
        "|---|---|",
    ]
    for k, v in res.items():
        if k not in ("missing_share", "epochs"):
            lines.append(f"| {k} | {v:.4f} |")
    return "\n".join(lines + [""])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--seq-len", type=int, default=60)
    ap.add_argument("--metrics", type=int, nargs="+", default=[39, 192, 12288])
    ap.add_argument("--big-batch", type=int, default=64,
                    help="batch for M >= 4096 (the tensors of B 2048 do not fit)")
    ap.add_argument("--rates", type=float, nargs="+", default=[0.0, 0.3])
    ap.add_argument("--iters", type=int, default=20, help="calls per block")
    ap.add_argument("--blocks", type=int, default=5, help="alternating blocks per variant")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--mean-gap", type=float, default=20.0)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--only", choices=["op", "accuracy"], default=None)
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    args = ap.parse_args()

    if not torch.cuda.is_available():
        raise SystemExit("bench_masked_pinball.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    parts = []

    def emit(text):
        parts.append(text)
        print(text, flush=True)

    if args.only in (None, "op"):
        rows = []
        for M in args.metrics:
            B = args.batch if M < 4096 else args.big_batch
            for rate in args.rates:
                shape = (B, args.seq_len, M, len(QUANTILES))
                rows.append((shape + (rate,),
                             bench_op(dev, *shape, rate, args.iters, args.blocks,
                                      args.warmup)))
                torch.cuda.empty_cache()
        emit(report_op(rows))
    if args.only in (None, "accuracy"):
        emit(report_accuracy(accuracy_run(dev, args.epochs, 0.3, args.mean_gap,
                                          args.seed)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(parts) + "\n")


if __name__ == "__main__":
    main()
