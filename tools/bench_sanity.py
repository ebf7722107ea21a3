#!/usr/bin/env python3
"""One sanity-check request, two routes.

The request: N raw traffic windows (N, T, P) and the measured utilization
(N, T, M), both on the host, at the 256-endpoint model.

- host route (what a client had to do before ``Predictor.sanity_check``):
  ``Predictor.predict`` — the whole (N, T, M, 3) band tensor comes to the
  host — then ``AnomalyScorer.score_all`` per window;
- device route: ``Predictor.sanity_check`` — the model output stays on the
  GPU, one kernel scores it, the (N, M) summaries come back.

Per tier (default 16 and 256; 1024 only if those two together took under
``--budget-s`` seconds, default 120): warm repetitions of each route, median
and min..max wall time (host clock around work that ends in a device
synchronise), the host route split into predict and scoring, bytes copied to
the host and to the device (counted from the shapes), and the kernel alone
(device events around ``ops.band_scores`` on resident tensors) with its
algorithmic bytes.  The two routes' verdicts are compared at every tier.

Run on a GPU host:  python tools/bench_sanity.py [--tiers 16,256,1024]
``--dry-run`` walks the same code on the CPU at a toy size (no timing is
printed as a result: a CPU says nothing about the GPU).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import numpy as np
import torch

from deeprest_amd.data.synthetic import SyntheticApp, SyntheticAppConfig
from deeprest_amd.data.windows import MinMaxScaler
from deeprest_amd.models.net import DeepRestNet, DeepRestNetConfig, build_model_spec
from deeprest_amd.ops import band_scores
from deeprest_amd.serve.anomaly import AnomalyScorer
from deeprest_amd.serve.predictor import Predictor


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--tiers", default="16,256,1024")
    p.add_argument("--window", type=int, default=60)
    p.add_argument("--endpoints", type=int, default=256)
    p.add_argument("--components", type=int, default=64)
    p.add_argument("--reps-host", type=int, default=3)
    p.add_argument("--reps-device", type=int, default=10)
    p.add_argument("--budget-s", type=float, default=120.0,
                   help="tier 1024 runs only if the smaller tiers took less")
    p.add_argument("--threshold", type=float, default=0.25)
    p.add_argument("--min-run", type=int, default=3)
    p.add_argument("--dry-run", action="store_true")
    args = p.parse_args()
    tiers = sorted(int(s) for s in args.tiers.split(","))
    T = args.window

    if args.dry_run:
        dev = torch.device("cpu")
    else:
        assert torch.cuda.is_available(), "bench_sanity.py times the GPU: needs one"
        dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize if dev.type == "cuda" else (lambda: None)

    app = SyntheticApp(SyntheticAppConfig(
        n_apis=args.endpoints, n_components=args.components,
        windows_per_day=240, n_days=1, seed=7))
    data = app.generate_featurized()
    spec = build_model_spec(data)
    P, M = spec.num_paths, spec.num_metrics
    names = list(data.metric_names)
    torch.manual_seed(0)
    model = DeepRestNet(spec, DeepRestNetConfig(dropout=0.0)).to(dev).eval()
    x_scaler = MinMaxScaler().fit(data.traffic.astype(np.float64), 200)
    y_scalers = [MinMaxScaler(min_val=1.0 + (m % 7), max_val=50.0 + 3 * (m % 11))
                 for m in range(M)]
    pred = Predictor(model, x_scaler, y_scalers, names, device=dev,
                     graph_batches=tuple(tiers))
    scorer = AnomalyScorer(threshold=args.threshold, min_run=args.min_run)
    info = {"device": torch.cuda.get_device_name(0) if dev.type == "cuda" else "cpu (dry run)",
            "num_paths": P, "num_metrics": M, "window": T,
            "threshold": args.threshold, "min_run": args.min_run}
    print(json.dumps(info), flush=True)

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        return (time.perf_counter() - t0) * 1000.0, out

    rng = np.random.default_rng(11)
    spent = 0.0
    for N in tiers:
        if N == 1024 and len(tiers) > 1 and spent >= args.budget_s:
            print(json.dumps({"tier": N, "skipped": f"smaller tiers took {spent:.0f} s "
                              f">= {args.budget_s:.0f} s"}), flush=True)
            continue
        t_tier = time.perf_counter()
        x = (rng.random((N, T, P)) * 20.0).astype(np.float32)
        # measured: the model's own median with noise, bursts on some series,
        # a share of gaps (NaN)
        first = pred.predict(x[: min(N, 16)])
        q = np.stack([first[k] for k in names], axis=2)            # (n0, T, M, 3)
        reps = -(-N // q.shape[0])
        q = np.tile(q, (reps, 1, 1, 1))[:N]
        width = q[..., 2] - q[..., 0]
        y = q[..., 1] + width * rng.normal(0.0, 0.3, (N, T, M))
        burst = rng.random((N, 1, M)) < 0.05
        y = y + burst * (np.arange(T)[None, :, None] >= T // 2) * 3.0 * width
        y[rng.random((N, T, M)) < 0.02] = np.nan
        y = y.astype(np.float32)
        del q, width, first

        def host_predict():
            return pred.predict(x)

        def host_score(preds):
            hits = np.zeros((N, M), dtype=bool)
            for i in range(N):
                reports = scorer.score_all(
                    {k: y[i, :, m] for m, k in enumerate(names)},
                    {k: preds[k][i] for k in names})
                hits[i] = [reports[k].is_anomalous for k in names]
            return hits

        def device_route():
            return pred.sanity_check(x, y, threshold=args.threshold,
                                     min_run=args.min_run)

        # warm both (graph capture, code objects, allocator)
        preds = host_predict()
        host_hits = host_score(preds)
        check = device_route()
        agree = int((check.anomalous == host_hits).sum())

        t_pred, t_score = [], []
        for _ in range(args.reps_host):
            ms, preds = timed(host_predict)
            t_pred.append(ms)
            ms, _ = timed(lambda: host_score(preds))
            t_score.append(ms)
        t_host = [a + b for a, b in zip(t_pred, t_score)]
        t_dev = [timed(device_route)[0] for _ in range(args.reps_device)]
        del preds

        # the kernel alone, on resident tensors
        out_d = torch.randn(N, T, M, 3, device=dev)
        y_d = torch.from_numpy(y).to(dev)
        sv = pred._scaler_vectors(dev)
        run_kernel = lambda: band_scores(out_d, y_d, sv[1], sv[0],
                                         threshold=args.threshold,
                                         min_run=args.min_run)
        run_kernel()
        t_kern = []
        if dev.type == "cuda":
            for _ in range(args.reps_device):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run_kernel()
                e1.record()
                e1.synchronize()
                t_kern.append(e0.elapsed_time(e1))
        else:
            t_kern = [timed(run_kernel)[0]]
        del out_d, y_d

        el = N * T * M
        kernel_bytes = el * (12 + 4 + 4 + 1) + N * M * 16       # out, measured; scores, flags; summaries
        med = statistics.median
        res = {
            "tier": N,
            "host_route_ms": {"median": round(med(t_host), 2),
                              "min": round(min(t_host), 2), "max": round(max(t_host), 2),
                              "predict_median": round(med(t_pred), 2),
                              "scoring_median": round(med(t_score), 2),
                              "reps": len(t_host)},
            "device_route_ms": {"median": round(med(t_dev), 2),
                                "min": round(min(t_dev), 2), "max": round(max(t_dev), 2),
                                "reps": len(t_dev)},
            "kernel_ms": {"median": round(med(t_kern), 4), "min": round(min(t_kern), 4),
                          "max": round(max(t_kern), 4), "bytes": kernel_bytes,
                          "GBps_at_median": round(kernel_bytes / med(t_kern) / 1e6, 1)},
            "to_host_bytes": {"host_route": el * 3 * 4, "device_route": N * M * 16},
            "to_device_bytes": {"host_route": N * T * P * 4,
                                "device_route": N * T * P * 4 + el * 4},
            "verdicts_agree": f"{agree}/{N * M}",
            "anomalous_series": int(check.anomalous.sum()),
        }
        if args.dry_run:
            res = {"tier": N, "dry_run": "ok", "verdicts_agree": res["verdicts_agree"],
                   "to_host_bytes": res["to_host_bytes"]}
        print(json.dumps(res), flush=True)
        spent += time.perf_counter() - t_tier


if __name__ == "__main__":
    main()
