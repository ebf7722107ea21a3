#!/usr/bin/env python3
"""Serving a mix of window lengths: one graph per (tier, T) against one graph
per tier with ``max_window``.

A fixed stream of requests (default 200, each ``--batch`` windows, T drawn
from ``--lengths``) is served twice through ``Predictor.predict_normalized``:

- ``max_window=None``: every distinct T captures its own graph at first sight
  (two warm-up forwards, one capture, buffers kept);
- ``max_window=max(lengths)``: one graph per tier; shorter windows are padded
  and carry their length.

Reported per predictor: wall time of the first pass (captures included), wall
time of a second pass over the same stream (everything captured), number of
graphs, and device memory held after the first pass (allocator bytes above
the level before the predictor saw a request — graph pools and buffers).
A third figure serves the whole stream as ragged batches (``--ragged`` windows
of mixed T per call), which only the ``max_window`` predictor can do.

Run on a GPU host:  python tools/bench_varlen.py [--requests 200]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import numpy as np
import torch

from deeprest_amd.data.synthetic import SyntheticApp, SyntheticAppConfig
from deeprest_amd.data.windows import MinMaxScaler
from deeprest_amd.models.net import DeepRestNet, DeepRestNetConfig, build_model_spec
from deeprest_amd.serve.predictor import Predictor


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--requests", type=int, default=200)
    p.add_argument("--lengths", default="8,23,60")
    p.add_argument("--batch", type=int, default=16, help="windows per request")
    p.add_argument("--ragged", type=int, default=16,
                   help="windows of mixed T per ragged call")
    p.add_argument("--endpoints", type=int, default=256)
    p.add_argument("--components", type=int, default=64)
    p.add_argument("--fp8", action="store_true")
    args = p.parse_args()
    lengths = [int(s) for s in args.lengths.split(",")]
    W = max(lengths)

    assert torch.cuda.is_available(), "bench_varlen.py measures graph capture: needs a GPU"
    dev = torch.device("cuda:0")
    app = SyntheticApp(SyntheticAppConfig(
        n_apis=args.endpoints, n_components=args.components,
        windows_per_day=240, n_days=1, seed=7))
    data = app.generate_featurized()
    spec = build_model_spec(data)
    torch.manual_seed(0)
    model = DeepRestNet(spec, DeepRestNetConfig(
        dropout=0.0, fp8_inference=args.fp8)).to(dev).eval()
    x_scaler = MinMaxScaler().fit(data.traffic.astype(np.float64), 200)
    y_scalers = [MinMaxScaler() for _ in data.metric_names]

    rng = np.random.default_rng(11)
    req_T = rng.choice(lengths, size=args.requests)
    gen = torch.Generator().manual_seed(5)
    reqs = [torch.rand(args.batch, int(T), spec.num_paths, generator=gen).to(dev)
            for T in req_T]

    def sync_time(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1000.0

    results = {"device": torch.cuda.get_device_name(0), "requests": args.requests,
               "windows_per_request": args.batch, "lengths": lengths,
               "mix": {int(T): int((req_T == T).sum()) for T in lengths},
               "num_paths": spec.num_paths, "components": args.components,
               "fp8": args.fp8}
    tiers = (max(args.batch, args.ragged),)
    for name, mw in (("per_T_graphs", None), ("max_window", W)):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        pred = Predictor(model, x_scaler, y_scalers, data.metric_names, device=dev,
                         graph_batches=tiers, use_graph=True, max_window=mw)

        def serve_all():
            for x in reqs:
                pred.predict_normalized(x)

        first = sync_time(serve_all)
        held = torch.cuda.memory_allocated() - base
        steady = min(sync_time(serve_all) for _ in range(3))
        entry = {"first_pass_ms": round(first, 2),
                 "steady_pass_ms": round(steady, 2),
                 "steady_ms_per_request": round(steady / args.requests, 4),
                 "graphs": len(pred._graphs),
                 "held_bytes_after_first_pass": int(held)}
        if mw is not None:
            # the same windows as ragged batches: one replay per --ragged
            # windows of mixed length
            wins = [x[0] for x in reqs]
            groups = [wins[i:i + args.ragged] for i in range(0, len(wins), args.ragged)]
            lens = [torch.tensor([w.shape[0] for w in g], dtype=torch.int32,
                                 device=dev) for g in groups]
            padded = []
            for g in groups:
                x = torch.zeros(len(g), max(w.shape[0] for w in g),
                                spec.num_paths, device=dev)
                for i, w in enumerate(g):
                    x[i, : w.shape[0]] = w
                padded.append(x)

            def serve_ragged():
                for x, l in zip(padded, lens):
                    pred.predict_normalized(x, l)

            def serve_single():
                for w in wins:
                    pred.predict_normalized(w[None])

            serve_ragged()
            entry["ragged_ms_per_window"] = round(
                min(sync_time(serve_ragged) for _ in range(3)) / len(wins), 4)
            entry["single_ms_per_window"] = round(
                min(sync_time(serve_single) for _ in range(3)) / len(wins), 4)
        results[name] = entry
        print(f"{name}: {json.dumps(entry)}", flush=True)
        del pred
    print(json.dumps(results))


if __name__ == "__main__":
    main()
