"""Online prediction path.

Loads a checkpoint (weights + spec + fitted scalers + call-path feature
space M — everything inference needs) and serves
batched quantile predictions.  On GPU the forward is captured once into a
hipGraph (torch.cuda.CUDAGraph IS hipGraph on ROCm) per configured batch
size; every request is served by replays of the smallest graph that fits —
one graph launch instead of hundreds of kernel launches per request (north
star: "the online prediction step is hipGraph-captured", BASELINE config 3:
batched 1k-window inference).

Staging-buffer ingestion: requests are copied straight into the captured
graph's fixed input buffer (H2D for numpy requests, D2D for resident
tensors) — no intermediate device tensor, so bulk 1k-window inference is a
single copy + one replay, which beats the eager path (round 1's single
64-window graph lost at bulk sizes because 1k windows took 16 chunked
replays; measured in profiles/r02_serve_p50.md).

Variable-length windows (``max_window``): without it every distinct window
length T captures its own graph per batch tier.  With ``max_window=W`` there
is ONE graph per tier, captured over a ``(tier, W, P)`` input buffer and a
``(tier,)`` int32 lengths buffer the model reads on the device; a request of
any T <= W — or a ragged mix of lengths — is copied into the buffer's
``[:n, :T]`` corner, its lengths are written, and the same graph replays.
Padded positions come back as NaN.  Measured in profiles/r06_varlen.md.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .anomaly import AnomalyReport, flag_intervals

from ..data.featurize import FeatureSpace
from ..data.windows import MinMaxScaler
from ..engine.checkpoint import load_checkpoint
from ..models.net import DeepRestNet

DEFAULT_GRAPH_BATCHES = (16, 256, 1024)


@dataclass
class SanityCheck:
    """What ``Predictor.sanity_check`` found, per window n and metric m.  The
    (N, M) summaries are host arrays; ``check[metric]`` gives one metric's
    ``(N,)`` columns.  ``scores`` / ``flags`` (N, T, M) and ``bands``
    (N, T, M, 3) are device tensors, present with ``detail=True`` only."""

    metric_names: List[str]
    threshold: float
    min_run: int
    max_score: np.ndarray             # (N, M) f32, over observed samples
    n_flagged: np.ndarray             # (N, M) int32
    first_flag: np.ndarray            # (N, M) int32, -1: nothing flagged
    n_observed: np.ndarray            # (N, M) int32
    scores: Optional[torch.Tensor] = None
    flags: Optional[torch.Tensor] = None
    bands: Optional[torch.Tensor] = None
    lengths: Optional[torch.Tensor] = None    # (N,) int32 as given, or None

    @property
    def anomalous(self) -> np.ndarray:
        """(N, M) bool: anything flagged."""
        return self.n_flagged > 0

    def keys(self) -> List[str]:
        return list(self.metric_names)

    def __getitem__(self, metric: str) -> Dict[str, np.ndarray]:
        m = self.metric_names.index(metric)
        return {"anomalous": self.n_flagged[:, m] > 0,
                "max_score": self.max_score[:, m],
                "n_flagged": self.n_flagged[:, m],
                "first_flag": self.first_flag[:, m],
                "n_observed": self.n_observed[:, m]}

    def items(self):
        return [(name, self[name]) for name in self.metric_names]

    def reports(self, i: int) -> Dict[str, AnomalyReport]:
        """Window i as ``AnomalyScorer.score_all`` would report it (its own
        length with ``lengths``); the interval lists are built here, on the
        host, from the flags."""
        if self.flags is None:
            raise ValueError("reports() needs sanity_check(..., detail=True)")
        T = self.flags.shape[1]
        L = T if self.lengths is None else min(max(int(self.lengths[i]), 1), T)
        scores = self.scores[i, :L].cpu().numpy()
        flags = self.flags[i, :L].cpu().numpy().astype(bool)
        return {name: AnomalyReport(metric=name, scores=scores[:, m],
                                    flags=flags[:, m],
                                    windows=flag_intervals(flags[:, m]))
                for m, name in enumerate(self.metric_names)}


class Predictor:
    def __init__(
        self,
        model: DeepRestNet,
        x_scaler: MinMaxScaler,
        y_scalers: List[MinMaxScaler],
        metric_names: List[str],
        feature_space: Optional[FeatureSpace] = None,
        device: Optional[torch.device] = None,
        graph_batch: Optional[int] = None,
        graph_batches: Optional[Sequence[int]] = None,
        use_graph: bool = True,
        target_transform: str = "none",
        residual_ridge: Optional[np.ndarray] = None,   # (P+1, M): the net's
        # outputs are residuals over this ridge (train.residual_base)
        conformal: Optional[np.ndarray] = None,        # (M,) CQR band widening
        max_window: Optional[int] = None,     # serve any T <= max_window (and
        # ragged batches) from one graph per tier; None: one graph per (tier, T)
    ) -> None:
        if max_window is not None and int(max_window) < 1:
            raise ValueError(f"max_window must be >= 1, got {max_window}")
        self.max_window = int(max_window) if max_window is not None else None
        self.target_transform = target_transform
        self.residual_ridge = (np.asarray(residual_ridge)
                               if residual_ridge is not None else None)
        self.conformal = (np.asarray(conformal)
                          if conformal is not None else None)
        self._ridge_t: Optional[torch.Tensor] = None    # device caches
        self._conformal_t: Optional[torch.Tensor] = None
        self._scaler_t: Optional[torch.Tensor] = None
        self.device = device or torch.device(
            "cuda" if torch.cuda.is_available() else "cpu"
        )
        self.model = model.to(self.device).eval()
        self.x_scaler = x_scaler
        self.y_scalers = y_scalers
        self.metric_names = metric_names
        self.feature_space = feature_space
        if graph_batches is None:
            graph_batches = (graph_batch,) if graph_batch else DEFAULT_GRAPH_BATCHES
        self.graph_batches: Tuple[int, ...] = tuple(sorted(set(graph_batches)))
        self.use_graph = use_graph and self.device.type == "cuda"
        # (batch, T) -> (graph, input buffer, output buffer, lengths buffer);
        # with max_window the key is (batch, max_window) and the lengths
        # buffer is the (batch,) int32 tensor the captured forward reads,
        # otherwise it is None
        self._graphs: Dict[Tuple[int, int], tuple] = {}

    @staticmethod
    def from_checkpoint(path: str, device: Optional[torch.device] = None,
                        **kw) -> "Predictor":
        state = load_checkpoint(path)
        model = DeepRestNet.from_full_state(state["model"])
        sc = state["scalers"]
        x_scaler = MinMaxScaler.from_state_dict(sc["x_scaler"])
        y_scalers = [MinMaxScaler.from_state_dict(s) for s in sc["y_scalers"]]
        fs = (FeatureSpace.from_state_dict(state["feature_space"])
              if state.get("feature_space") else None)
        kw.setdefault("target_transform", sc.get("target_transform", "none"))
        kw.setdefault("residual_ridge",
                      (state.get("extra") or {}).get("residual_ridge"))
        kw.setdefault("conformal", (state.get("extra") or {}).get("conformal"))
        return Predictor(model, x_scaler, y_scalers, sc["metric_names"],
                         feature_space=fs, device=device, **kw)

    @property
    def captured_batches(self) -> List[int]:
        return sorted({b for (b, _t) in self._graphs})

    # ---------------------------------------------------------------- capture
    def _tier(self, n: int) -> int:
        """Smallest configured graph batch >= n."""
        for bb in self.graph_batches:
            if bb >= n:
                return bb
        raise ValueError(
            f"batch of {n} windows exceeds the largest configured graph "
            f"batch {self.graph_batches[-1]}")

    def _check_window(self, T: int) -> None:
        if self.max_window is not None and T > self.max_window:
            raise ValueError(
                f"window length {T} exceeds max_window {self.max_window}")

    def _graph_for(self, n: int, T: int, P: int) -> tuple:
        """Graph of the smallest configured batch >= n: for windows of length
        T, or — with max_window — the one graph of that tier, which serves
        every T <= max_window."""
        b = self._tier(n)
        self._check_window(T)
        varlen = self.max_window is not None
        key = (b, self.max_window if varlen else T)
        got = self._graphs.get(key)
        if got is not None:
            return got
        gin = torch.zeros(b, key[1], P, device=self.device)
        glen = (torch.ones(b, dtype=torch.int32, device=self.device)
                if varlen else None)
        run = (lambda: self.model(gin, glen)) if varlen else (
            lambda: self.model(gin))
        # warmup on a side stream (required before capture)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                with torch.no_grad():
                    run()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            with torch.no_grad():
                gout = run()
        got = (g, gin, gout, glen)
        self._graphs[key] = got
        return got

    # ----------------------------------------------------- staged ingestion
    def staging_buffer(self, n: int, T: int, P: int) -> torch.Tensor:
        """A writable (n, T, P) view of the captured graph's input buffer.

        Streamed ingestion writes normalized windows directly here (no
        intermediate tensor), then calls ``predict_staged(n)`` — the
        whole-request cost is one replay."""
        _, gin, _, _ = self._graph_for(n, T, P)
        return gin[:n, :T]

    @torch.no_grad()
    def predict_staged(self, n: int, T: int) -> torch.Tensor:
        """Replay the graph whose staging buffer was filled with n windows."""
        b = self._tier(n)
        self._check_window(T)
        g, gin, gout, glen = self._graphs[
            (b, T if self.max_window is None else self.max_window)]
        if n < b:
            gin[n:].zero_()
        if glen is not None:
            glen[:n].fill_(T)
            glen[n:].fill_(1)
        g.replay()
        return gout[:n, :T]

    # ---------------------------------------------------------------- predict
    @torch.no_grad()
    def predict_normalized(self, x: torch.Tensor,
                           lengths: Optional[torch.Tensor] = None
                           ) -> torch.Tensor:
        """x: (N, T, P) normalized traffic -> (N, T, M, Q).

        Requests up to the largest configured graph batch are one padded
        replay; larger requests chunk at the largest batch (a 4096-window
        request = four 1024-replays).  CPU inputs are copied H2D straight
        into the staging buffer.

        With ``max_window``: ``lengths`` (N,) gives each window's own length
        (default: all T); the output is exact zero at padded positions.  The
        lengths travel to the model as a device tensor and are never read
        back on the host."""
        x = x.float()
        N, T, P = x.shape
        if self.max_window is None:
            if lengths is not None:
                raise ValueError("lengths need a Predictor built with max_window")
            if not self.use_graph:
                return self.model(x.to(self.device))
        else:
            self._check_window(T)
            if lengths is None:
                lengths = torch.full((N,), T, dtype=torch.int32,
                                     device=self.device)
            else:
                lengths = torch.as_tensor(lengths).to(
                    device=self.device, dtype=torch.int32).reshape(-1)
                if lengths.shape[0] != N:
                    raise ValueError(
                        f"lengths must have {N} entries, got {lengths.shape[0]}")
            if not self.use_graph:
                return self.model(x.to(self.device), lengths)
        bmax = self.graph_batches[-1]
        outs = []
        s = 0
        while s < N:
            n = min(N - s, bmax)
            g, gin, gout, glen = self._graph_for(n, T, P)
            gin[:n, :T].copy_(x[s : s + n])
            if n < gin.shape[0]:
                gin[n:].zero_()
            if glen is not None:
                glen[:n].copy_(lengths[s : s + n])
                glen[n:].fill_(1)
            g.replay()
            outs.append(gout[:n, :T].clone())
            s += n
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)

    def predict(self, traffic_windows: np.ndarray) -> Dict[str, np.ndarray]:
        """Raw call-path count windows (N, T, P) -> per-metric denormalized
        quantile predictions {metric: (N, T, Q)}.

        The whole request pipeline (normalization, residual base, quantile
        sort, conformal widening) runs on-device in f32: the former f64
        numpy normalization alone cost ~50 ms per 16-window request at the
        256-endpoint width and GIL-serialized concurrent serving."""
        x = np.ascontiguousarray(np.asarray(traffic_windows),
                                 dtype=np.float32)
        return self.predict_tensor(torch.from_numpy(x).to(self.device))

    def _ridge_base(self, xt: torch.Tensor, device: torch.device) -> torch.Tensor:
        """The ridge residual base (N, T, M) of normalized traffic xt
        (N, T, P): one GEMM against the cached device copy of the ridge."""
        if self._ridge_t is None or self._ridge_t.device != device:
            self._ridge_t = torch.from_numpy(np.asarray(
                self.residual_ridge, dtype=np.float32)).to(device)
        N, T, P = xt.shape
        base = xt.reshape(-1, P) @ self._ridge_t[:P] + self._ridge_t[P]
        return base.reshape(N, T, -1)

    @torch.no_grad()
    def predict_tensor(self, xt: torch.Tensor,
                       lengths: Optional[torch.Tensor] = None
                       ) -> Dict[str, np.ndarray]:
        """Raw count windows already on device as f32 (N, T, P) — the
        zero-extra-copy entry the micro-batcher uses (client threads do
        their own H2D, the batch concatenates on device).

        ``lengths`` (N,), with ``max_window`` only: window i is
        ``xt[i, :lengths[i]]``; the returned arrays are NaN at its padded
        positions (a denormalized zero would look like a prediction)."""
        if lengths is not None:
            lengths = torch.as_tensor(lengths).to(
                device=xt.device, dtype=torch.int32).reshape(-1)
        if self.x_scaler.scale != 0.0:
            xt = (xt - self.x_scaler.min_val) * (1.0 / self.x_scaler.scale)
        out = self.predict_normalized(xt, lengths).float()
        if self.residual_ridge is not None:
            out = out + self._ridge_base(xt, out.device).unsqueeze(-1)
        # quantile regression can emit crossed quantiles (q95 < q50) early in
        # training; serving consumers (anomaly bands, demo plots) assume a
        # monotone triple, so sort the Q axis — a no-op once calibrated
        out, _ = torch.sort(out, dim=-1)
        if self.conformal is not None:
            # split-conformal band widening fitted at train time (CQR);
            # negative scores shrink the band — clamp at the median so the
            # served triple stays monotone (clamping a shrink only raises
            # coverage, the guarantee direction)
            if (self._conformal_t is None
                    or self._conformal_t.device != out.device):
                self._conformal_t = torch.from_numpy(np.asarray(
                    self.conformal, dtype=np.float32)).to(out.device)
            c = self._conformal_t
            out[..., 0] = torch.minimum(out[..., 0] - c, out[..., 1])
            out[..., -1] = torch.maximum(out[..., -1] + c, out[..., -2])
        pad = None
        if lengths is not None:
            T = out.shape[1]
            pad = (torch.arange(T, device=out.device)[None, :]
                   >= lengths.to(out.device).clamp(1, T)[:, None]).cpu().numpy()
        out = out.cpu().numpy()                     # (N, T, M, Q)
        preds = {}
        for m, name in enumerate(self.metric_names):
            v = self.y_scalers[m].inverse_transform(out[:, :, m, :])
            if self.target_transform == "log1p":
                v = np.expm1(v)
            v = np.maximum(v, 1e-6)
            if pad is not None:
                v = np.array(v, dtype=np.result_type(v.dtype, np.float32))
                v[pad] = np.nan
            preds[name] = v
        return preds

    def predict_ragged(self, windows: Sequence[np.ndarray]
                       ) -> List[Dict[str, np.ndarray]]:
        """Windows of different lengths, each (T_i, P) raw call-path counts,
        served as one padded batch -> one ``{metric: (T_i, Q)}`` per window.
        Needs ``max_window`` (every T_i <= max_window)."""
        if self.max_window is None:
            raise ValueError("predict_ragged needs a Predictor built with max_window")
        if len(windows) == 0:
            return []
        arrs = [np.asarray(w, dtype=np.float32) for w in windows]
        lens = [int(a.shape[0]) for a in arrs]
        for a in arrs:
            if a.ndim != 2 or a.shape[1] != arrs[0].shape[1] or a.shape[0] < 1:
                raise ValueError("each window must be (T_i >= 1, P) with one P")
        T = max(lens)
        self._check_window(T)
        x = np.zeros((len(arrs), T, arrs[0].shape[1]), dtype=np.float32)
        for i, a in enumerate(arrs):
            x[i, : lens[i]] = a
        out = self.predict_tensor(
            torch.from_numpy(x).to(self.device),
            torch.tensor(lens, dtype=torch.int32, device=self.device))
        return [{k: v[i, : lens[i]] for k, v in out.items()}
                for i in range(len(arrs))]

    # ----------------------------------------------------------- sanity check
    def _scaler_vectors(self, device: torch.device) -> torch.Tensor:
        """(2, M) f32 on the device: row 0 the per-metric scale, row 1 the
        min.  A scaler whose scale is 0 leaves its metric alone
        (``MinMaxScaler.inverse_transform``): scale 1, min 0."""
        if self._scaler_t is None or self._scaler_t.device != device:
            live = [s.scale != 0.0 for s in self.y_scalers]
            v = np.array([[s.scale if ok else 1.0 for s, ok in zip(self.y_scalers, live)],
                          [s.min_val if ok else 0.0 for s, ok in zip(self.y_scalers, live)]],
                         dtype=np.float32)
            self._scaler_t = torch.from_numpy(v).to(device)
        return self._scaler_t

    def _measured_tensor(self, measured, N: int, T: int) -> torch.Tensor:
        M = len(self.metric_names)
        if isinstance(measured, dict):
            unknown = sorted(set(measured) - set(self.metric_names))
            if unknown:
                raise ValueError(f"measured names unknown metrics: {unknown}")
            arr = np.full((N, T, M), np.nan, dtype=np.float32)
            for m, name in enumerate(self.metric_names):
                if name in measured:
                    a = np.asarray(measured[name], dtype=np.float32)
                    if a.shape != (N, T):
                        raise ValueError(
                            f"measured[{name!r}] must be {(N, T)}, got {a.shape}")
                    arr[:, :, m] = a
            return torch.from_numpy(arr).to(self.device)
        if isinstance(measured, torch.Tensor):
            y = measured.to(device=self.device, dtype=torch.float32)
        else:
            y = torch.from_numpy(np.ascontiguousarray(
                np.asarray(measured), dtype=np.float32)).to(self.device)
        if tuple(y.shape) != (N, T, M):
            raise ValueError(
                f"measured must be {(N, T, M)} in metric_names order, "
                f"got {tuple(y.shape)}")
        return y.contiguous()

    @torch.no_grad()
    def sanity_check(self, traffic_windows, measured, threshold: float = 0.25,
                     min_run: int = 3, lengths=None,
                     detail: bool = False) -> "SanityCheck":
        """Is the measured utilization justified by the traffic?  Raw count
        windows (N, T, P) and ``measured`` — an (N, T, M) array in
        ``metric_names`` order or ``{metric: (N, T)}``, a metric left out being
        entirely unobserved, a non-finite value "not observed" — are scored
        against the model's own band without the band leaving the device: the
        pipeline of ``predict_tensor`` up to the normalized output (graph
        replay, ``lengths`` / ``max_window`` as there, the ridge GEMM), then
        ``ops.band_scores``.  Only the (N, M) summaries are copied to the
        host; with ``detail`` the result also holds scores, flags and bands
        (device tensors) and ``reports(i)``."""
        from ..ops.sanity import band_scores

        if int(min_run) < 1:
            raise ValueError(f"min_run must be >= 1, got {min_run}")
        if isinstance(traffic_windows, torch.Tensor):
            xt = traffic_windows.to(device=self.device, dtype=torch.float32)
        else:
            xt = torch.from_numpy(np.ascontiguousarray(
                np.asarray(traffic_windows), dtype=np.float32)).to(self.device)
        if xt.dim() != 3:
            raise ValueError(f"traffic windows must be (N, T, P), got {tuple(xt.shape)}")
        N, T, _ = xt.shape
        y = self._measured_tensor(measured, N, T)
        if lengths is not None:
            lengths = torch.as_tensor(lengths).to(
                device=self.device, dtype=torch.int32).reshape(-1)
        if self.x_scaler.scale != 0.0:
            xt = (xt - self.x_scaler.min_val) * (1.0 / self.x_scaler.scale)
        out = self.predict_normalized(xt, lengths)
        if out.dtype not in (torch.float32, torch.bfloat16):
            out = out.float()
        base = (self._ridge_base(xt, out.device)
                if self.residual_ridge is not None else None)
        conf = None
        if self.conformal is not None:
            if (self._conformal_t is None
                    or self._conformal_t.device != out.device):
                self._conformal_t = torch.from_numpy(np.asarray(
                    self.conformal, dtype=np.float32)).to(out.device)
            conf = self._conformal_t
        sv = self._scaler_vectors(out.device)
        res = band_scores(out.contiguous(), y, sv[1], sv[0], base=base,
                          conformal=conf,
                          log1p=self.target_transform == "log1p",
                          lengths=lengths, threshold=float(threshold),
                          min_run=int(min_run), want_bands=detail)
        check = SanityCheck(
            metric_names=list(self.metric_names), threshold=float(threshold),
            min_run=int(min_run),
            max_score=res.max_score.cpu().numpy(),
            n_flagged=res.n_flagged.cpu().numpy(),
            first_flag=res.first_flag.cpu().numpy(),
            n_observed=res.n_observed.cpu().numpy())
        if detail:
            check.scores, check.flags, check.bands = res.scores, res.flags, res.bands
            check.lengths = lengths
        return check

    def predict_what_if(self, synthesizer, traffic_plan, step_size: int,
                        rng=None) -> Dict[str, np.ndarray]:
        """What-if pipeline: synthesize traffic for a hypothetical API mix,
        window it, and predict (reference: synthesizer.py + SURVEY.md 3.3)."""
        series = synthesizer.synthesize_series(traffic_plan, rng=rng)  # (T, P)
        n = len(series) - step_size
        if n <= 0:
            windows = series[None, :, :].astype(np.float64)
        else:
            from ..data.windows import sliding_window

            windows = sliding_window(series.astype(np.float64), step_size)
        return self.predict(windows)
