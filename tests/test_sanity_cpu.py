"""The device sanity check without a device: ``reference_band_scores`` (the
CPU path of ``ops.band_scores`` and the kernel's oracle) against the existing
host scorer, the run-length edge cases, ``Predictor.sanity_check`` against
``predict`` + ``AnomalyScorer.score_all``, and the ``{'windows', 'measured'}``
form of ``POST /anomaly``.

The bands of the first test are computed here, in numpy float64, by the
documented steps — not by the code under test.
"""

import numpy as np
import pytest
import torch

from deeprest_amd.data.synthetic import SyntheticApp, SyntheticAppConfig
from deeprest_amd.data.windows import MinMaxScaler, sliding_window
from deeprest_amd.engine.config import DataConfig, EngineConfig, TrainConfig
from deeprest_amd.engine.trainer import Trainer
from deeprest_amd.models.net import DeepRestNetConfig
from deeprest_amd.ops import band_scores, reference_band_scores
from deeprest_amd.serve.anomaly import AnomalyScorer, flag_intervals
from deeprest_amd.serve.predictor import Predictor

THR = 0.25
KS = (-0.5, 0.0, THR / 4, 2 * THR, 5 * THR)


def _bands_by_the_steps(out, base, conformal, y_min, y_scale, log1p):
    """numpy float64: add base, sort, widen, inverse-scale, expm1, clamp."""
    q = np.asarray(out, dtype=np.float64)
    if base is not None:
        q = q + np.asarray(base, dtype=np.float64)[..., None]
    q = np.sort(q, axis=-1)
    if conformal is not None:
        c = np.asarray(conformal, dtype=np.float64)
        q[..., 0] = np.minimum(q[..., 0] - c, q[..., 1])
        q[..., 2] = np.maximum(q[..., 2] + c, q[..., 1])
    q = q * np.asarray(y_scale)[:, None] + np.asarray(y_min)[:, None]
    if log1p:
        q = np.expm1(q)
    return np.maximum(q, 1e-6)


def _measured_on_margin(q, rng, thr=THR, gaps=0.0):
    """q2 + k * band with k drawn from {-0.5, 0, thr/4, 2 thr, 5 thr}, in runs
    of random length so that long and short runs both occur."""
    ks = np.array((-0.5, 0.0, thr / 4, 2 * thr, 5 * thr))
    shape = q.shape[:-1]
    N, T, M = shape
    k = np.empty(shape)
    for n in range(N):
        for m in range(M):
            t = 0
            while t < T:
                run = int(rng.integers(1, 6))
                hot = rng.random() < 0.5
                k[n, t:t + run, m] = rng.choice(ks[3:] if hot else ks[:3], size=min(run, T - t))
                t += run
    y = q[..., 2] + k * np.maximum(q[..., 2] - q[..., 0], 1e-9)
    if gaps:
        y[rng.random(shape) < gaps] = np.nan
    return y


@pytest.mark.parametrize("base,conformal,log1p,lengths", [
    (True, True, True, (12, 1, 7)),
    (False, False, False, None),
    (True, False, False, (5, 12, 40)),
    (False, True, True, None),
])
@pytest.mark.parametrize("min_run", [1, 3])
def test_reference_matches_anomaly_scorer(base, conformal, log1p, lengths, min_run):
    N, T, M = 3, 12, 4
    rng = np.random.default_rng(7 + min_run)
    out = rng.normal(0.5, 0.5, (N, T, M, 1)) + rng.permuted(
        np.array([-0.3, 0.0, 0.4]) * rng.uniform(0.5, 1.5, (N, T, M, 1)), axis=-1)
    b = rng.normal(0, 0.2, (N, T, M)) if base else None
    c = np.array([0.05, -0.02, 0.2, 0.0]) if conformal else None
    y_min = np.array([0.0, 2.0, 0.5, 1.0])
    y_scale = np.array([1.0, 3.0, 0.7, 2.0])
    q = _bands_by_the_steps(out, b, c, y_min, y_scale, log1p)
    y = _measured_on_margin(q, rng, gaps=0.1)
    t64 = lambda a: None if a is None else torch.from_numpy(np.asarray(a, dtype=np.float64))
    lens = None if lengths is None else torch.tensor(lengths, dtype=torch.int32)
    res = reference_band_scores(
        t64(out), t64(y), t64(y_min), t64(y_scale), base=t64(b), conformal=t64(c),
        log1p=log1p, lengths=lens, threshold=THR, min_run=min_run, want_bands=True)
    assert res.scores.dtype == torch.float64 and res.flags.dtype == torch.uint8
    scorer = AnomalyScorer(threshold=THR, min_run=min_run)
    some_flag = False
    for n in range(N):
        L = T if lengths is None else min(max(lengths[n], 1), T)
        for m in range(M):
            rep = scorer.score(y[n, :L, m], q[n, :L, m, 0], q[n, :L, m, 1], q[n, :L, m, 2])
            got_flags = res.flags[n, :L, m].numpy().astype(bool)
            assert np.array_equal(got_flags, rep.flags), (n, m)
            assert flag_intervals(got_flags) == rep.windows, (n, m)
            np.testing.assert_allclose(res.scores[n, :L, m].numpy(), rep.scores,
                                       rtol=0, atol=1e-12, equal_nan=True)
            np.testing.assert_allclose(res.bands[n, :L, m].numpy(), q[n, :L, m],
                                       rtol=0, atol=1e-12)
            # padding: NaN scores and bands, no flags
            assert torch.isnan(res.scores[n, L:, m]).all()
            assert torch.isnan(res.bands[n, L:, m]).all()
            assert not res.flags[n, L:, m].any()
            obs = np.isfinite(y[n, :L, m])
            assert int(res.n_observed[n, m]) == int(obs.sum())
            want_max = float(rep.scores[obs].max()) if obs.any() else 0.0
            assert abs(float(res.max_score[n, m]) - want_max) <= 1e-12
            assert int(res.n_flagged[n, m]) == int(rep.flags.sum())
            first = int(np.argmax(rep.flags)) if rep.flags.any() else -1
            assert int(res.first_flag[n, m]) == first
            some_flag |= bool(rep.flags.any())
    assert some_flag, "the inputs must flag something"


# out triple (1, 2, 3) under the identity scaler: q2 = 3, band = 2.
# 'x': over (y = 3 + 2 * 1.0), '.': under (y = 2), 'n': not observed.
RUN_CASES = [
    # pattern,          L,    min_run, expected flags
    ("xx.xxx.x",        None, 1,  "xx.xxx.x"),
    ("xx.xxx.x",        None, 3,  "...xxx.."),
    ("xxxxxxxx",        None, 9,  "........"),     # min_run = T + 1
    ("xxxxxxxx",        None, 8,  "xxxxxxxx"),
    ("xxx.....",        None, 3,  "xxx....."),     # run touching t = 0
    (".....xxx",        None, 3,  ".....xxx"),     # run touching t = T - 1
    ("......xx",        None, 3,  "........"),
    ("xxnxx.xx",        None, 3,  "........"),     # run cut by a NaN
    ("xxnxxx..",        None, 3,  "...xxx.."),
    ("..xxxxxx",        5,    3,  "..xxx..."),     # run ending exactly at L
    (".xxxxxxx",        3,    3,  "........"),     # two overs before L only
    ("x.......",        0,    1,  "x......."),     # L clamps to 1
]


@pytest.mark.parametrize("pattern,L,min_run,expected", RUN_CASES)
def test_run_length_cases(pattern, L, min_run, expected):
    T = len(pattern)
    y = torch.tensor([{"x": 5.0, ".": 2.0, "n": float("nan")}[ch] for ch in pattern],
                     dtype=torch.float64).reshape(1, T, 1)
    out = torch.tensor([2.0, 3.0, 1.0], dtype=torch.float64).expand(1, T, 1, 3).contiguous()
    one, zero = torch.ones(1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    lens = None if L is None else torch.tensor([L], dtype=torch.int32)
    for fn in (reference_band_scores, band_scores):          # CPU: the same path
        res = fn(out, y, zero, one, lengths=lens, threshold=THR, min_run=min_run)
        got = "".join("x" if f else "." for f in res.flags[0, :, 0].tolist())
        assert got == expected
        assert int(res.n_flagged[0, 0]) == expected.count("x")
        assert int(res.first_flag[0, 0]) == expected.find("x")
        Lc = T if L is None else min(max(L, 1), T)
        assert int(res.n_observed[0, 0]) == sum(ch != "n" for ch in pattern[:Lc])
        want_max = 1.0 if "x" in pattern[:Lc] else 0.0
        assert float(res.max_score[0, 0]) == want_max


def test_nothing_observed_and_garbage_is_selected_away():
    """max_score is 0 without an observation, and NaN / Inf in the padding
    and the gaps reach nothing valid."""
    N, T, M = 2, 6, 3
    g = torch.Generator().manual_seed(3)
    out = torch.rand(N, T, M, 3, generator=g, dtype=torch.float64) + 1.0
    base = torch.rand(N, T, M, generator=g, dtype=torch.float64)
    y = 10.0 * torch.rand(N, T, M, generator=g, dtype=torch.float64)
    y[:, :, 1] = float("nan")                       # metric 1: nothing observed
    y[0, 2, 0] = float("nan")
    lens = torch.tensor([4, 6], dtype=torch.int32)
    mn, sc = torch.zeros(M, dtype=torch.float64), torch.ones(M, dtype=torch.float64)
    kw = dict(lengths=lens, threshold=THR, min_run=1, want_bands=True)
    clean = reference_band_scores(out, y, mn, sc, base=base, **kw)
    assert (clean.max_score[:, 1] == 0).all() and (clean.n_observed[:, 1] == 0).all()
    assert (clean.first_flag[:, 1] == -1).all()
    out2, base2, y2 = out.clone(), base.clone(), y.clone()
    out2[0, 4:] = float("nan")
    base2[0, 4:] = float("inf")
    y2[0, 4:] = float("-inf")
    y2[0, 2, 0] = float("inf")
    dirty = reference_band_scores(out2, y2, mn, sc, base=base2, **kw)
    for name in ("scores", "flags", "max_score", "n_flagged", "first_flag",
                 "n_observed", "bands"):
        a, b = getattr(clean, name), getattr(dirty, name)
        assert torch.equal(torch.nan_to_num(a.double(), nan=-7.0),
                           torch.nan_to_num(b.double(), nan=-7.0)), name


def test_op_rejects_bad_input():
    out = torch.zeros(2, 4, 3, 3)
    y = torch.zeros(2, 4, 3)
    mn, sc = torch.zeros(3), torch.ones(3)
    good = torch.tensor([4, 2], dtype=torch.int32)
    band_scores(out, y, mn, sc, lengths=good)
    for fn in (band_scores, reference_band_scores):
        with pytest.raises(ValueError, match="Q must be 3"):
            fn(torch.zeros(2, 4, 3, 2), y, mn, sc)
        with pytest.raises(ValueError, match="min_run"):
            fn(out, y, mn, sc, min_run=0)
        for bad in (good.long(), torch.tensor([4], dtype=torch.int32), [4, 2]):
            with pytest.raises(ValueError, match="lengths"):
                fn(out, y, mn, sc, lengths=bad)
        with pytest.raises(ValueError, match="measured"):
            fn(out, y[:, :3], mn, sc)
        with pytest.raises(ValueError, match="y_scale"):
            fn(out, y, mn, torch.ones(4))
        with pytest.raises(ValueError, match="base"):
            fn(out, y, mn, sc, base=torch.zeros(2, 4))
        with pytest.raises(ValueError, match="conformal"):
            fn(out, y, mn, sc, conformal=torch.zeros(2))


# ------------------------------------------------------------------ predictor
@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    # the small trainer setup of tests/test_serve.py
    torch.manual_seed(0)
    np.random.seed(0)
    tmp = tmp_path_factory.mktemp("sanity")
    app = SyntheticApp(SyntheticAppConfig(
        n_apis=4, n_components=5, windows_per_day=60, n_days=2, seed=33))
    data = app.generate_featurized()
    cfg = EngineConfig()
    cfg.data = DataConfig(step_size=20, split=0.4)
    cfg.train = TrainConfig(epochs=1, batch_size=8, run_baselines=False,
                            log_every=0, checkpoint_path=str(tmp / "ckpt.pt"))
    cfg.model = DeepRestNetConfig(d_model=32, n_heads=4, n_layers=1, d_ff=64,
                                  hidden=16, comp_dim=8, dropout=0.0)
    Trainer(data, cfg, device=torch.device("cpu")).train()
    pred = Predictor.from_checkpoint(str(tmp / "ckpt.pt"), device=torch.device("cpu"))
    windows = sliding_window(np.asarray(data.traffic, dtype=np.float64), 20)[:3]
    return data, pred, windows


def _check_against_host_route(pred, windows, rng, thr=THR, min_run=3):
    """sanity_check == predict -> AnomalyScorer.score_all, window by window,
    on measured series built from the predictor's own bands on the margin
    (f32-representable, so both routes see the same numbers)."""
    preds = pred.predict(windows)
    names = pred.metric_names
    q = np.stack([preds[k] for k in names], axis=2).astype(np.float64)   # (N, T, M, 3)
    y = _measured_on_margin(q, rng, thr=thr, gaps=0.05).astype(np.float32)
    measured = {k: y[:, :, m] for m, k in enumerate(names)}
    check = pred.sanity_check(windows, measured, threshold=thr, min_run=min_run,
                              detail=True)
    assert check.keys() == list(names)
    scorer = AnomalyScorer(threshold=thr, min_run=min_run)
    flagged = 0
    for i in range(len(windows)):
        want = scorer.score_all({k: y[i, :, m].astype(np.float64)
                                 for m, k in enumerate(names)},
                                {k: preds[k][i] for k in names})
        got = check.reports(i)
        for m, k in enumerate(names):
            assert np.array_equal(got[k].flags, want[k].flags), (i, k)
            assert got[k].windows == want[k].windows
            obs = np.isfinite(y[i, :, m])
            want_max = float(want[k].scores[obs].max()) if obs.any() else 0.0
            assert abs(check.max_score[i, m] - want_max) <= 1e-5 * abs(want_max), (i, k)
            assert check[k]["max_score"][i] == check.max_score[i, m]
            assert bool(check[k]["anomalous"][i]) == want[k].is_anomalous
            assert check[k]["n_flagged"][i] == want[k].flags.sum()
            assert check[k]["n_observed"][i] == obs.sum()
            first = int(np.argmax(want[k].flags)) if want[k].flags.any() else -1
            assert check[k]["first_flag"][i] == first
            flagged += int(want[k].flags.sum())
    assert flagged > 0
    # the (N, T, M) array form is the same request
    again = pred.sanity_check(windows, y, threshold=thr, min_run=min_run)
    assert np.array_equal(again.n_flagged, check.n_flagged)
    assert again.flags is None and again.bands is None
    with pytest.raises(ValueError):
        again.reports(0)


def test_predictor_sanity_check_matches_host_route(trained):
    data, pred, windows = trained
    _check_against_host_route(pred, windows, np.random.default_rng(5))


def test_hand_built_predictor_with_zero_scale_ridge_and_conformal(trained):
    """One scaler with scale 0 (its metric passes through unscaled), the
    ridge residual base and the conformal widening, all on the host route's
    terms."""
    data, ckpt_pred, windows = trained
    M, P = len(ckpt_pred.metric_names), ckpt_pred.model.spec.num_paths
    rng = np.random.default_rng(9)
    y_scalers = [MinMaxScaler(min_val=2.0 + m, max_val=5.0 + 2 * m) for m in range(M)]
    y_scalers[1] = MinMaxScaler(min_val=3.0, max_val=3.0)
    assert y_scalers[1].scale == 0.0
    pred = Predictor(ckpt_pred.model, ckpt_pred.x_scaler, y_scalers,
                     ckpt_pred.metric_names, device=torch.device("cpu"),
                     residual_ridge=rng.normal(0, 0.05, (P + 1, M)),
                     conformal=rng.uniform(-0.02, 0.2, M))
    _check_against_host_route(pred, windows, rng)
    # an absent metric is entirely unobserved
    some = pred.metric_names[0]
    check = pred.sanity_check(windows, {some: np.full(windows.shape[:2], 1e9)},
                              min_run=1)
    assert check[some]["anomalous"].all() and (check[some]["first_flag"] == 0).all()
    for k in pred.metric_names[1:]:
        assert not check[k]["anomalous"].any()
        assert (check[k]["n_observed"] == 0).all() and (check[k]["max_score"] == 0).all()
    with pytest.raises(ValueError, match="unknown"):
        pred.sanity_check(windows, {"no_such_metric": np.zeros(windows.shape[:2])})
    with pytest.raises(ValueError, match="max_window"):
        pred.sanity_check(windows, {}, lengths=[20, 20, 20])


def test_injected_burst_is_flagged(trained):
    """The burst of test_cryptojacking_detection_end_to_end, through the
    device route's entry point."""
    data, pred, windows = trained
    w = windows[:1]
    out = pred.predict(w)
    hit, calm = data.metric_names[0], data.metric_names[1]
    q = out[hit][0]
    measured = {k: out[k][:, :, 1].copy() for k in data.metric_names}   # on the median
    burst = 50.0 * float(np.mean(q[:, 2] - q[:, 0])) + 50.0
    measured[hit][0, 8:14] += burst
    check = pred.sanity_check(w, measured, threshold=1.0, min_run=3, detail=True)
    assert check[hit]["anomalous"][0]
    assert 8 <= check[hit]["first_flag"][0] < 14
    assert check[hit]["n_flagged"][0] == 6
    assert check.reports(0)[hit].windows == [(8, 14)]
    assert not check[calm]["anomalous"][0] and check[calm]["first_flag"][0] == -1
    assert check[calm]["max_score"][0] == 0.0


# ----------------------------------------------------------------------- REST
def test_rest_anomaly_from_windows_and_measured(trained):
    from starlette.testclient import TestClient

    from deeprest_amd.serve.api import create_app

    data, pred, windows = trained
    client = TestClient(create_app(predictor=pred))
    names = data.metric_names
    out = pred.predict(windows[:2])
    measured = {k: out[k][:, :, 1].tolist() for k in names}
    burst = 50.0 * float(np.mean(out[names[0]][..., 2] - out[names[0]][..., 0])) + 50.0
    for t in range(8, 14):
        measured[names[0]][1][t] += burst               # window 1 only
    measured[names[1]][0][3] = None                     # JSON null: not observed
    del measured[names[2]]                              # absent: unobserved
    r = client.post("/anomaly", json={"windows": windows[:2].tolist(),
                                      "measured": measured, "threshold": 1.0})
    assert r.status_code == 200, r.text
    body = r.json()
    assert isinstance(body, list) and len(body) == 2
    assert set(body[0]) == set(names)
    assert set(body[1][names[0]]) == {"anomalous", "windows", "max_score", "n_observed"}
    assert body[1][names[0]]["anomalous"] is True
    assert body[1][names[0]]["windows"] == [[8, 14]]
    assert body[1][names[0]]["max_score"] > 1.0
    assert body[0][names[0]]["anomalous"] is False
    assert body[0][names[1]]["n_observed"] == 19 and body[1][names[1]]["n_observed"] == 20
    assert body[0][names[2]] == {"anomalous": False, "windows": [],
                                 "max_score": 0.0, "n_observed": 0}
    # one window: one dict, as the 'predicted' form answers
    one = client.post("/anomaly", json={
        "windows": windows[1:2].tolist(),
        "measured": {names[0]: [measured[names[0]][1]]},
        "threshold": 1.0, "min_run": 6})
    assert one.status_code == 200 and one.json()[names[0]]["windows"] == [[8, 14]]
    bad = client.post("/anomaly", json={"windows": windows[:1].tolist(),
                                        "measured": {"nope": [[0.0] * 20]}})
    assert bad.status_code == 422
    # no model: 400
    bare = TestClient(create_app())
    r = bare.post("/anomaly", json={"windows": windows[:1].tolist(),
                                    "measured": {names[0]: [[1.0] * 20]}})
    assert r.status_code == 400
    # the 'predicted' form is untouched and needs no model
    for c in (client, bare):
        r = c.post("/anomaly", json={"measured": {names[0]: [100.0] * 10},
                                     "predicted": {names[0]: [[10.0, 20.0, 30.0]] * 10},
                                     "windows": windows[:1].tolist()})
        assert r.status_code == 200
        assert r.json() == {names[0]: {"anomalous": True, "windows": [[0, 10]],
                                       "max_score": 3.5}}
