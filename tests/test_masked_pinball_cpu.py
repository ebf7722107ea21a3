"""Missing labels (NaN = not observed) end to end on the CPU: the masked
pinball reference, NaN-aware scaling and filling, the collector's ``nan``
mode, burst injection, and a training run on gappy labels."""

import numpy as np
import pytest
import torch

from deeprest_amd.data.collector import Collector
from deeprest_amd.data.synthetic import (SyntheticApp, SyntheticAppConfig,
                                         inject_missing)
from deeprest_amd.data.windows import MinMaxScaler, forward_fill, minmax_fit
from deeprest_amd.engine.config import DataConfig, EngineConfig, TrainConfig
from deeprest_amd.engine.dataset import EstimationDataset
from deeprest_amd.engine.trainer import Trainer
from deeprest_amd.models.net import DeepRestNetConfig
from deeprest_amd.ops import (masked_pinball_loss, reference_masked_pinball_loss,
                              reference_pinball_loss)

QUANTILES = (0.05, 0.5, 0.95)


def _per_metric_loop(outputs, labels, quantiles):
    """The definition, one metric at a time, in plain Python/float64."""
    total, used = 0.0, 0
    B, T, M, Q = outputs.shape
    for m in range(M):
        s, c = 0.0, 0
        for b in range(B):
            for t in range(T):
                y = float(labels[b, t, m])
                if not np.isfinite(y):
                    continue
                for i, q in enumerate(quantiles):
                    e = y - float(outputs[b, t, m, i])
                    s += max((q - 1.0) * e, q * e)
                c += 1
        if c:
            total += s / c
            used += 1
    return total / used if used else 0.0


# ------------------------------------------------------------- reference op
def test_reference_without_nan_equals_dense_reference():
    out = torch.randn(4, 12, 5, 3, dtype=torch.float64)
    y = torch.rand(4, 12, 5, dtype=torch.float64)
    assert torch.equal(reference_masked_pinball_loss(out, y, QUANTILES),
                       reference_pinball_loss(out, y, QUANTILES))
    out32, y32 = out.float(), y.float()
    assert torch.equal(reference_masked_pinball_loss(out32, y32, QUANTILES),
                       reference_pinball_loss(out32, y32, QUANTILES))


def test_reference_with_nan_matches_per_metric_loop():
    gen = torch.Generator().manual_seed(3)
    out = torch.randn(3, 7, 6, 3, dtype=torch.float64, generator=gen)
    y = torch.rand(3, 7, 6, dtype=torch.float64, generator=gen)
    miss = torch.rand(3, 7, 6, generator=gen) < 0.4
    miss[:, :, 2] = True                                  # one metric gone
    assert miss[:, :, [0, 1, 3, 4, 5]].any() and not miss[:, :, 0].all()
    y[miss] = float("nan")

    o = out.clone().requires_grad_(True)
    loss = reference_masked_pinball_loss(o, y, QUANTILES)
    loss.backward()
    assert abs(float(loss.detach()) - _per_metric_loop(out, y, QUANTILES)) < 1e-12
    assert torch.isfinite(o.grad).all()
    assert (o.grad[miss] == 0).all()
    assert (o.grad[~miss] != 0).all()

    # whatever outputs hold at a missing position changes nothing
    poisoned = out.clone()
    poisoned[miss] = float("nan")
    p = poisoned.requires_grad_(True)
    loss_p = reference_masked_pinball_loss(p, y, QUANTILES)
    loss_p.backward()
    assert torch.equal(loss_p, loss)
    assert torch.equal(p.grad, o.grad)
    # the public op is the reference on the CPU
    assert torch.equal(masked_pinball_loss(out, y, QUANTILES), loss.detach())


def test_reference_all_missing_is_zero():
    out = torch.randn(2, 5, 3, 3).requires_grad_(True)
    y = torch.full((2, 5, 3), float("nan"))
    loss = reference_masked_pinball_loss(out, y, QUANTILES)
    loss.backward()
    assert float(loss.detach()) == 0.0
    assert (out.grad == 0).all()


def test_model_loss_routes_missing_flag():
    from deeprest_amd.models.net import DeepRestNet, build_model_spec

    spec = build_model_spec(_tiny_data())
    model = DeepRestNet(spec, _tiny_config().model)
    out = torch.randn(2, 4, spec.num_metrics, 3)
    y = torch.rand(2, 4, spec.num_metrics)
    assert torch.equal(model.loss(out, y), model.loss(out, y, missing=True))
    y[0, 1, 0] = float("nan")
    assert torch.isnan(model.loss(out, y))
    assert torch.isfinite(model.loss(out, y, missing=True))


# ------------------------------------------------------------------ windows
def test_minmax_fit_ignores_nan_and_keeps_finite_results():
    rng = np.random.default_rng(0)
    a = rng.normal(size=(40, 6))
    assert minmax_fit(a, 25) == (float(a[:25].min()), float(a[:25].max()))
    b = a.copy()
    b[3, 2] = np.nan
    b[30, 0] = np.nan                       # past the split: not looked at
    keep = np.ones_like(a[:25], dtype=bool)
    keep[3, 2] = False
    assert minmax_fit(b, 25) == (float(a[:25][keep].min()), float(a[:25][keep].max()))
    sc = MinMaxScaler().fit(b, 25)
    out = sc.transform(b)
    assert np.isnan(out[3, 2]) and np.isnan(out[30, 0])
    assert np.isfinite(out[:25][keep]).all()


def test_minmax_fit_all_nan_train_names_the_series():
    a = np.arange(10.0)
    a[:6] = np.nan
    with pytest.raises(ValueError, match="svc-7_cpu"):
        minmax_fit(a, 6, name="svc-7_cpu")
    assert minmax_fit(a, 7, name="svc-7_cpu") == (6.0, 6.0)


def test_forward_fill():
    nan = np.nan
    s = np.array([nan, nan, 3.0, nan, 5.0, nan, nan])
    np.testing.assert_array_equal(forward_fill(s), [3, 3, 3, 3, 5, 5, 5])
    assert np.isnan(s[0])                                 # input untouched
    two = np.array([[1.0, nan], [nan, nan], [nan, 7.0], [4.0, nan]])
    np.testing.assert_array_equal(forward_fill(two),
                                  [[1, 7], [1, 7], [1, 7], [4, 7]])
    dense = np.arange(6.0).reshape(3, 2)
    np.testing.assert_array_equal(forward_fill(dense), dense)
    assert np.isnan(forward_fill(np.array([nan, nan]))).all()


# ---------------------------------------------------------------- collector
def _sample(t, comp, res, value):
    return {"component": comp, "resource": res, "value": value, "timestamp": t}


def _stream():
    # 10 s windows from t0 = 0.  a/cpu: sampled in windows 0, 1, 4 (gap 2-3);
    # b/mem: first seen in window 2 (late start), then 3 and 4
    return [
        _sample(1.0, "a", "cpu", 1.0), _sample(12.0, "a", "cpu", 2.0),
        _sample(41.0, "a", "cpu", 5.0),
        _sample(25.0, "b", "mem", 30.0), _sample(33.0, "b", "mem", 31.0),
        _sample(47.0, "b", "mem", 32.0),
    ]


def _values(windows):
    return [{(m["component"], m["resource"]): m["value"] for m in w["metrics"]}
            for w in windows]


def test_collector_nan_mode_marks_unsampled_windows():
    from deeprest_amd.data.contract import validate_raw_data

    col = Collector(window_sec=10.0, t0=0.0, missing="nan")
    col.add_metric_samples(_stream())
    windows = col.windows()
    validate_raw_data(windows)                 # NaN is a valid float value
    vals = _values(windows)
    assert len(vals) == 5
    a = [v[("a", "cpu")] for v in vals]
    b = [v[("b", "mem")] for v in vals]
    np.testing.assert_array_equal(a, [1.0, 2.0, np.nan, np.nan, 5.0])
    np.testing.assert_array_equal(b, [np.nan, np.nan, 30.0, 31.0, 32.0])
    # identity and order of the metrics are the same in every window
    keys = [[(m["component"], m["resource"]) for m in w["metrics"]] for w in windows]
    assert all(k == keys[0] for k in keys)


def test_collector_carry_mode_is_unchanged():
    default = Collector(window_sec=10.0, t0=0.0)
    carry = Collector(window_sec=10.0, t0=0.0, missing="carry")
    for col in (default, carry):
        col.add_metric_samples(_stream())
    assert default.windows() == carry.windows()
    vals = _values(default.windows())
    assert [v[("a", "cpu")] for v in vals] == [1.0, 2.0, 2.0, 2.0, 5.0]
    assert [v[("b", "mem")] for v in vals] == [0.0, 0.0, 30.0, 31.0, 32.0]
    with pytest.raises(ValueError):
        Collector(missing="zero")


# ------------------------------------------------------------ inject_missing
def _tiny_data():
    app = SyntheticApp(SyntheticAppConfig(
        n_apis=4, n_components=5, windows_per_day=60, n_days=2, seed=21))
    return app.generate_featurized()


def _tiny_config(epochs=2):
    cfg = EngineConfig()
    cfg.data = DataConfig(step_size=20, split=0.4)
    cfg.train = TrainConfig(epochs=epochs, batch_size=8, baseline_epochs=3,
                            eval_cycles=3, log_every=0, seed=0)
    cfg.model = DeepRestNetConfig(d_model=32, n_heads=4, n_layers=1, d_ff=64,
                                  hidden=16, comp_dim=8, dropout=0.0)
    return cfg


RATE, MEAN_GAP, SEED = 0.3, 4.0, 7


def _missing_share(data):
    y = np.stack([data.resources[n] for n in data.metric_names], axis=-1)
    return float(np.isnan(y).mean()), y


def test_inject_missing_deterministic_and_near_rate():
    clean = _tiny_data()
    a = inject_missing(_tiny_data(), RATE, MEAN_GAP, SEED)
    b = inject_missing(_tiny_data(), RATE, MEAN_GAP, SEED)
    c = inject_missing(_tiny_data(), RATE, MEAN_GAP, SEED + 1)
    share, ya = _missing_share(a)
    _, yb = _missing_share(b)
    _, yc = _missing_share(c)
    _, y0 = _missing_share(clean)
    np.testing.assert_array_equal(np.isnan(ya), np.isnan(yb))
    assert not np.array_equal(np.isnan(ya), np.isnan(yc))
    # observed values untouched, traffic untouched
    np.testing.assert_array_equal(ya[~np.isnan(ya)], y0[~np.isnan(ya)])
    np.testing.assert_array_equal(a.traffic, clean.traffic)
    # 18 metrics x 120 windows, gaps of mean 4 and observed runs of mean
    # 9.3: ~160 gap/run cycles.  With geometric lengths (variance ~ mean^2)
    # the share's standard deviation is sqrt(160 * (0.7^2 * 16 + 0.3^2 * 87))
    # / 2160 ~ 0.023, so +-0.1 is four sigma
    assert abs(share - RATE) < 0.1, share
    # bursts, not salt and pepper: fewer gaps than missing samples / 2
    gone = np.isnan(ya)
    starts = (gone[1:] & ~gone[:-1]).sum() + gone[0].sum()
    assert starts < gone.sum() / 2
    # a selection of metrics leaves the others whole
    names = clean.metric_names[:2]
    d = inject_missing(_tiny_data(), RATE, MEAN_GAP, SEED, metrics=names)
    for n in d.metric_names:
        assert np.isnan(d.resources[n]).any() == (n in names)
    assert inject_missing(_tiny_data(), 0.0, MEAN_GAP, SEED).resources[names[0]].tolist() \
        == clean.resources[names[0]].tolist()


# ------------------------------------------------------------- end to end
def test_dataset_keeps_nan_and_builds_filled_copies():
    dense = EstimationDataset(_tiny_data(), step_size=20, split_fraction=0.4)
    assert not dense.has_missing
    assert dense.y_filled is dense.y and dense.y_raw_filled is dense.y_raw

    data = inject_missing(_tiny_data(), RATE, MEAN_GAP, SEED)
    ds = EstimationDataset(data, step_size=20, split_fraction=0.4)
    assert ds.has_missing
    gone = np.isnan(ds.y_raw)
    assert gone.any()
    np.testing.assert_array_equal(np.isnan(ds.y.numpy()), gone)
    assert np.isnan(ds.y_train.numpy()).any() and np.isnan(ds.y_test.numpy()).any()
    assert np.isfinite(ds.y_filled.numpy()).all()
    assert np.isfinite(ds.y_raw_filled).all()
    # filled copies agree with the labels wherever those were observed
    np.testing.assert_array_equal(ds.y_raw_filled[~gone], ds.y_raw[~gone])
    np.testing.assert_array_equal(ds.y_filled.numpy()[~gone], ds.y.numpy()[~gone])
    # the scalers saw the observed values only
    for idx, sc in enumerate(ds.y_scalers):
        col = ds.y_raw[: ds.split, :, idx]
        assert sc.min_val == np.nanmin(col) and sc.max_val == np.nanmax(col)


@pytest.mark.parametrize("residual_base", ["none", "trace-ridge"])
def test_training_on_gappy_labels_end_to_end(residual_base):
    data = inject_missing(_tiny_data(), RATE, MEAN_GAP, SEED)
    cfg = _tiny_config(epochs=2)
    cfg.train.residual_base = residual_base
    cfg.train.conformal = 0.9
    trainer = Trainer(data, cfg, device=torch.device("cpu"))
    ds = trainer.dataset
    assert ds.has_missing
    # something to mask, and every metric keeps observed samples to learn from
    y_train = ds.y_train.numpy()
    assert np.isnan(y_train).any()
    assert np.isfinite(y_train).any(axis=(0, 1)).all()
    eval_idx = ds.eval_window_indices(cfg.train.eval_cycles)
    y_eval = ds.y_test[eval_idx].numpy()
    assert np.isnan(y_eval).any()
    assert np.isfinite(y_eval).any(axis=(0, 1)).all()

    result = trainer.train()
    assert len(result.train_losses) == 2
    assert np.isfinite(result.train_losses).all()
    assert len(result.test_losses) >= 2 and np.isfinite(result.test_losses).all()
    assert set(result.error_tables) == set(data.metric_names)
    for per_est in result.error_tables.values():
        assert set(per_est) == {"resrc", "comp", "deepr"}
        for stats in per_est.values():
            assert np.isfinite(list(stats.values())).all()
    for c in result.coverage.values():
        assert abs(c["coverage"] + c["below"] + c["above"] - 1.0) < 1e-9
    assert np.isfinite(trainer._conformal).all()
