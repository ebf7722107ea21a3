"""Variable-length windows on the CPU path (fp32): the references with
per-sample lengths, the model's ``lengths`` argument, the predictor's
``max_window`` and the micro-batcher's mixed-length flush.

The contract checked everywhere: ``f(x, lengths)[b, :L]`` equals ``f`` on the
sample truncated to its own length, nothing stored in the padding (NaN
included) reaches a valid output, and padded outputs are exact zeros (NaN
after the predictor's denormalization)."""

import threading

import numpy as np
import pytest
import torch

H = 128


# ------------------------------------------------------------------ attention
def _qkv(B=3, NH=2, T=9, D=8, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(B, NH, T, D, generator=gen) for _ in range(3)]


def test_reference_mha_lengths_match_truncated_samples():
    from deeprest_amd.ops import mha_forward, reference_mha

    q, k, v = _qkv()
    lens = [9, 1, 4]
    lengths = torch.tensor(lens, dtype=torch.int32)
    out = reference_mha(q, k, v, kv_lengths=lengths)
    for b, L in enumerate(lens):
        ref = reference_mha(q[b:b + 1, :, :L], k[b:b + 1, :, :L], v[b:b + 1, :, :L])
        torch.testing.assert_close(out[b, :, :L], ref[0], rtol=1e-5, atol=1e-6)
        assert (out[b, :, L:] == 0).all()
    # the op's CPU route is the reference
    assert torch.equal(mha_forward(q, k, v, kv_lengths=lengths), out)

    # NaN in the padded q/k/v positions: valid rows unchanged and finite
    qp, kp, vp = (t.clone() for t in (q, k, v))
    for b, L in enumerate(lens):
        for t in (qp, kp, vp):
            t[b, :, L:] = float("nan")
    poisoned = reference_mha(qp, kp, vp, kv_lengths=lengths)
    assert torch.isfinite(poisoned).all()
    assert torch.equal(poisoned, out)


def test_mha_lengths_are_inference_only():
    from deeprest_amd.ops import mha_forward

    q, k, v = _qkv()
    q.requires_grad_(True)
    with pytest.raises(RuntimeError):
        mha_forward(q, k, v, kv_lengths=torch.tensor([9, 1, 4], dtype=torch.int32))


# ------------------------------------------------------------------------ gru
def _gru_inputs(B=3, T=7, C=5, O=9, seed=1):
    gen = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=gen) * 0.4
    return [mk(B, T, 3 * H), mk(3 * H, H) / H ** 0.5, mk(3 * H) * 0.2,
            mk(B, C, H), 1.0 + 0.1 * mk(C, 3 * H), 0.1 * mk(C, 3 * H),
            mk(O, H) / H ** 0.5]


@pytest.mark.parametrize("reverse", [False, True])
def test_reference_gru_lengths_match_truncated_samples(reverse):
    from deeprest_amd.ops import fused_gru_decode
    from deeprest_amd.ops.gru import reference_gru_sequence

    xg, w_hh, b_hh, h0, gamma, beta, w_head = _gru_inputs()
    lens = [7, 1, 4]
    lengths = torch.tensor(lens, dtype=torch.int32)
    h_all = reference_gru_sequence(xg, w_hh, b_hh, h0, gamma, beta, reverse,
                                   lengths=lengths)
    out, h_last = fused_gru_decode(xg, w_hh, b_hh, h0, gamma, beta, w_head,
                                   reverse=reverse, lengths=lengths)
    for b, L in enumerate(lens):
        solo = reference_gru_sequence(xg[b:b + 1, :L], w_hh, b_hh, h0[b:b + 1],
                                      gamma, beta, reverse)
        torch.testing.assert_close(h_all[b, :L], solo[0], rtol=1e-6, atol=1e-6)
        assert (h_all[b, L:] == 0).all()
        torch.testing.assert_close(out[b, :L], solo[0] @ w_head.t(),
                                   rtol=1e-5, atol=1e-6)
        assert (out[b, L:] == 0).all()
        last = solo[0, 0 if reverse else -1]
        torch.testing.assert_close(h_last[b], last, rtol=1e-6, atol=1e-6)

    # NaN poison in the padded x_gates changes nothing
    xp = xg.clone()
    for b, L in enumerate(lens):
        xp[b, L:] = float("nan")
    h_all_p = reference_gru_sequence(xp, w_hh, b_hh, h0, gamma, beta, reverse,
                                     lengths=lengths)
    out_p, h_last_p = fused_gru_decode(xp, w_hh, b_hh, h0, gamma, beta, w_head,
                                       reverse=reverse, lengths=lengths)
    assert torch.equal(h_all_p, h_all)
    assert torch.equal(out_p, out) and torch.equal(h_last_p, h_last)


def test_reference_gru_without_lengths_is_unchanged():
    from deeprest_amd.ops.gru import reference_gru_sequence

    xg, w_hh, b_hh, h0, gamma, beta, _ = _gru_inputs()
    full = torch.full((3,), 7, dtype=torch.int32)
    a = reference_gru_sequence(xg, w_hh, b_hh, h0, gamma, beta, True)
    b = reference_gru_sequence(xg, w_hh, b_hh, h0, gamma, beta, True, lengths=full)
    assert torch.equal(a, b)


# ---------------------------------------------------------------------- model
def _spec(n_components):
    from deeprest_amd.data.synthetic import SyntheticApp, SyntheticAppConfig
    from deeprest_amd.models.net import build_model_spec

    app = SyntheticApp(SyntheticAppConfig(
        n_apis=5, n_components=n_components, windows_per_day=120, n_days=1,
        seed=23))
    return build_model_spec(app.generate_featurized())


def _model(spec, seed=4, **kw):
    from deeprest_amd.models.net import DeepRestNet, DeepRestNetConfig

    torch.manual_seed(seed)
    return DeepRestNet(spec, DeepRestNetConfig(
        d_model=64, n_heads=2, n_layers=1, d_ff=128, hidden=128, comp_dim=16,
        dropout=0.0, **kw))


@pytest.fixture(scope="module")
def spec6():
    return _spec(6)


@pytest.mark.parametrize("fused_norm", [False, True])
def test_model_lengths_match_solo_forwards(spec6, fused_norm):
    model = _model(spec6, fused_residual_norm=fused_norm).eval()
    lens = [20, 1, 7, 13]
    gen = torch.Generator().manual_seed(9)
    x = torch.rand(4, 20, spec6.num_paths, generator=gen)
    for b, L in enumerate(lens):                 # finite garbage in the padding
        x[b, L:] = 50.0 * torch.randn(20 - L, spec6.num_paths, generator=gen)
    lengths = torch.tensor(lens, dtype=torch.int32)
    with torch.no_grad():
        out = model(x, lengths)
        for b, L in enumerate(lens):
            solo = model(x[b:b + 1, :L])
            torch.testing.assert_close(out[b, :L], solo[0], rtol=1e-5, atol=1e-5)
            assert (out[b, L:] == 0).all()
        # lengths=None is the model's plain forward
        assert torch.equal(model(x, None), model(x))


def test_model_lengths_are_inference_only(spec6):
    model = _model(spec6)
    x = torch.rand(2, 5, spec6.num_paths)
    lengths = torch.tensor([5, 2], dtype=torch.int32)
    model.train()
    with pytest.raises(ValueError):
        model(x, lengths)
    model.eval()
    with pytest.raises(ValueError):              # grad mode still on
        model(x, lengths)
    with torch.no_grad():
        with pytest.raises(ValueError):          # one length per sample
            model(x, torch.tensor([5], dtype=torch.int32))


# ------------------------------------------------------------------ predictor
def _predictor(spec, **kw):
    from deeprest_amd.data.windows import MinMaxScaler
    from deeprest_amd.serve.predictor import Predictor

    gen = np.random.default_rng(3)
    x_scaler = MinMaxScaler().fit(gen.random((50, spec.num_paths)) * 20.0, 100)
    # ranges that keep the denormalized values away from zero: the relative
    # comparisons below then measure the model, not the cancellation in
    # out * scale + min of an untrained net's near-zero outputs
    y_scalers = [MinMaxScaler(min_val=5.0 + m, max_val=7.0 + m)
                 for m in range(spec.num_metrics)]
    return Predictor(_model(spec), x_scaler, y_scalers, spec.metric_names,
                     device=torch.device("cpu"), **kw)


def test_predictor_ragged_matches_single_predicts(spec6):
    pred = _predictor(spec6, max_window=12, graph_batches=(4,))
    plain = _predictor(spec6)
    gen = np.random.default_rng(5)
    windows = [gen.random((T, spec6.num_paths)) * 20.0 for T in (12, 3, 1)]
    got = pred.predict_ragged(windows)
    assert len(got) == 3
    for w, g in zip(windows, got):
        ref = plain.predict(w[None])
        for name in spec6.metric_names:
            assert g[name].shape == (w.shape[0], 3)
            np.testing.assert_allclose(g[name], ref[name][0], rtol=1e-5)

    with pytest.raises(ValueError, match="13.*12"):
        pred.predict_ragged([gen.random((13, spec6.num_paths))])
    with pytest.raises(ValueError, match="13.*12"):
        pred.predict(gen.random((1, 13, spec6.num_paths)))


def test_predictor_padded_positions_are_nan(spec6):
    pred = _predictor(spec6, max_window=12)
    gen = np.random.default_rng(6)
    x = torch.from_numpy(gen.random((3, 9, spec6.num_paths)).astype(np.float32))
    lens = [9, 2, 5]
    out = pred.predict_tensor(x, torch.tensor(lens, dtype=torch.int32))
    short = pred.predict_tensor(x[:, :5])            # T < max_window, no lengths
    for name in spec6.metric_names:
        assert out[name].shape == (3, 9, 3) and short[name].shape == (3, 5, 3)
        assert np.isfinite(short[name]).all()
        for b, L in enumerate(lens):
            assert np.isfinite(out[name][b, :L]).all()
            assert np.isnan(out[name][b, L:]).all()
        np.testing.assert_allclose(out[name][2, :5], short[name][2], rtol=1e-5)


def test_predictor_oversize_batch_is_a_value_error(spec6):
    """n above the largest tier used to escape as StopIteration."""
    pred = _predictor(spec6, max_window=12, graph_batches=(4,))
    with pytest.raises(ValueError, match="5.*4"):
        pred._graph_for(5, 12, spec6.num_paths)
    with pytest.raises(ValueError, match="5.*4"):
        _predictor(spec6, graph_batches=(4,))._graph_for(5, 12, spec6.num_paths)


# -------------------------------------------------------------------- batcher
class _VarlenStub:
    """Encodes its inputs: out[i, t, :] = sum_p x[i, t, p], NaN where padded."""

    device = torch.device("cpu")

    def __init__(self, max_window):
        self.max_window = max_window
        self.calls = []
        self.lock = threading.Lock()

    def predict_tensor(self, x, lengths):
        with self.lock:
            self.calls.append((tuple(x.shape), lengths.tolist()))
        v = x.sum(dim=2, keepdim=True).expand(-1, -1, 3).clone().numpy()
        for i, L in enumerate(lengths.tolist()):
            v[i, L:] = np.nan
        return {"m0": v}


def _req(i):
    T = (2, 4, 5)[i % 3]
    return np.random.default_rng(100 + i).random((1 + i % 2, T, 6)).astype(np.float32)


def test_batcher_coalesces_mixed_window_lengths():
    from deeprest_amd.serve.batcher import MicroBatcher

    pred = _VarlenStub(max_window=5)
    b = MicroBatcher(pred, max_batch=64, max_wait_ms=50.0)
    results, errors = {}, {}

    def call(i, w):
        try:
            results[i] = b.predict(w)
        except Exception as e:  # noqa: BLE001
            errors[i] = e

    reqs = {i: _req(i) for i in range(8)}
    reqs[8] = np.zeros((1, 6, 6), dtype=np.float32)      # T = 6 > max_window
    threads = [threading.Thread(target=call, args=(i, w)) for i, w in reqs.items()]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=30)
    # the oversize request fails alone; everybody else completes
    assert list(errors) == [8] and isinstance(errors[8], ValueError)
    assert sorted(results) == list(range(8))
    assert len(pred.calls) < 8
    assert b.requests_served == 8
    assert any(len(set(lens)) > 1 for _, lens in pred.calls), "no mixed flush"
    for i in range(8):
        w = reqs[i]
        out = results[i]["m0"]
        assert out.shape == (w.shape[0], w.shape[1], 3)
        np.testing.assert_allclose(out[:, :, 0], w.sum(axis=2), rtol=1e-6)


def test_batcher_without_max_window_is_unchanged():
    from deeprest_amd.serve.batcher import MicroBatcher

    class Plain:
        def __init__(self):
            self.seen = []

        def predict(self, windows):
            w = np.asarray(windows)
            self.seen.append((w.shape, w.dtype))
            return {"m0": w.sum(axis=(1, 2), keepdims=True) + np.zeros((len(w), 1, 3))}

    pred = Plain()
    b = MicroBatcher(pred, max_batch=3, max_wait_ms=10_000.0)
    w = np.random.default_rng(0).random((3, 4, 5))
    out = b.predict(w)
    assert pred.seen == [((3, 4, 5), np.dtype("float64"))]
    np.testing.assert_allclose(out["m0"][:, 0, 0], w.sum(axis=(1, 2)), rtol=1e-12)
