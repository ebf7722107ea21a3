"""GPU tests of per-sample window lengths on the inference path: the
key-length mask of mha_fwd_kernel, the per-row lengths of the HEADS decode
kernel (ops.fused_gru_decode), the model's ``lengths`` argument, graph replay
with the lengths buffer rewritten in place, and the predictor's ``max_window``.

References are never the code under test: attention is checked against
``reference_mha`` in fp32 on each truncated sample; the GRU decode against
the EXISTING fixed-length decode kernel run on the whole batch truncated to
each length (same batch size, hence the same kernel variant) — holding a
state is exact and rows are independent, so the match is bit-for-bit; the
model against the CPU fp32 forward of each truncated sample with a bound
measured from the existing GPU path inside the test.
"""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

H = 128


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deeprest_amd.ops import native_available

    if not native_available():
        pytest.fail("HIP extension not built — GPU tests must not fall back")
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def _release_shared_cases():
    yield
    _gru_case.cache_clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def _i32(vals, dev):
    return torch.tensor(list(vals), dtype=torch.int32, device=dev)


# ------------------------------------------------------------------ attention
# (B, T, D, lengths), heads = 2
MHA_CASES = [
    (3, 70, 32, (70, 1, 33)),   # 3 key tiles, 2 query tiles, one key into tile 2
    (2, 32, 8, (32, 31)),       # exactly one key tile, one key short of it
    (2, 40, 64, (40, 5)),       # widest head
]


def _mha_inputs(B, T, D, dtype, dev):
    gen = torch.Generator().manual_seed(100 * B + T + D)
    return [torch.randn(B, 2, T, D, generator=gen).to(dev, dtype) for _ in range(3)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", MHA_CASES)
def test_mha_key_lengths(dev, case, dtype):
    from deeprest_amd.ops import mha_forward, reference_mha

    B, T, D, lens = case
    q, k, v = _mha_inputs(B, T, D, dtype, dev)
    lengths = _i32(lens, dev)
    with torch.no_grad():
        o = mha_forward(q, k, v, kv_lengths=lengths)
    assert o.shape == q.shape and o.dtype == dtype
    for b, L in enumerate(lens):
        ref = reference_mha(q[b:b + 1, :, :L].float(), k[b:b + 1, :, :L].float(),
                            v[b:b + 1, :, :L].float())
        # the tolerances of test_mha_forward_matches_reference (both dtypes)
        torch.testing.assert_close(o[b, :, :L].float(), ref[0], rtol=3e-2, atol=2e-2)
        assert (o[b, :, L:] == 0).all(), f"padded rows of sample {b} not zero"

    # NaN in every padded q/k/v position: bit-equal valid rows, zero padding
    qp, kp, vp = (t.clone() for t in (q, k, v))
    for b, L in enumerate(lens):
        for t in (qp, kp, vp):
            t[b, :, L:] = float("nan")
    with torch.no_grad():
        op = mha_forward(qp, kp, vp, kv_lengths=lengths)
    assert torch.equal(op, o)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_mha_lengths_are_clamped(dev, dtype):
    from deeprest_amd.ops import mha_forward

    B, T, D, _ = MHA_CASES[0]
    q, k, v = _mha_inputs(2, T, D, dtype, dev)
    with torch.no_grad():
        got = mha_forward(q, k, v, kv_lengths=_i32([0, T + 5], dev))
        neg = mha_forward(q, k, v, kv_lengths=_i32([-3, 2 ** 31 - 1], dev))
        want = mha_forward(q, k, v, kv_lengths=_i32([1, T], dev))
        full = mha_forward(q, k, v)
    assert torch.equal(got, want) and torch.equal(neg, want)
    # L = T is the unmasked computation (another instantiation: the
    # reference tolerances, not bit equality)
    torch.testing.assert_close(want[1].float(), full[1].float(), rtol=3e-2, atol=2e-2)


def test_mha_lengths_reject_grad_and_bad_lengths(dev):
    from deeprest_amd.ops import mha_forward
    from deeprest_amd.ops.native import require_native

    q, k, v = _mha_inputs(2, 32, 8, torch.float32, dev)
    good = _i32([32, 31], dev)
    q.requires_grad_(True)
    with pytest.raises(RuntimeError):
        mha_forward(q, k, v, kv_lengths=good)
    q = q.detach()
    ext = require_native("test")
    for bad in (good.long(), _i32([32], dev), good.cpu()):
        with pytest.raises(RuntimeError):
            ext.mha_forward(q, k, v, 0.5, bad)


# ----------------------------------------------------------------- gru decode
# (shape (B, T, C, O) from test_gru_decode_gpu.py's tables, lengths cycle)
GRU_CASES = [
    ((3, 7, 5, 9), (7, 1, 4)),          # one tile holding three lengths
    ((5, 4, 13, 9), (4, 1, 2, 3, 4)),   # ragged last tile
    ((3, 5, 4, 17), (5, 2, 1)),         # second N-tile of the head phase
    ((400, 3, 64, 9), (3, 1, 2)),       # 8-wave kernel
    ((3080, 2, 8, 15), (1, 2)),         # 8-wave, ragged tail block
]
FP8_CASES = GRU_CASES[:2]


def _gru_inputs(shape, dtype):
    B, T, C, O = shape
    gen = torch.Generator().manual_seed(1000 * B + 100 * T + 10 * C + O)
    mk = lambda *s: torch.randn(*s, generator=gen) * 0.4
    ins = [mk(B, T, 3 * H), mk(3 * H, H) / H ** 0.5, mk(3 * H) * 0.2,
           mk(B, C, H), 1.0 + 0.1 * mk(C, 3 * H), 0.1 * mk(C, 3 * H),
           mk(O, H) / H ** 0.5]
    return [t if i == 2 else t.to(dtype) for i, t in enumerate(ins)]


@functools.lru_cache(maxsize=None)
def _gru_case(shape, lens_cycle, reverse, dtype, fp8):
    """Inputs, per-sample lengths and the reference assembled from the
    existing fixed-length decode kernel, once per case: for each distinct
    length L the whole batch truncated to xg[:, :L] (same batch size: same
    kernel variant), of which the rows of length L are kept."""
    from deeprest_amd.ops import fused_gru_decode

    dev = torch.device("cuda:0")
    B, T, C, O = shape
    ins = [t.to(dev) for t in _gru_inputs(shape, dtype)]
    lens = torch.tensor([lens_cycle[b % len(lens_cycle)] for b in range(B)])
    ref_out = torch.zeros(B, T, C, O, device=dev, dtype=dtype)
    ref_h = torch.zeros(B, C, H, device=dev, dtype=dtype)
    with torch.no_grad():
        for L in sorted(set(lens_cycle)):
            out_L, h_L = fused_gru_decode(ins[0][:, :L].contiguous(), *ins[1:],
                                          reverse=reverse, fp8=fp8)
            rows = (lens == L).to(dev)
            ref_out[rows, :L] = out_L[rows]
            ref_h[rows] = h_L[rows]
    return ins, lens, ref_out, ref_h


def _run_gru_case(shape, lens_cycle, reverse, dtype, fp8, dev):
    from deeprest_amd.ops import fused_gru_decode

    ins, lens, ref_out, ref_h = _gru_case(shape, lens_cycle, reverse, dtype, fp8)
    T = shape[1]
    lengths = lens.to(dev, torch.int32)
    what = f"{shape} {lens_cycle} rev={reverse} {dtype} fp8={fp8}"
    with torch.no_grad():
        out, h_last = fused_gru_decode(*ins, reverse=reverse, fp8=fp8,
                                       lengths=lengths)
    assert out.dtype == dtype and out.is_contiguous(), what
    valid = (torch.arange(T)[None, :] < lens[:, None]).to(dev)
    assert (out[~valid] == 0).all(), f"{what}: padded out not zero"
    assert torch.equal(out, ref_out), f"{what}: out differs from the fixed-length kernel"
    assert torch.equal(h_last, ref_h), f"{what}: h_last differs"

    # NaN in every padded x_gates row: everything bit-equal
    xp = ins[0].clone()
    xp[~valid] = float("nan")
    with torch.no_grad():
        out_p, h_p = fused_gru_decode(xp, *ins[1:], reverse=reverse, fp8=fp8,
                                      lengths=lengths)
    assert torch.equal(out_p, out) and torch.equal(h_p, h_last), f"{what}: poison leaked"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("case", GRU_CASES)
def test_gru_decode_lengths_match_fixed_length_kernel(dev, case, reverse, dtype):
    _run_gru_case(case[0], case[1], reverse, dtype, False, dev)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("case", FP8_CASES)
def test_gru_decode_lengths_fp8_match_fixed_length_kernel(dev, case, reverse, dtype):
    _run_gru_case(case[0], case[1], reverse, dtype, True, dev)


@pytest.mark.parametrize("reverse", [False, True])
def test_gru_decode_lengths_are_clamped(dev, reverse):
    from deeprest_amd.ops import fused_gru_decode

    shape = GRU_CASES[0][0]
    T = shape[1]
    ins = [t.to(dev) for t in _gru_inputs(shape, torch.float32)]
    with torch.no_grad():
        want = fused_gru_decode(*ins, reverse=reverse, lengths=_i32([1, T, 1], dev))
        got = fused_gru_decode(*ins, reverse=reverse,
                               lengths=_i32([0, T + 5, -2 ** 31], dev))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_gru_decode_binding_rejects_bad_lengths(dev):
    from deeprest_amd.ops.native import require_native

    ext = require_native("test")
    xg, w_hh, b_hh, h0, gamma, beta, _ = [
        t.to(dev) for t in _gru_inputs((2, 2, 3, 9), torch.float32)]
    img = torch.zeros(32, H, device=dev, dtype=torch.bfloat16)
    args = (xg, w_hh, b_hh, h0, gamma, beta, img, 9, False, False)
    good = _i32([2, 1], dev)
    ext.gru_seq_decode(*args, good)
    for bad in (good.long(), _i32([2, 1, 1], dev), good.cpu()):
        with pytest.raises(RuntimeError):
            ext.gru_seq_decode(*args, bad)


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
        dropout=0.0, **kw)).eval()


@pytest.fixture(scope="module")
def spec6():
    return _spec(6)


@pytest.fixture
def decode_calls(monkeypatch):
    from deeprest_amd.models import net

    calls = []
    real = net.fused_gru_decode

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(net, "fused_gru_decode", counted)
    return calls


MODEL_LENS = (40, 1, 17, 33)


def _model_inputs(spec, T=40, lens=MODEL_LENS):
    gen = torch.Generator().manual_seed(12)
    x = torch.rand(len(lens), T, spec.num_paths, generator=gen)
    for b, L in enumerate(lens):                 # finite garbage in the padding
        x[b, L:] = 50.0 * torch.randn(T - L, spec.num_paths, generator=gen)
    return x


@pytest.mark.parametrize("flags", [dict(fused_residual_norm=True),
                                   dict(fp8_inference=True)],
                         ids=["fused_norm", "fp8"])
def test_model_lengths_match_cpu_oracle(dev, spec6, decode_calls, flags):
    """|model_gpu(x, lengths)[b, :L] - ref_b| <= 2 * d0 + 1e-6, where ref_b is
    the CPU fp32 forward of the truncated sample and d0 the largest error of
    the EXISTING GPU path (the solo forward of each truncated sample, same
    flags) against it: bf16 operand rounding flips are independent between
    two GPU runs, hence the factor 2."""
    cpu = _model(spec6, **flags)
    gpu = _model(spec6, **flags).to(dev)
    gpu.load_state_dict(cpu.state_dict())
    assert not gpu.cfg.fused_head_decode
    x = _model_inputs(spec6)
    xd = x.to(dev)
    with torch.no_grad():
        refs = [cpu(x[b:b + 1, :L])[0] for b, L in enumerate(MODEL_LENS)]
        solos = [gpu(xd[b:b + 1, :L])[0].cpu() for b, L in enumerate(MODEL_LENS)]
        assert len(decode_calls) == 0
        out = gpu(xd, _i32(MODEL_LENS, dev)).cpu()
    assert len(decode_calls) == 2                # one per direction
    d0 = max((s - r).abs().max().item() for s, r in zip(solos, refs))
    err = max((out[b, :L] - refs[b]).abs().max().item()
              for b, L in enumerate(MODEL_LENS))
    print(f"{flags}: d0 (solo GPU vs CPU) {d0:.3e}, lengths GPU vs CPU {err:.3e}, "
          f"bound {2 * d0 + 1e-6:.3e}")
    assert err <= 2 * d0 + 1e-6
    for b, L in enumerate(MODEL_LENS):
        assert (out[b, L:] == 0).all()


def test_graph_replay_with_rewritten_lengths(dev, spec6):
    model = _model(spec6).to(dev)
    gin = _model_inputs(spec6).to(dev)
    glen = _i32(MODEL_LENS, dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for _ in range(2):
            model(gin, glen)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s), torch.no_grad():
        gout = model(gin, glen)
    for lens in (MODEL_LENS, (5, 40, 40, 2)):
        glen.copy_(_i32(lens, dev))
        g.replay()
        got = gout.clone()
        with torch.no_grad():
            eager = model(gin, glen)
        torch.testing.assert_close(got, eager, rtol=2e-4, atol=2e-4)
        for b, L in enumerate(lens):
            assert (got[b, L:] == 0).all()
            assert got[b, :L].abs().sum() > 0


def test_predictor_max_window_serves_every_length_from_one_graph(dev, spec6):
    """predict_ragged against per-window predict of a max_window=None
    predictor, with the model test's bound: d0 is the existing predictor's
    error against the CPU predictor on the same windows."""
    from deeprest_amd.data.windows import MinMaxScaler
    from deeprest_amd.serve.predictor import Predictor

    gen = np.random.default_rng(3)
    x_scaler = MinMaxScaler().fit(gen.random((50, spec6.num_paths)) * 20.0, 100)
    y_scalers = [MinMaxScaler(min_val=5.0 + m, max_val=7.0 + m)
                 for m in range(spec6.num_metrics)]
    mk = lambda device, **kw: Predictor(
        _model(spec6), x_scaler, y_scalers, spec6.metric_names, device=device,
        graph_batches=(4,), **kw)
    varlen = mk(dev, max_window=24)
    plain = mk(dev)
    oracle = mk(torch.device("cpu"))
    windows = [gen.random((T, spec6.num_paths)) * 20.0 for T in (24, 3, 1, 10)]
    got = varlen.predict_ragged(windows)
    d0 = err = 0.0
    for w, g in zip(windows, got):
        ref = oracle.predict(w[None])
        solo = plain.predict(w[None])
        for name in spec6.metric_names:
            assert g[name].shape == (w.shape[0], 3)
            d0 = max(d0, np.abs(solo[name][0] - ref[name][0]).max())
            err = max(err, np.abs(g[name] - ref[name][0]).max())
    print(f"predictor: d0 {d0:.3e}, ragged vs CPU {err:.3e}")
    assert err <= 2 * d0 + 1e-6
    assert varlen.captured_batches == [4]
    assert len(varlen._graphs) == 1              # three T's, one graph
    short = varlen.predict(windows[3][None])     # rectangular, T < max_window
    for name in spec6.metric_names:
        np.testing.assert_allclose(short[name][0], got[3][name], rtol=1e-4)
    assert len(varlen._graphs) == 1
    with pytest.raises(ValueError, match="25.*24"):
        varlen.predict(gen.random((1, 25, spec6.num_paths)))
