"""GPU tests of the sanity-check kernel (csrc/sanity.hip, ops.band_scores)
and of ``Predictor.sanity_check`` on the device.

Oracle: ``reference_band_scores`` in float64 on the same inputs.  Flags and
the integer summaries must be exact; the inputs make that a fair demand —
``measured`` is ``q2 + k * band`` on the float64 reference bands with k from
{-0.5, 0, thr/4, 2 thr, 5 thr}, so that every observed score is at most thr/2
or at least 2 thr (asserted on the reference before anything is compared; the
f32 rounding of ``measured`` is directed away from the threshold so that this
holds by construction).

Scores, bands and max_score: ``|kernel - ref64| <= 2 * d0 + 1e-6`` with d0 the
largest error against ref64 of the existing f32 route — the same steps as
torch ops in f32 on the device, i.e. ``reference_band_scores`` run in f32 on
the GPU — taken per output (scores and max_score are O(1), bands are in raw
units).  The factor 2 is the practice of tests/test_varlen_gpu.py: two f32
evaluations round independently.
"""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

THR = 0.25
DEV = "cuda:0"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deeprest_amd.ops import native_available

    if not native_available():
        pytest.fail("HIP extension not built — GPU tests must not fall back")
    return torch.device(DEV)


@pytest.fixture(scope="module", autouse=True)
def _release_shared_cases():
    yield
    _case.cache_clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def _measured_on_margin(q0, q2, gen, thr=THR, gaps=0.1):
    """float64 bands -> f32 measured = q2 + k * band, k in runs of random
    length (short and long runs both occur), rounded to f32 away from the
    threshold, with a share of gaps (NaN, +Inf, -Inf)."""
    shape = q2.shape
    N, T, M = shape
    ks = torch.tensor((-0.5, 0.0, thr / 4, 2 * thr, 5 * thr), dtype=torch.float64)
    # a fresh draw every 1..4 steps decides hot / calm for the steps it covers
    hot = torch.rand(N, T, M, generator=gen) < 0.5
    keep = torch.rand(N, T, M, generator=gen) < 0.6        # repeat the previous step
    for t in range(1, T):
        hot[:, t] = torch.where(keep[:, t], hot[:, t - 1], hot[:, t])
    pick_hot = torch.randint(3, 5, shape, generator=gen)
    pick_calm = torch.randint(0, 3, shape, generator=gen)
    k = ks[torch.where(hot, pick_hot, pick_calm)].to(q2.device)
    hot = hot.to(q2.device)
    y64 = q2 + k * (q2 - q0).clamp(min=1e-9)
    y = y64.float()
    inf = torch.full_like(y, float("inf"))
    up = torch.nextafter(torch.nextafter(y, inf), inf)
    down = torch.nextafter(torch.nextafter(y, -inf), -inf)
    y = torch.where(hot, up, down)
    gap = (torch.rand(N, T, M, generator=gen) < gaps).to(q2.device)
    kind = torch.randint(0, 3, shape, generator=gen).to(q2.device)
    garbage = torch.where(kind == 0, torch.full_like(y, float("nan")),
                          torch.where(kind == 1, inf, -inf))
    return torch.where(gap, garbage, y), gap


def _assert_on_margin(ref64, thr=THR):
    s = ref64.scores[torch.isfinite(ref64.scores)]
    assert s.numel() > 0
    assert ((s <= thr / 2) | (s >= 2 * thr)).all(), "inputs off the margin"


# (N, T, M), lengths
SHAPES = [
    ((3, 7, 5), None),
    ((2, 1, 67), None),                                # T = 1, two waves
    ((5, 33, 130), (33, 1, 17, 40, 0)),                # clamped both ways
    ((5, 33, 130), None),
]
# base, conformal, log1p
VARIANTS = [(True, True, True), (False, False, False), (True, False, True),
            (False, True, False)]


@functools.lru_cache(maxsize=None)
def _case(shape, lens, variant, bf16):
    """Inputs of one case on the device; the float64 bands measured is built
    from come from one reference call (min_run does not enter the bands)."""
    from deeprest_amd.ops import reference_band_scores

    dev = torch.device(DEV)
    N, T, M = shape
    base_on, conf_on, log1p = variant
    gen = torch.Generator().manual_seed(1000 * N + 10 * T + M + 7 * sum(variant))
    if bf16:
        # multiples of 1/8, exact in bf16: triples at least 0.125 apart
        centre = torch.randint(-16, 17, (N, T, M, 1), generator=gen) / 8.0
        lo = torch.randint(1, 5, (N, T, M, 1), generator=gen) / 8.0
        hi = torch.randint(1, 5, (N, T, M, 1), generator=gen) / 8.0
    else:
        centre = torch.randn(N, T, M, 1, generator=gen)
        lo = 0.1 + 0.5 * torch.rand(N, T, M, 1, generator=gen)
        hi = 0.1 + 0.5 * torch.rand(N, T, M, 1, generator=gen)
    triple = torch.cat((centre - lo, centre, centre + hi), dim=-1)
    order = torch.rand(N, T, M, 3, generator=gen).argsort(dim=-1)   # unsorted input
    out = triple.gather(-1, order).to(torch.bfloat16 if bf16 else torch.float32)
    assert torch.equal(out.float().sort(-1).values, triple.float()) or not bf16
    # log1p targets live in log space: keep exp's argument in a sane range
    y_min = torch.rand(M, generator=gen) * (2.0 if log1p else 10.0)
    y_scale = 0.5 + torch.rand(M, generator=gen) * (1.5 if log1p else 5.0)
    y_min[0], y_scale[0] = 0.0, 1.0                    # the identity scaler
    base = 0.5 * torch.randn(N, T, M, generator=gen) if base_on else None
    conf = (torch.rand(M, generator=gen) * 0.25 - 0.05) if conf_on else None
    to = lambda t: None if t is None else t.to(dev)
    out, y_min, y_scale, base, conf = map(to, (out, y_min, y_scale, base, conf))
    lengths = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
    d = lambda t: None if t is None else t.double()
    bands64 = reference_band_scores(
        out, torch.zeros(N, T, M, dtype=torch.float64, device=dev), d(y_min),
        d(y_scale), base=d(base), conformal=d(conf), log1p=log1p,
        want_bands=True).bands
    y, gap = _measured_on_margin(bands64[..., 0], bands64[..., 2], gen)
    return dict(out=out, y=y, gap=gap, y_min=y_min, y_scale=y_scale, base=base,
                conf=conf, log1p=log1p, lengths=lengths)


def _run(fn, c, dtype, min_run, **over):
    cast = lambda t: None if t is None else t.to(dtype)
    kw = dict(base=cast(c["base"]), conformal=cast(c["conf"]), log1p=c["log1p"],
              lengths=c["lengths"], threshold=THR, min_run=min_run, want_bands=True)
    out, y = over.pop("out", c["out"]), over.pop("y", c["y"])
    kw.update(over)
    return fn(out, cast(y), cast(c["y_min"]), cast(c["y_scale"]), **kw)


def _max_err(a, b):
    """largest |a - b| over the positions where b is finite; the NaN pattern
    must be the same."""
    fin = torch.isfinite(b)
    assert torch.equal(torch.isnan(a), torch.isnan(b)), "NaN pattern differs"
    if not fin.any():
        return 0.0
    return (a.double()[fin] - b[fin]).abs().max().item()


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("variant", VARIANTS,
                         ids=["base+conf+log1p", "plain", "base+log1p", "conf"])
@pytest.mark.parametrize("shape,lens", SHAPES,
                         ids=["3x7x5", "2x1x67", "5x33x130-lengths", "5x33x130"])
def test_kernel_matches_float64_reference(dev, shape, lens, variant, bf16):
    from deeprest_amd.ops import band_scores, reference_band_scores

    c = _case(shape, lens, variant, bf16)
    T = shape[1]
    flagged = 0
    for min_run in (1, 3, T + 1):
        ref64 = _run(reference_band_scores, c, torch.float64, min_run)
        _assert_on_margin(ref64)
        ref32 = _run(reference_band_scores, c, torch.float32, min_run)
        got = _run(band_scores, c, torch.float32, min_run)
        what = f"{shape} lens={lens} {variant} bf16={bf16} min_run={min_run}"
        assert got.scores.dtype == torch.float32 and got.flags.dtype == torch.uint8
        assert got.bands.shape == (*shape, 3) and got.flags.shape == shape
        # the existing f32 route agrees on the flags too (the margin is fair)
        assert torch.equal(ref32.flags, ref64.flags), what
        assert torch.equal(got.flags, ref64.flags), f"{what}: flags"
        for name in ("n_flagged", "first_flag", "n_observed"):
            g = getattr(got, name)
            assert g.dtype == torch.int32
            assert torch.equal(g, getattr(ref64, name)), f"{what}: {name}"
        for name in ("scores", "bands", "max_score"):
            d0 = _max_err(getattr(ref32, name), getattr(ref64, name))
            err = _max_err(getattr(got, name), getattr(ref64, name))
            print(f"{what}: {name} d0 {d0:.3e} kernel {err:.3e} "
                  f"bound {2 * d0 + 1e-6:.3e}")
            assert err <= 2 * d0 + 1e-6, f"{what}: {name} err {err:.3e}, d0 {d0:.3e}"
        flagged += int(ref64.n_flagged.sum())
        if min_run == T + 1:
            assert not got.flags.any() and (got.first_flag == -1).all()
    if T >= 3:
        assert flagged > 0, "the case must flag something"
    # without bands: the same everything else, and no bands
    lean = _run(band_scores, c, torch.float32, 3, want_bands=False)
    full = _run(band_scores, c, torch.float32, 3)
    assert lean.bands is None
    for name in ("scores", "flags", "max_score", "n_flagged", "first_flag", "n_observed"):
        assert torch.equal(getattr(lean, name).view(torch.uint8),
                           getattr(full, name).view(torch.uint8)), name


def _bits(t):
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape,lens", [SHAPES[2], ((3, 7, 5), (7, 2, 4))],
                         ids=["5x33x130", "3x7x5"])
def test_garbage_in_padding_and_gaps_reaches_nothing(dev, shape, lens, bf16):
    """NaN and Inf at every padded position of out, base and measured, and in
    measured at the gaps, against zeros at the padded positions (and plain
    NaN at the gaps): every output bit-identical."""
    from deeprest_amd.ops import band_scores

    c = _case(shape, lens, VARIANTS[0], bf16)
    N, T, M = shape
    L = c["lengths"].clamp(1, T)
    pad = (torch.arange(T, device=dev)[None, :] >= L[:, None])       # (N, T)
    assert pad.any() and c["gap"].any()
    nan = float("nan")

    def variant_of(fill_out, fill_base, fill_y, gap_fill):
        out, base, y = c["out"].clone(), c["base"].clone(), c["y"].clone()
        out[pad] = fill_out
        base[pad] = fill_base
        if gap_fill is not None:
            y = torch.where(c["gap"], torch.full_like(y, gap_fill), y)
        y[pad] = fill_y
        cc = dict(c, out=out, base=base, y=y)
        return _run(band_scores, cc, torch.float32, 3)

    clean = variant_of(0.0, 0.0, 0.0, nan)
    assert clean.flags.any()
    for fills in ((nan, float("inf"), float("-inf"), None),
                  (float("inf"), nan, nan, float("inf")),
                  (float("-inf"), float("-inf"), float("inf"), float("-inf"))):
        dirty = variant_of(*fills)
        for name in ("scores", "flags", "max_score", "n_flagged", "first_flag",
                     "n_observed", "bands"):
            assert torch.equal(_bits(getattr(dirty, name)), _bits(getattr(clean, name))), \
                f"{fills}: {name} changed"
    # what the padding holds by definition
    assert torch.isnan(clean.scores[pad]).all() and torch.isnan(clean.bands[pad]).all()
    assert not clean.flags[pad].any()
    assert torch.isnan(clean.scores[c["gap"]]).all() and not clean.flags[c["gap"]].any()


def test_bad_input_is_an_exception_not_a_launch(dev):
    from deeprest_amd.ops import band_scores
    from deeprest_amd.ops.native import require_native

    ext = require_native("test")
    N, T, M = 2, 4, 3
    out = torch.zeros(N, T, M, 3, device=dev)
    y = torch.zeros(N, T, M, device=dev)
    mn, sc = torch.zeros(M, device=dev), torch.ones(M, device=dev)
    good = torch.tensor([4, 2], dtype=torch.int32, device=dev)
    args = lambda o=out, lengths=good, min_run=3: (
        o, y, mn, sc, None, None, False, lengths, THR, min_run, False)
    ext.band_scores(*args())
    bad_q = torch.zeros(N, T, M, 2, device=dev)
    for a in (args(o=bad_q), args(min_run=0), args(lengths=good.long()),
              args(lengths=good[:1].contiguous()), args(lengths=good.cpu()),
              args(lengths=good.reshape(2, 1)), args(o=out.double())):
        with pytest.raises((RuntimeError, TypeError)):
            ext.band_scores(*a)
    with pytest.raises((RuntimeError, TypeError)):
        ext.band_scores(out, y[:, :3].contiguous(), mn, sc, None, None, False,
                        None, THR, 3, False)
    # the op says the same in its own words, before it gets that far
    with pytest.raises(ValueError, match="Q must be 3"):
        band_scores(bad_q, y, mn, sc)
    with pytest.raises(ValueError, match="min_run"):
        band_scores(out, y, mn, sc, min_run=0)
    for bad in (good.long(), good[:1], good.cpu()):
        with pytest.raises(ValueError, match="lengths"):
            band_scores(out, y, mn, sc, lengths=bad)


# ------------------------------------------------------------ through the model
def _spec(n_components):
    from deeprest_amd.data.synthetic import SyntheticApp, SyntheticAppConfig
    from deeprest_amd.models.net import build_model_spec

    app = SyntheticApp(SyntheticAppConfig(
        n_apis=5, n_components=n_components, windows_per_day=120, n_days=1,
        seed=23))
    return build_model_spec(app.generate_featurized())


def _model(spec, seed=4):
    from deeprest_amd.models.net import DeepRestNet, DeepRestNetConfig

    torch.manual_seed(seed)
    return DeepRestNet(spec, DeepRestNetConfig(
        d_model=64, n_heads=2, n_layers=1, d_ff=128, hidden=128, comp_dim=16,
        dropout=0.0)).eval()


def test_predictor_sanity_check_on_the_device(dev):
    """sanity_check == predict_ragged -> AnomalyScorer on the same GPU
    predictor, flags exact (measured on the margin of that predictor's own
    bands); a second request of other lengths replays the same graph."""
    from deeprest_amd.data.windows import MinMaxScaler
    from deeprest_amd.serve.anomaly import AnomalyScorer
    from deeprest_amd.serve.predictor import Predictor

    spec = _spec(6)
    names, P, M = spec.metric_names, spec.num_paths, spec.num_metrics
    rng = np.random.default_rng(3)
    x_scaler = MinMaxScaler().fit(rng.random((50, P)) * 20.0, 100)
    y_scalers = [MinMaxScaler(min_val=5.0 + m, max_val=7.0 + m) for m in range(M)]
    y_scalers[2] = MinMaxScaler(min_val=4.0, max_val=4.0)          # scale 0
    pred = Predictor(_model(spec), x_scaler, y_scalers, names, device=dev,
                     graph_batches=(4,), max_window=24,
                     residual_ridge=rng.normal(0, 0.02, (P + 1, M)),
                     conformal=rng.uniform(0.01, 0.05, M))
    scorer = AnomalyScorer(threshold=THR, min_run=3)
    gen = torch.Generator().manual_seed(11)
    graphs = None
    for lens in ((24, 3, 1, 10), (7, 24, 12, 2)):
        windows = [rng.random((T, P)) * 20.0 for T in lens]
        bands = pred.predict_ragged(windows)
        W = max(lens)
        x = np.zeros((len(lens), W, P), dtype=np.float32)
        y = np.full((len(lens), W, M), np.nan, dtype=np.float32)   # padding: NaN
        for i, (w, b) in enumerate(zip(windows, bands)):
            x[i, : lens[i]] = w
            q = torch.from_numpy(np.stack([b[k] for k in names], axis=1)).double()
            yi, _ = _measured_on_margin(q[None, :, :, 0], q[None, :, :, 2], gen)
            # the host scorer knows NaN gaps only (an Inf is a value to it)
            y[i, : lens[i]] = torch.nan_to_num(yi[0], nan=np.nan, posinf=np.nan,
                                               neginf=np.nan).numpy()
        check = pred.sanity_check(x, y, threshold=THR, min_run=3, lengths=lens,
                                  detail=True)
        if graphs is None:
            graphs = len(pred._graphs)
            assert graphs == 1
        assert len(pred._graphs) == graphs
        flagged = 0
        for i, b in enumerate(bands):
            want = scorer.score_all(
                {k: y[i, : lens[i], m].astype(np.float64) for m, k in enumerate(names)}, b)
            got = check.reports(i)
            for m, k in enumerate(names):
                obs = np.isfinite(y[i, : lens[i], m])
                s = want[k].scores[obs]
                assert ((s <= THR / 2) | (s >= 2 * THR)).all(), "inputs off the margin"
                assert np.array_equal(got[k].flags, want[k].flags), (lens, i, k)
                assert got[k].windows == want[k].windows
                assert check.n_flagged[i, m] == want[k].flags.sum()
                assert check.n_observed[i, m] == obs.sum()
                assert bool(check.anomalous[i, m]) == want[k].is_anomalous
                flagged += int(want[k].flags.sum())
        assert flagged > 0
        for i, L in enumerate(lens):
            assert torch.isnan(check.scores[i, L:]).all()
            assert torch.isnan(check.bands[i, L:]).all() and not check.flags[i, L:].any()
