"""The bindings' side of the kernel entry contract (docs/KERNELS.md, "Entry
contract"): a bad operand is an exception that names the operand, raised
before anything is launched, and an empty problem returns its empty result
without a launch.

Every rejected operand here would stay inside its allocations even if its
check were missing and the kernel ran: a wrong dtype of the same element size
(int32 for f32, f16 for bf16), an operand with MORE elements than wanted, or a
non-contiguous view covering the same storage.  CPU tensors, short operands
and other devices are not tried on purpose.

That valid calls still compute the same is what the ops' own test files check
at these and larger sizes (test_ops_gpu.py, test_residual_norm_gpu.py,
test_masked_pinball_gpu.py, test_gru_heads_gpu.py, test_mha_packed_gpu.py,
test_adam_gpu.py, test_sanity_gpu.py); only the call that follows the empty
attention problem is repeated here.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deeprest_amd.ops import native_available

    if not native_available():
        pytest.fail("HIP extension not built — GPU tests must not fall back")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ext(dev):
    from deeprest_amd.ops.native import require_native

    return require_native("test")


def _rejects(fn, good, cases):
    """fn(**good) with one operand replaced at a time must raise and name it."""
    for operand, bad, match in cases:
        with pytest.raises(RuntimeError, match=match):
            fn(**{**good, operand: bad})
    torch.cuda.synchronize()      # nothing was launched, nothing is pending


def _i32(t):
    return torch.zeros(t.shape, dtype=torch.int32, device=t.device)


def _more(t, dim=0):
    """Same rank and dtype, one more slice along `dim`."""
    shape = list(t.shape)
    shape[dim] += 1
    return torch.zeros(shape, dtype=t.dtype, device=t.device)


def _strided(t):
    """t's shape over a transposed buffer: same storage size, not contiguous."""
    assert t.dim() >= 2 and t.shape[-1] != 1 and t.shape[-2] != 1
    shape = list(t.shape)
    shape[-1], shape[-2] = shape[-2], shape[-1]
    v = torch.zeros(shape, dtype=t.dtype, device=t.device).transpose(-1, -2)
    assert v.shape == t.shape and not v.is_contiguous()
    return v


# ------------------------------------------------------------------ attention
def _mha_operands(dev):
    B, H, T, D = 1, 1, 8, 8
    torch.manual_seed(0)
    mk = lambda: torch.randn(B, H, T, D, device=dev)
    return dict(q=mk(), k=mk(), v=mk(), o=mk(), dout=mk(),
                lse=torch.zeros(B, H, T, device=dev))


def test_mha_forward_rejects_bad_k_v(dev, ext):
    t = _mha_operands(dev)
    good = dict(q=t["q"], k=t["k"], v=t["v"])
    fn = lambda q, k, v: ext.mha_forward(q, k, v, 0.5)
    fn(**good)
    _rejects(fn, good, [
        ("q", _i32(t["q"]), "q must be bf16 or f32"),
        ("q", _strided(t["q"]), "q must be a contiguous"),
        ("k", _i32(t["k"]), "mha k must be"),
        ("k", _strided(t["k"]), "mha k must be contiguous"),
        ("k", _more(t["k"], 2), "mha k must have shape"),
        ("v", _i32(t["v"]), "mha v must be"),
        ("v", _strided(t["v"]), "mha v must be contiguous"),
        ("v", _more(t["v"], 0), "mha v must have shape"),
    ])


def test_mha_backward_rejects_bad_operands(dev, ext):
    good = _mha_operands(dev)
    fn = lambda q, k, v, o, dout, lse: ext.mha_backward(q, k, v, o, dout, lse, 0.5)
    fn(**good)
    cases = [("q", _i32(good["q"]), "q must be bf16 or f32"),
             ("q", _strided(good["q"]), "q must be a contiguous"),
             ("lse", _i32(good["lse"]), "mha lse must be"),
             ("lse", _more(good["lse"], 2), "mha lse must have shape")]
    for name in ("k", "v", "o", "dout"):
        cases += [(name, _i32(good[name]), f"mha {name} must be"),
                  (name, _strided(good[name]), f"mha {name} must be contiguous"),
                  (name, _more(good[name], 2), f"mha {name} must have shape")]
    _rejects(fn, good, cases)


def test_mha_empty_batch_returns_empty_without_a_launch(dev):
    """B == 0 used to launch a grid with y == 0; the refusal went unread and
    stayed behind as the runtime's last error."""
    from deeprest_amd.ops import mha_forward, reference_mha

    H, T, D = 2, 8, 8
    q0 = torch.empty(0, H, T, D, device=dev, requires_grad=True)
    k0, v0 = torch.empty_like(q0), torch.empty_like(q0)
    o0 = mha_forward(q0, k0, v0)
    assert o0.shape == (0, H, T, D)
    o0.backward(torch.empty_like(o0))
    assert q0.grad.shape == (0, H, T, D)
    torch.cuda.synchronize()

    torch.manual_seed(6)
    q, k, v = (torch.randn(1, H, T, D, device=dev) for _ in range(3))
    o = mha_forward(q, k, v)
    torch.cuda.synchronize()
    # tolerance of test_ops_gpu.test_mha_forward_matches_reference
    torch.testing.assert_close(o, reference_mha(q, k, v), rtol=3e-2, atol=2e-2)


# -------------------------------------------------------------------- pinball
def _pinball_operands(dev):
    torch.manual_seed(1)
    return dict(grad=torch.ones((), device=dev),
                outputs=torch.randn(1, 2, 3, 3, device=dev),
                labels=torch.randn(1, 2, 3, device=dev),
                q=torch.tensor([0.05, 0.5, 0.95], device=dev))


def _pinball_cases(t):
    return [
        ("outputs", _i32(t["outputs"]), "pinball outputs must be bf16 or f32"),
        ("outputs", _strided(t["outputs"]), "pinball outputs must be a contiguous"),
        ("labels", _i32(t["labels"]), "pinball labels must be"),
        ("labels", _more(t["labels"], 2), "pinball labels must have 6 elements"),
        # (2, 3): the right count in another rank is fine, its strides are not
        ("labels", _strided(t["labels"][0]), "pinball labels must be contiguous"),
        ("q", _i32(t["q"]), "pinball quantiles must be"),
        ("q", _more(t["q"]), "pinball quantiles must have 3 elements"),
    ]


def test_pinball_forward_rejects_bad_operands(dev, ext):
    t = _pinball_operands(dev)
    good = {k: t[k] for k in ("outputs", "labels", "q")}
    fn = lambda outputs, labels, q: ext.pinball_forward(outputs, labels, q)
    # any rank of labels with one entry per output row is accepted
    torch.testing.assert_close(fn(**good),
                               fn(t["outputs"], t["labels"].reshape(6), t["q"]))
    _rejects(fn, good, _pinball_cases(t))


def test_pinball_backward_rejects_bad_operands(dev, ext):
    good = _pinball_operands(dev)
    fn = lambda grad, outputs, labels, q: ext.pinball_backward(grad, outputs, labels, q)
    assert fn(**good).shape == good["outputs"].shape
    _rejects(fn, good, _pinball_cases(good) + [
        ("grad", _i32(good["grad"]), "pinball grad must be"),
        ("grad", torch.ones(2, device=dev), "pinball grad must have 1 elements"),
    ])


# ----------------------------------------------------------------- layer norm
def test_dropout_add_ln_backward_rejects_bad_operands(dev, ext):
    torch.manual_seed(2)
    x = torch.randn(4, 8, device=dev)
    w, b = torch.ones(8, device=dev), torch.zeros(8, device=dev)
    _, _, mean, rstd = ext.dropout_add_ln_forward(None, x, w, b, None, 0.0, 1e-5)
    good = dict(d_normed=torch.randn_like(x), d_r_out=torch.randn_like(x),
                r_out=x, weight=w, mean=mean, rstd=rstd)
    fn = lambda **t: ext.dropout_add_ln_backward(
        t["d_normed"], t["d_r_out"], t["r_out"], t["weight"], t["mean"],
        t["rstd"], None, 0.0)
    fn(**good)
    fn(**{**good, "d_r_out": None})          # plain layer norm
    cases = [("r_out", _i32(x), "r_out must be bf16 or f32")]
    for name in ("d_normed", "d_r_out"):
        cases += [(name, _i32(x), f"{name} must be"),
                  (name, _strided(x), f"{name} must be contiguous"),
                  (name, _more(x), f"{name} must have shape")]
    for name, label in (("weight", "layer_norm weight"), ("mean", "layer_norm mean"),
                        ("rstd", "layer_norm rstd")):
        cases += [(name, _i32(good[name]), f"{label} must be"),
                  (name, _more(good[name]), f"{label} must have . elements")]
    _rejects(fn, good, cases)


# ------------------------------------------------------------------------ gru
def test_gru_backward_bindings_reject_bad_operands(dev, ext):
    from deeprest_amd.ops import gru as gru_mod

    B, T, C, H, O = 1, 1, 3, 128, 9
    torch.manual_seed(3)
    xg = torch.randn(B, T, 3 * H, device=dev) * 0.5
    w_hh = torch.randn(3 * H, H, device=dev) / np.sqrt(H)
    b_hh = torch.randn(3 * H, device=dev) * 0.1
    h0 = torch.randn(B, C, H, device=dev) * 0.3
    gamma = 1.0 + 0.1 * torch.randn(C, 3 * H, device=dev)
    beta = 0.1 * torch.randn(C, 3 * H, device=dev)
    h_all, saves = ext.gru_seq_forward(xg, w_hh, b_hh, h0, gamma, beta, False, True)
    w_img, w_fwd = gru_mod._bwd_weight_images(w_hh)
    good = dict(grad=torch.randn(B, T, C, H, device=dev), w_img=w_img, w_fwd=w_fwd,
                xg=xg, gamma=gamma, beta=beta, b_hh=b_hh, h0=h0, h_all=h_all,
                saves=saves)
    fn = lambda **t: ext.gru_seq_backward_kernel(*t.values(), False)
    dpre, dh0 = fn(**good)
    assert dpre.shape == (B, T, C, 4 * H) and dh0.shape == (B, C, H)

    f16 = lambda t: torch.zeros(t.shape, dtype=torch.float16, device=dev)
    cases = [("grad", _i32(good["grad"]), "gru grad must be bf16 or f32"),
             ("b_hh", _i32(b_hh), "b_hh must be"),
             ("b_hh", _more(b_hh), "b_hh must have 384 elements"),
             ("saves", _i32(saves), "gru saves must be"),
             ("saves", _more(saves, 3), "gru saves must have 768 elements"),
             ("saves", _strided(saves), "gru saves must be contiguous")]
    # h_all is where the binding reads B, T, C from, so it has no "more
    # elements" case of its own; x_gates (1, 1, 3H) has no non-contiguous view
    cases += [("h_all", _i32(h_all), "gru h_all must be"),
              ("h_all", _strided(h_all), "gru h_all must be contiguous"),
              ("xg", _i32(xg), "x_gates must be"),
              ("xg", _more(xg, 2), "x_gates must have shape")]
    for name, label in (("grad", "gru grad"), ("gamma", "gamma"), ("beta", "beta"),
                        ("h0", "h0")):
        if name != "grad":
            cases.append((name, _i32(good[name]), f"{label} must be"))
        cases += [(name, _more(good[name], good[name].dim() - 1),
                   f"{label} must have shape"),
                  (name, _strided(good[name]), f"{label} must be contiguous")]
    for name in ("w_img", "w_fwd"):      # bf16 images: f16 is the same size
        cases += [(name, f16(good[name]), f"{name} must be"),
                  (name, _more(good[name]), f"{name} must have shape"),
                  (name, _strided(good[name]), f"{name} must be contiguous")]
    _rejects(fn, good, cases)

    # the fused-heads entry shares the checks; its own operand is wh_img
    wh_img = torch.zeros(H, 32, device=dev, dtype=torch.bfloat16)
    goodh = dict(grad=torch.randn(B, T, C, O, device=dev), wh_img=wh_img,
                 **{k: v for k, v in good.items() if k != "grad"})
    fnh = lambda **t: ext.gru_seq_backward_heads_kernel(*t.values(), False)
    dpre, _ = fnh(**goodh)
    assert dpre.shape == (B, T, C, 4 * H)
    _rejects(fnh, goodh, [
        ("wh_img", f16(wh_img), "wh_img must be"),
        ("wh_img", _more(wh_img, 1), "wh_img must have shape"),
        ("wh_img", _strided(wh_img), "wh_img must be contiguous"),
        ("h_all", _i32(h_all), "gru h_all must be"),
        ("gamma", _strided(gamma), "gamma must be contiguous"),
    ])
