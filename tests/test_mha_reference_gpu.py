"""The four attention kernels against ``ops.reference_mha_step`` in float64.

Every case compares o, lse, dq, dk, dv of the kernels with the float64
reference on the same (IO-dtype-valued) inputs.  No tolerance is picked in
advance: per case and tensor

    max|X_kernel - X_ref64| <= K * max|X_emu - X_ref64| + floor(X)

where ``X_emu`` is the bf16/float32 emulation of the kernels' arithmetic
(``reference_mha_step(emulate=)``), K = ``MHA_ERROR_FACTOR`` and the floor is
one IO-dtype ulp of the largest reference element (lse: ``MHA_LSE_FLOOR``);
``ops/attention_reference.py`` has the helper, the input families and the case
lists, and tests/test_mha_reference_cpu.py shows on the CPU that this bound
admits at most 5 % of a tensor's largest element and that nine wrong formulas
miss it.  Each comparison prints an ``MHA-RATIO`` line (kernel error, emulation
error, their ratio); profiles/r16_mha_reference.md records the worst per
kernel family and IO dtype.

T <= 64 with Dh in {16, 32, 64} runs the whole-head tile kernels, everything
else (and every call with lengths) the flash-style bodies.
"""

import math

import pytest
import torch

from deeprest_amd.ops.attention_reference import (
    BHTD_CASES, FAMILY_CASES, IO_DTYPE, MAIN_CASES, REPEAT_CASES, SCALE_CASES,
    TENSORS, VARLEN_CASES, max_err, mha_case_data, varlen_case_data, whole_tile)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from deeprest_amd.ops import native_available

    if not native_available():
        pytest.fail("HIP extension not built — GPU tests must not fall back")
    return torch.device("cuda:0")


def _ids(cases):
    return [c.id for c in cases]


def _check(case, data, got, names, what):
    """Hold ``got[name]`` to the bound of ``data`` for every name; every figure
    is printed before anything is asserted."""
    family = "tile" if what != "lengths" and whole_tile(case.T, case.D) else "flash"
    failed = []
    for name in names:
        err = max_err(got[name], data["ref"][name])
        emu, bound = data["err_emu"][name], data["bound"][name]
        ratio = err / emu if emu > 0 else float("inf") if err > 0 else 0.0
        print(f"MHA-RATIO {what} {family} {case.io} {case.id} {name}: "
              f"err_kernel {err:.3e} err_emu {emu:.3e} ratio {ratio:.3f} "
              f"bound {bound:.3e} max|ref| "
              f"{float(data['ref'][name].abs().max()):.3e}")
        if not err <= bound:
            failed.append((name, err, bound))
    assert not failed, (case.id, failed)


def _run_packed(case, data, dev):
    """``ops.mha_packed`` with autograd on the packed image of the case's
    q, k, v; lse from the binding.  Everything back in (B, H, T, D)."""
    from deeprest_amd.ops import mha_packed
    from deeprest_amd.ops.native import require_native

    q, k, v, dout = data["inputs"]
    B, H, T, D = q.shape
    dt = IO_DTYPE[case.io]
    # (B, T, 3, H, D)
    qkv = torch.stack([q, k, v], dim=0).permute(1, 3, 0, 2, 4).contiguous()
    qkv = qkv.reshape(B, T, 3 * H * D).to(dev, dt).requires_grad_(True)
    d_out = dout.permute(0, 2, 1, 3).reshape(B, T, H * D).to(dev, dt)
    o = mha_packed(qkv, H, case.scale)
    o.backward(d_out)
    assert o.shape == (B, T, H * D) and o.dtype == dt and qkv.grad.dtype == dt
    ext = require_native("mha_packed_forward")
    o2, lse = ext.mha_packed_forward(qkv.detach(), H, case.scale_value)
    assert torch.equal(o2, o.detach())
    g = qkv.grad.view(B, T, 3, H, D).permute(2, 0, 3, 1, 4)
    return dict(o=o.detach().view(B, T, H, D).permute(0, 2, 1, 3), lse=lse,
                dq=g[0], dk=g[1], dv=g[2])


def _run_bhtd(case, data, dev):
    """``ops.mha_forward`` with autograd on (B, H, T, D) tensors."""
    from deeprest_amd.ops import mha_forward
    from deeprest_amd.ops.native import require_native

    dt = IO_DTYPE[case.io]
    q, k, v, dout = (t.to(dev, dt) for t in data["inputs"])
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    o = mha_forward(q, k, v, case.scale)
    o.backward(dout)
    ext = require_native("mha_forward")
    o2, lse = ext.mha_forward(q.detach(), k.detach(), v.detach(), case.scale_value)
    assert torch.equal(o2, o.detach())
    return dict(o=o.detach(), lse=lse, dq=q.grad, dk=k.grad, dv=v.grad)


ALL = ("o", "lse") + TENSORS[1:]


@pytest.mark.parametrize("case", MAIN_CASES, ids=_ids(MAIN_CASES))
def test_packed_main_grid(dev, case):
    data = mha_case_data(case)
    _check(case, data, _run_packed(case, data, dev), ALL, "main")


@pytest.mark.parametrize("case", FAMILY_CASES, ids=_ids(FAMILY_CASES))
def test_packed_input_families(dev, case):
    data = mha_case_data(case)
    got = _run_packed(case, data, dev)
    for name in ALL:
        assert torch.isfinite(got[name].float()).all(), (case.id, name)
    _check(case, data, got, ALL, "family")


@pytest.mark.parametrize("case", SCALE_CASES, ids=_ids(SCALE_CASES))
def test_packed_scale(dev, case):
    data = mha_case_data(case)
    _check(case, data, _run_packed(case, data, dev), ALL, "scale")


@pytest.mark.parametrize("case", BHTD_CASES, ids=_ids(BHTD_CASES))
def test_bhtd_entry_is_the_packed_kernels(dev, case):
    """The same kernels on other strides: bit for bit, except a dq that goes
    through the flash backward's fp32 atomics.  That is every dq outside the
    whole-head tile kernels, T <= 64 at Dh = 24 included: the 4 waves of the
    one key-tile block each add their 16 keys' share to the same dq element,
    in no fixed order.  Such a dq is held to the bound only."""
    data = mha_case_data(case)
    got = _run_bhtd(case, data, dev)
    _check(case, data, got, ALL, "bhtd")
    packed = _run_packed(case, data, dev)
    exact = ["o", "lse", "dk", "dv"] + (["dq"] if whole_tile(case.T, case.D) else [])
    for name in exact:
        assert torch.equal(got[name], packed[name]), (case.id, name)


@pytest.mark.parametrize("case", REPEAT_CASES, ids=_ids(REPEAT_CASES))
def test_flash_backward_twice(dev, case):
    """The zeroed dq accumulator and the atomics: a second backward on the same
    input is within the bound, dk and dv are bit-equal, and the two dq are
    within the bound of each other."""
    data = mha_case_data(case)
    a = _run_packed(case, data, dev)
    b = _run_packed(case, data, dev)
    _check(case, data, a, ALL, "repeat-1")
    _check(case, data, b, ALL, "repeat-2")
    for name in ("o", "lse", "dk", "dv"):
        assert torch.equal(a[name], b[name]), (case.id, name)
    gap = max_err(a["dq"], b["dq"].double())
    print(f"MHA-REPEAT {case.id}: max|dq_1 - dq_2| {gap:.3e} "
          f"bound {data['bound']['dq']:.3e}")
    assert gap <= data["bound"]["dq"]


@pytest.mark.parametrize("case", VARLEN_CASES, ids=_ids(VARLEN_CASES))
def test_forward_with_lengths(dev, case):
    from deeprest_amd.ops import mha_forward
    from deeprest_amd.ops.native import require_native

    data = varlen_case_data(case)
    dt = IO_DTYPE[case.io]
    q, k, v = (t.to(dev, dt) for t in data["inputs"])
    lengths = data["lengths"].to(dev)
    ext = require_native("mha_forward")
    scale = 1.0 / math.sqrt(case.D)          # the default of ops.mha_forward
    with torch.no_grad():
        o = mha_forward(q, k, v, kv_lengths=lengths)
        o2, lse = ext.mha_forward(q, k, v, scale, lengths)
    assert torch.equal(o, o2)
    _check(case, data, dict(o=o, lse=lse), ("o", "lse"), "lengths")
    clamped = [min(max(L, 1), case.T) for L in case.lengths]
    for b, L in enumerate(clamped):
        assert (o[b, :, L:] == 0).all() and (lse[b, :, L:] == 0).all(), (case.id, b)
        assert (data["ref"]["o"][b, :, L:] == 0).all()
        assert (data["ref"]["lse"][b, :, L:] == 0).all()
    # NaN in every padded position leaves the result bit-equal
    qn, kn, vn = (t.clone() for t in (q, k, v))
    for b, L in enumerate(clamped):
        for t in (qn, kn, vn):
            t[b, :, L:] = float("nan")
    with torch.no_grad():
        on, lse_n = ext.mha_forward(qn, kn, vn, scale, lengths)
    assert torch.equal(on, o) and torch.equal(lse_n, lse)
