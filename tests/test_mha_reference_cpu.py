"""``ops.reference_mha_step`` and the bound of the attention reference tests,
on the CPU.

1. The float64 reference is the formula: against autograd through plain
   ``softmax(q k^T * scale) v`` and ``torch.logsumexp`` to 1e-10 relative, and
   with ``kv_lengths`` against ``reference_mha`` at float32.
2. The emulation is finite for every input family, bf16-valued for bf16 IO, and
   its error against float64 is non-zero where it should be.
3. The bound is computed from reference and emulation alone, so what it admits
   is checked here for every case tests/test_mha_reference_gpu.py runs: at most
   5 % of the largest reference element (``bound_is_capped``).
4. Nine wrong formulas ("mutants"), each in float64 so that nothing but the
   defect separates it from the reference, miss that bound by at least 2x in
   some output of some GPU case.  profiles/r16_mha_reference.md has the table.
"""

import math

import pytest
import torch

from deeprest_amd.ops import reference_mha, reference_mha_step
from deeprest_amd.ops.attention_reference import (
    FAMILIES, FAMILY_CASES, GRAD_CASES, MAIN_CASES, MHA_BOUND_CAP,
    MHA_ERROR_FACTOR, MHA_LSE_FLOOR, MHA_LSE_FLOOR_CAP, TENSORS, VARLEN_CASES,
    bound_is_capped, max_err, mha_case_data, mha_inputs, varlen_case_data,
    varlen_length_pool, whole_tile)

ALL_GRAD_CASES = list(dict.fromkeys(GRAD_CASES))


# ------------------------------------------------------- 1. the reference
@pytest.mark.parametrize("scale", [None, 0.3])
@pytest.mark.parametrize("shape", [(2, 3, 17, 24), (1, 2, 65, 32), (1, 1, 1, 8)])
def test_reference_is_autograd_of_plain_softmax(shape, scale):
    q, k, v, dout = (t.double() for t in mha_inputs("peaky", *shape, "f32"))
    o, lse, dq, dk, dv = reference_mha_step(q, k, v, dout, scale)
    assert all(t.dtype == torch.float64 for t in (o, lse, dq, dk, dv))
    qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
    sc = 1.0 / math.sqrt(shape[-1]) if scale is None else scale
    s = qa @ ka.transpose(-1, -2) * sc
    oa = torch.softmax(s, dim=-1) @ va
    oa.backward(dout)
    for name, got, want in (("o", o, oa.detach()), ("dq", dq, qa.grad),
                            ("dk", dk, ka.grad), ("dv", dv, va.grad),
                            ("lse", lse, torch.logsumexp(s.detach(), dim=-1))):
        tol = 1e-10 * max(float(want.abs().max()), 1e-3)
        assert max_err(got, want) <= tol, (name, max_err(got, want), tol)


def test_reference_with_lengths_matches_reference_mha():
    B, H, T, D = 4, 2, 70, 24
    q, k, v, _ = mha_inputs("peaky", B, H, T, D, "f32")
    lengths = torch.tensor([0, 33, 70, 75], dtype=torch.int32)
    want = reference_mha(q, k, v, kv_lengths=lengths)
    o, lse, dq, dk, dv = reference_mha_step(q, k, v, None, kv_lengths=lengths)
    assert dq is None and dk is None and dv is None
    assert o.dtype == torch.float32
    # two float32 computations of one formula
    assert max_err(o, want) <= 1e-5 * float(want.abs().max())
    for b, L in enumerate([1, 33, 70, 70]):
        assert (o[b, :, L:] == 0).all() and (lse[b, :, L:] == 0).all()
        want_lse = torch.logsumexp(
            q[b, :, :L].double() @ k[b, :, :L].double().transpose(-1, -2)
            / math.sqrt(D), dim=-1)
        assert max_err(lse[b, :, :L], want_lse) <= 1e-5
    # NaN in every padded position never reaches a valid row
    qn, kn, vn = (t.clone() for t in (q, k, v))
    for b, L in enumerate([1, 33, 70, 70]):
        for t in (qn, kn, vn):
            t[b, :, L:] = float("nan")
    for emulate in (None, "bf16", "f32"):
        a = reference_mha_step(q, k, v, None, kv_lengths=lengths, emulate=emulate)
        n = reference_mha_step(qn, kn, vn, None, kv_lengths=lengths, emulate=emulate)
        assert torch.equal(a[0], n[0]) and torch.equal(a[1], n[1]), emulate
    with pytest.raises(ValueError, match="forward only"):
        reference_mha_step(q, k, v, q, kv_lengths=lengths)
    with pytest.raises(ValueError, match="emulate"):
        reference_mha_step(q, k, v, q, emulate="fp8")


# ------------------------------------------------------- 2. the emulation
@pytest.mark.parametrize("io", ["bf16", "f32"])
@pytest.mark.parametrize("family", FAMILIES)
def test_emulation_is_finite_and_in_the_io_dtype(family, io):
    inputs = mha_inputs(family, 2, 3, 129, 32, io)
    ref = reference_mha_step(*(t.double() for t in inputs))
    emu = reference_mha_step(*inputs, emulate=io)
    for name, e, r in zip(("o", "lse", "dq", "dk", "dv"), emu, ref):
        assert e.dtype == torch.float32 and torch.isfinite(e).all(), name
        assert torch.isfinite(r).all(), name
        if io == "bf16" and name != "lse":
            assert torch.equal(e, e.to(torch.bfloat16).float()), name
        if name != "lse":
            # the emulation rounds: it is not the reference
            assert max_err(e, r) >= 2.0 ** -12 * float(r.abs().max()), name


def test_emulation_rounds_f32_operands_only():
    """f32 IO: the outputs are not bf16 values, and an input that is already
    bf16-valued gives the same o as bf16 IO before the output rounding."""
    inputs = mha_inputs("uniform", 1, 2, 33, 16, "bf16")
    o32 = reference_mha_step(*inputs, emulate="f32")[0]
    o16 = reference_mha_step(*inputs, emulate="bf16")[0]
    assert not torch.equal(o32, o32.to(torch.bfloat16).float())
    assert torch.equal(o32.to(torch.bfloat16).float(), o16)


# ---------------------------------------------------- 3. what the bound admits
def test_case_lists_cover_what_they_claim():
    assert MHA_ERROR_FACTOR <= 8 and MHA_LSE_FLOOR <= MHA_LSE_FLOOR_CAP
    assert all(c.B * c.H <= 8 for c in ALL_GRAD_CASES)
    # every remainder of B*H mod 4 meets the tile and the flash bodies, at
    # every head size
    for D in sorted({c.D for c in MAIN_CASES}):
        for tile in {whole_tile(c.T, D) for c in MAIN_CASES}:
            rem = {c.B * c.H % 4 for c in MAIN_CASES
                   if c.D == D and whole_tile(c.T, c.D) == tile}
            assert rem == {0, 1, 2, 3}, (D, tile, rem)
    for T in (60, 64, 129):
        used = {L for c in VARLEN_CASES if c.T == T for L in c.lengths}
        assert used == set(varlen_length_pool(T)), T


def test_bound_is_capped_for_every_gpu_case():
    worst = {}
    for case in ALL_GRAD_CASES:
        d = mha_case_data(case)
        for name in TENSORS:
            big = float(d["ref"][name].abs().max())
            assert math.isfinite(d["bound"][name]), (case.id, name)
            if big == 0.0:
                assert case.T == 1 and name in ("dq", "dk"), (case.id, name)
                continue
            share = d["bound"][name] / big
            key = (case.family, name, case.io)
            worst[key] = max(worst.get(key, 0.0), share)
            if bound_is_capped(case.family, name):
                assert share <= MHA_BOUND_CAP, (case.id, name, share)
    for case in VARLEN_CASES:
        d = varlen_case_data(case)
        share = d["bound"]["o"] / float(d["ref"]["o"].abs().max())
        key = (case.family + "+lengths", "o", case.io)
        worst[key] = max(worst.get(key, 0.0), share)
        assert share <= MHA_BOUND_CAP, (case.id, share)
    for key in sorted(worst):
        print("MHA-CAP %-18s %-3s %-4s bound / max|ref| = %.4f" % (*key, worst[key]))


# ------------------------------------------------------------- 4. mutants
def _online_forward(s, v, step=32, rescale=True, m0=-1e30, flush=False):
    """Online softmax over ``step``-key tiles as the flash forward runs it, in
    the dtype of ``s``: (o, lse).  ``rescale=False`` leaves the ``alpha``
    rescale of ``o_acc`` out; ``m0`` is the initial running maximum; ``flush``
    sets exponentials below the float32 normal range to zero, as a hardware
    exponential without denormal results does."""
    m = torch.full(s.shape[:-1], m0, dtype=s.dtype)
    l = torch.zeros_like(m)
    acc = torch.zeros(*s.shape[:-1], v.shape[-1], dtype=s.dtype)
    for k0 in range(0, s.shape[-1], step):
        sk = s[..., k0:k0 + step]
        m_new = torch.maximum(m, sk.max(dim=-1).values)
        alpha = torch.exp(m - m_new)
        p = torch.exp(sk - m_new[..., None])
        if flush:
            p = torch.where(p < torch.finfo(torch.float32).tiny, torch.zeros_like(p), p)
        l = l * alpha + p.sum(dim=-1)
        if rescale:
            acc = acc * alpha[..., None]
        acc = acc + p @ v[..., k0:k0 + step, :]
        m = m_new
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    return acc * inv[..., None], m + torch.log(l.clamp_min(1e-30))


def _mutant(name, q, k, v, dout, scale):
    """(o, lse, dq, dk, dv) of one wrong formula, in float64 (mutant 9: its
    forward in float32).  The backward is the kernels': P from the saved lse,
    Drow from the saved o."""
    q, k, v, dout = (t.double() for t in (q, k, v, dout))
    T = q.shape[2]
    if name == "scale_x1.1":
        return reference_mha_step(q, k, v, dout, scale * 1.1)
    if name == "last_key_duplicated":
        k, v = k.clone(), v.clone()
        k[..., T - 2, :], v[..., T - 2, :] = k[..., T - 1, :], v[..., T - 1, :]
        return reference_mha_step(q, k, v, dout, scale)
    s = q @ k.transpose(-1, -2) * scale
    if name == "last_key_dropped":
        s[..., T - 1] = float("-inf")
    lse = torch.logsumexp(s, dim=-1)
    if name == "denominator_misses_a_key":
        m = s.max(dim=-1).values
        lse = m + torch.log(torch.exp(s[..., :T - 1] - m[..., None]).sum(dim=-1))
    o = torch.exp(s - lse[..., None]) @ v
    if name == "no_alpha_rescale":
        o, lse = _online_forward(s, v, rescale=False)
    if name == "running_max_starts_at_0":
        o, lse = _online_forward(s.float(), v.float(), m0=0.0, flush=True)
        o, lse = o.double(), lse.double()
    p = torch.exp(s - lse[..., None])
    drow = (dout * o).sum(dim=-1, keepdim=True)
    if name == "drow_misses_last_d":
        drow = (dout[..., :-1] * o[..., :-1]).sum(dim=-1, keepdim=True)
    ds = p * (dout @ v.transpose(-1, -2) - drow) * scale
    dq = ds @ k
    if name == "dq_accumulated_twice":
        dq = 2 * dq
    ds_k, p_v = ds, p
    if name == "last_query_missing_from_dk_dv":
        ds_k, p_v = ds.clone(), p.clone()
        ds_k[..., T - 1, :] = 0
        p_v[..., T - 1, :] = 0
    return o, lse, dq, ds_k.transpose(-1, -2) @ q, p_v.transpose(-1, -2) @ dout


MUTANTS = ["scale_x1.1", "last_key_dropped", "last_key_duplicated",
           "denominator_misses_a_key", "no_alpha_rescale", "drow_misses_last_d",
           "last_query_missing_from_dk_dv", "dq_accumulated_twice",
           "running_max_starts_at_0"]


def _mutant_cases(name):
    if name == "running_max_starts_at_0":
        return [c for c in FAMILY_CASES if c.family == "shifted-" and c.io == "f32"]
    return FAMILY_CASES


def test_mutant_engine_without_a_mutation_is_the_reference():
    case = FAMILY_CASES[0]._replace(family="peaky", T=65)
    d = mha_case_data(case)
    got = _mutant("none", *d["inputs"], case.scale_value)
    for name, g in zip(("o", "lse", "dq", "dk", "dv"), got):
        assert max_err(g, d["ref"][name]) <= 1e-12, name
    # and the online forward with its rescale is the plain softmax
    q, k, v, _ = (t.double() for t in d["inputs"])
    o, lse = _online_forward(q @ k.transpose(-1, -2) * case.scale_value, v)
    assert max_err(o, d["ref"]["o"]) <= 1e-12 and max_err(lse, d["ref"]["lse"]) <= 1e-12


@pytest.mark.parametrize("name", MUTANTS)
def test_mutant_misses_the_bound(name):
    outs = ("o", "lse", "dq", "dk", "dv")
    best = (0.0, None, None)
    by_family = {}
    for case in _mutant_cases(name):
        d = mha_case_data(case)
        got = _mutant(name, *d["inputs"], case.scale_value)
        row = by_family.setdefault(case.family, dict.fromkeys(outs, 0.0))
        for out, g in zip(outs, got):
            ratio = max_err(g, d["ref"][out]) / d["bound"][out]
            row[out] = max(row[out], ratio)
            if ratio > best[0]:
                best = (ratio, case.id, out)
    for family, row in by_family.items():
        print(f"MHA-MUTANT {name:30s} {family:10s} worst err / bound: "
              + "  ".join(f"{out} {row[out]:9.3g}" for out in outs))
    print(f"MHA-MUTANT {name:30s} caught by {best[2]} of {best[1]}: {best[0]:.3g}x")
    assert best[0] >= 2.0, (name, best)
