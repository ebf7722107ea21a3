"""What the attention reference tests share: input families, the error bound
and the list of GPU cases (tests/test_mha_reference_cpu.py checks the bound on
the CPU for every case that tests/test_mha_reference_gpu.py runs).

Nothing here runs a kernel.  The bound of a case is computed from the float64
reference and the arithmetic emulation of ``ops.reference_mha_step`` alone.
"""

from __future__ import annotations

import functools
import math
from typing import List, NamedTuple, Optional, Tuple

import torch

from .attention import reference_mha_step

# ------------------------------------------------------------------ the bound
# max|X_kernel - X_ref64| <= K * max|X_emu - X_ref64| + floor(X)
#
# K: what the emulation does not model (summation order inside and across the
# MFMAs, the running maximum of the flash forward, __expf / __logf).  4 is the
# fused-Adam precedent; profiles/r16_mha_reference.md has the measured ratios.
MHA_ERROR_FACTOR = 4.0
# lse floor, as a share of max(1, max|lse_ref|): twice the worst kernel error
# measured over the bf16-IO cases, 1.69e-7 (profiles/r16_mha_reference.md; with
# bf16 IO the operands are exact, so that error is __expf / __logf and float32
# sums).  It may never exceed 1e-4: one key of average weight among T <= 161
# shifts lse by 1/161 = 6e-3, sixty times that cap.
MHA_LSE_FLOOR = 3.4e-7
MHA_LSE_FLOOR_CAP = 1e-4
# the bound may be at most this share of max|ref| (where a cap applies)
MHA_BOUND_CAP = 0.05

IO_ULP = {"bf16": 2.0 ** -8, "f32": 2.0 ** -23}
IO_DTYPE = {"bf16": torch.bfloat16, "f32": torch.float32}
TENSORS = ("o", "dq", "dk", "dv")
FAMILIES = ("uniform", "peaky", "ramp", "ramp_down", "shifted+", "shifted-")


def max_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max|got - ref| in float64 on the host; inf if anything is not finite
    (a NaN must not pass as "no error")."""
    d = (got.detach().to("cpu", torch.float64).reshape(ref.shape)
         - ref.detach().to("cpu", torch.float64)).abs().max()
    return float(d) if torch.isfinite(d) else float("inf")


def mha_zero_reference_term(q, k, v, dout, scale: float) -> float:
    """Absolute term of the bound for a dq or dk whose reference is exactly
    zero: T = 1, where P = 1 and dP = Drow in exact arithmetic, so dS = 0.

    The kernels take ``dP = dout . v`` from an MFMA and ``Drow = dout . o``
    from a float32 loop over d: two float32 sums of the same Dh products in
    different orders.  Each is off by at most ``(Dh - 1) * 2^-24`` of
    ``sum|terms| <= Dh * max|dout| * max|v|`` (the standard bound of a
    float32 sum in any order), so their difference is at most
    ``2^-23 * Dh * (Dh * max|dout| * max|v|)``.  dS multiplies that by
    ``scale``, and dq / dk multiply dS by an element of k / q (one key, one
    query)::

        2^-23 * Dh * (Dh * max|dout| * max|v| * scale) * max(max|q|, max|k|)

    (the rounding of dS to bf16 is relative and changes this by 2^-9 of
    itself).  For f32 IO the operand rounding of dout and v makes dP - Drow
    larger than this, but the emulation commits that rounding too, and the
    ``K * err_emu`` term of the bound carries it.
    """
    Dh = q.shape[-1]
    amax = lambda t: float(t.detach().abs().max())               # noqa: E731
    return (2.0 ** -23 * Dh * (Dh * amax(dout) * amax(v) * scale)
            * max(amax(q), amax(k)))


def mha_error_bound(name: str, ref: torch.Tensor, emu: torch.Tensor, io: str,
                    zero_term: float = 0.0) -> Tuple[float, float]:
    """``(bound, err_emu)`` for output ``name`` in {o, dq, dk, dv, lse} of one
    case: ``ref`` is the float64 reference, ``emu`` the emulation for IO dtype
    ``io`` ("bf16" or "f32").

    o, dq, dk, dv: ``K * max|emu - ref| + floor`` with the floor one IO-dtype
    ulp of the largest reference element (2^-8 or 2^-23 times ``max|ref|``);
    where the reference is exactly zero, ``zero_term``
    (:func:`mha_zero_reference_term`) is added.

    lse (float32 in both IO types): ``K * max|emu - ref| + MHA_LSE_FLOOR *
    max(1, max|ref|)``.
    """
    err_emu = max_err(emu, ref)
    big = float(ref.detach().abs().max())
    if name == "lse":
        return MHA_ERROR_FACTOR * err_emu + MHA_LSE_FLOOR * max(1.0, big), err_emu
    bound = MHA_ERROR_FACTOR * err_emu + IO_ULP[io] * big
    if big == 0.0:
        bound += zero_term
    return bound, err_emu


def bound_is_capped(family: str, name: str) -> bool:
    """Whether the bound of output ``name`` must stay under ``MHA_BOUND_CAP *
    max|ref|``.  dq of the ramp and shifted families is held to the bound but
    has no cap: the structured k column (up to 34 and 64 at Dh = 32) multiplies
    the bf16 rounding of dS, while the exact dq is small."""
    if name == "lse":
        return False
    return not (name == "dq" and family not in ("uniform", "peaky"))


# ------------------------------------------------------------------- inputs
def _bf16(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


def mha_inputs(family: str, B: int, H: int, T: int, D: int, io: str,
               scale: Optional[float] = None, seed: int = 0):
    """Seeded float32 host tensors ``q, k, v, dout`` of shape (B, H, T, D).

    - ``uniform``: 0.7 * randn, the suite's usual input;
    - ``peaky``: uniform with q * 4 (logit std near 2.8: few keys carry a row);
    - ``ramp`` / ``ramp_down``: uniform plus ``q[..., 0] = 2`` and ``k[..., 0]``
      rising (falling) linearly in the key index so that S gains 0..12 across
      the keys: the running maximum of the flash forward grows at every 32-key
      step (or is held by the first);
    - ``shifted+`` / ``shifted-``: uniform plus ``q[..., 0] = 8`` and
      ``k[..., 0] = +c / -c`` with ``8 * c * scale`` near 90: ``exp(90)``
      overflows float32 and ``exp(-90)`` is below its normal range.

    Every structured column is rounded to bf16 in both IO types (otherwise f32
    IO pays the kernels' operand rounding on the large component); for bf16 IO
    the whole input is rounded to bf16, so reference, emulation and kernel see
    the same values.
    """
    if family not in FAMILIES:
        raise ValueError(f"unknown family {family!r}")
    if scale is None:
        scale = 1.0 / math.sqrt(D)
    gen = torch.Generator(device="cpu").manual_seed(
        1_000_003 * seed + 10_007 * T + 101 * D + 11 * B + H)
    q, k, v, dout = (0.7 * torch.randn(B, H, T, D, generator=gen) for _ in range(4))
    if family == "peaky":
        q = q * 4.0
    elif family in ("ramp", "ramp_down"):
        q[..., 0] = 2.0
        ramp = torch.arange(T, dtype=torch.float32) / max(T - 1, 1)
        if family == "ramp_down":
            ramp = ramp.flip(0)
        k[..., 0] = _bf16(ramp * (12.0 / (2.0 * scale)))
    elif family in ("shifted+", "shifted-"):
        q[..., 0] = 8.0
        c = _bf16(torch.tensor(90.0 / (8.0 * scale)))
        k[..., 0] = c if family == "shifted+" else -c
    if io == "bf16":
        q, k, v, dout = (_bf16(t) for t in (q, k, v, dout))
    return q, k, v, dout


# -------------------------------------------------------------------- cases
class MhaCase(NamedTuple):
    family: str
    B: int
    H: int
    T: int
    D: int
    io: str
    scale: Optional[float] = None      # None: 1 / sqrt(D)

    @property
    def id(self) -> str:
        s = "" if self.scale is None else f"-s{self.scale}"
        return f"{self.family}-{self.B}x{self.H}-T{self.T}-D{self.D}-{self.io}{s}"

    @property
    def scale_value(self) -> float:
        return 1.0 / math.sqrt(self.D) if self.scale is None else float(self.scale)


def whole_tile(T: int, D: int) -> bool:
    """The launcher's choice (``mha_whole_tile`` in csrc/attention.hip)."""
    return 1 <= T <= 64 and D in (16, 32, 64)


IOS = ("bf16", "f32")
MAIN_T = (1, 2, 15, 16, 17, 31, 33, 48, 63, 64, 65, 96, 97, 127, 128, 129, 161)
MAIN_D = (8, 16, 24, 32, 40, 48, 56, 64)
MAIN_BH = ((1, 1), (1, 3), (3, 2), (2, 4))      # B*H mod 4 = 1, 3, 2, 0


def _main_cases() -> List[MhaCase]:
    out = []
    for it, T in enumerate(MAIN_T):
        for id_, D in enumerate(MAIN_D):
            # the case index, skewed by the row so that one head size meets
            # every (B, H) as T varies
            B, H = MAIN_BH[(it * len(MAIN_D) + id_ + it) % len(MAIN_BH)]
            out += [MhaCase("uniform", B, H, T, D, io) for io in IOS]
    return out


MAIN_CASES = _main_cases()
FAMILY_CASES = [MhaCase(f, 2, 3, T, D, io) for f in FAMILIES
                for T in (17, 60, 64, 65, 129) for D in (24, 32) for io in IOS]
SCALE_CASES = [MhaCase("uniform", 2, 3, T, 32, io, s) for s in (0.3, 1.0)
               for T in (60, 129) for io in IOS]
BHTD_CASES = [MhaCase("uniform", 2, 3, T, D, io) for T in (17, 60, 64, 65, 129)
              for D in (24, 32, 64) for io in IOS]
REPEAT_CASES = [MhaCase("uniform", 2, 3, 129, D, io) for D in (24, 32) for io in IOS]
GRAD_CASES = MAIN_CASES + FAMILY_CASES + SCALE_CASES + BHTD_CASES + REPEAT_CASES


class VarlenCase(NamedTuple):
    family: str
    T: int
    D: int
    io: str
    lengths: Tuple[int, ...]           # B = 4 samples, H = 2

    @property
    def id(self) -> str:
        ls = "_".join(str(x) for x in self.lengths)
        return f"{self.family}-T{self.T}-D{self.D}-{self.io}-L{ls}"


def varlen_length_pool(T: int) -> Tuple[int, ...]:
    return (0, 1, 31, 32, 33, 63, 64, 65, 96, T - 1, T, T + 5)


def _varlen_cases() -> List[VarlenCase]:
    out = []
    for T in (60, 64, 129):
        pool = varlen_length_pool(T)
        i = 0
        for D in (24, 32, 64):
            for io in IOS:
                for family in ("uniform", "peaky"):
                    # 4 consecutive entries of the pool: every 3 cases use all 12
                    lens = tuple(pool[(4 * i + j) % len(pool)] for j in range(4))
                    out.append(VarlenCase(family, T, D, io, lens))
                    i += 1
    return out


VARLEN_CASES = _varlen_cases()
VARLEN_H = 2


# ------------------------------------------------- references, computed once
# (the tests that share a case run next to each other: a bounded cache)
@functools.lru_cache(maxsize=64)
def mha_case_data(case: MhaCase) -> dict:
    """Inputs, float64 reference, emulation and bounds of one gradient case,
    computed once and never modified::

        {"inputs": (q, k, v, dout) f32, "ref": {name: f64}, "emu": {name: f32},
         "bound": {name: float}, "err_emu": {name: float}}

    with names o, lse, dq, dk, dv."""
    scale = case.scale_value
    inputs = mha_inputs(case.family, case.B, case.H, case.T, case.D, case.io, scale)
    names = ("o", "lse", "dq", "dk", "dv")
    ref = dict(zip(names, reference_mha_step(*(t.double() for t in inputs), scale)))
    if case.T == 1:
        # one key: dS = 0 exactly.  The float64 steps leave 1e-16 of their own
        # cancellation for f32 inputs; the reference is the exact answer.
        ref["dq"], ref["dk"] = torch.zeros_like(ref["dq"]), torch.zeros_like(ref["dk"])
    emu = dict(zip(names, reference_mha_step(*inputs, scale, emulate=case.io)))
    zero_term = mha_zero_reference_term(*inputs, scale)
    bound, err_emu = {}, {}
    for n in names:
        bound[n], err_emu[n] = mha_error_bound(n, ref[n], emu[n], case.io, zero_term)
    return dict(inputs=inputs, ref=ref, emu=emu, bound=bound, err_emu=err_emu)


@functools.lru_cache(maxsize=64)
def varlen_case_data(case: VarlenCase) -> dict:
    """The same for a forward case with lengths (names o, lse); ``lengths`` is
    the (4,) int32 host tensor."""
    q, k, v, _ = mha_inputs(case.family, len(case.lengths), VARLEN_H, case.T,
                            case.D, case.io)
    lengths = torch.tensor(case.lengths, dtype=torch.int32)
    ref = dict(zip(("o", "lse"), reference_mha_step(
        q.double(), k.double(), v.double(), None, kv_lengths=lengths)))
    emu = dict(zip(("o", "lse"), reference_mha_step(
        q, k, v, None, kv_lengths=lengths, emulate=case.io)))
    bound, err_emu = {}, {}
    for n in ("o", "lse"):
        bound[n], err_emu[n] = mha_error_bound(n, ref[n], emu[n], case.io)
    return dict(inputs=(q, k, v), lengths=lengths, ref=ref, emu=emu, bound=bound,
                err_emu=err_emu)
