"""CPU tests of the GRU backward reductions' host side: the pure-torch
reference of ext.gru_bwd_reduce (ops.gru.reference_bwd_reduce) and the
assembly of dW_hh, db_hh and dbeta from dpre's slice order dr|dz|d_hhn|dn in
ops.gru._bwd_reductions.

The pi packing and the slice order are rebuilt here with a plain loop, so the
tests do not share an index table with the code under test."""

import pytest
import torch

from deeprest_amd.ops import gru as gru_mod

H = 128
SLICES = ["r", "z", "hhn", "n"]          # dpre's slice order
GATES = ["r", "z", "n"]                  # x-side gate order (PyTorch GRU)


def _natural(B, T, C, seed):
    gen = torch.Generator().manual_seed(seed)
    nat = {s: torch.randn(B, T, C, H, generator=gen, dtype=torch.float64)
           for s in SLICES}
    gamma = torch.randn(C, 3 * H, generator=gen, dtype=torch.float64)
    xg = torch.randn(B, T, 3 * H, generator=gen, dtype=torch.float64)
    return nat, gamma, xg


def _pack(nat):
    """dpre (B, T, C, 4H): slice s at [s*H, (s+1)*H); inside a slice position
    cc*8 + e holds natural column cc + 16*e."""
    B, T, C, _ = nat["r"].shape
    dpre = torch.empty(B, T, C, 4 * H, dtype=torch.float64)
    for s, name in enumerate(SLICES):
        for cc in range(16):
            for e in range(8):
                dpre[..., s * H + cc * 8 + e] = nat[name][..., cc + 16 * e]
    return dpre


@pytest.mark.parametrize("shape", [(1, 1, 3), (2, 3, 5), (3, 2, 9)])
def test_reference_matches_einsum(shape):
    B, T, C = shape
    nat, gamma, xg = _natural(B, T, C, seed=B * 100 + T * 10 + C)
    dxg, dgamma, dbeta4 = gru_mod.reference_bwd_reduce(_pack(nat), gamma, xg)
    assert dxg.shape == (B, T, 3 * H)
    assert dgamma.shape == (C, 3 * H) and dbeta4.shape == (C, 4 * H)
    for g, name in enumerate(GATES):
        cols = slice(g * H, (g + 1) * H)
        torch.testing.assert_close(
            dxg[..., cols], torch.einsum("btcj,cj->btj", nat[name], gamma[:, cols]),
            rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(
            dgamma[:, cols], torch.einsum("btcj,btj->cj", nat[name], xg[..., cols]),
            rtol=1e-12, atol=1e-12)
    for s, name in enumerate(SLICES):
        torch.testing.assert_close(dbeta4[:, s * H:(s + 1) * H],
                                   nat[name].sum(dim=(0, 1)), rtol=1e-12, atol=1e-12)


class _ReferenceExt:
    """Stands in for the extension: the reductions come from the reference."""

    def __init__(self):
        self.modes = []

    def gru_bwd_reduce(self, dpre, gamma, xg, mode="auto"):
        self.modes.append(mode)
        return gru_mod.reference_bwd_reduce(dpre, gamma, xg)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("shape", [(2, 3, 4), (3, 1, 3)])      # T = 1: boundary only
def test_bwd_reductions_pick_the_right_slices(shape, reverse):
    B, T, C = shape
    nat, gamma, xg = _natural(B, T, C, seed=7 + T)
    gen = torch.Generator().manual_seed(11)
    h_all = torch.randn(B, T, C, H, generator=gen, dtype=torch.float64)
    h0 = torch.randn(B, C, H, generator=gen, dtype=torch.float64)
    dh0 = torch.randn(B, C, H, generator=gen, dtype=torch.float64)
    w_hh = torch.zeros(3 * H, H, dtype=torch.float64)
    ext = _ReferenceExt()
    dxg, dw_hh, db_hh, dh0_out, dgamma, dbeta = gru_mod._bwd_reductions(
        ext, _pack(nat), dh0, xg, w_hh, h0, gamma, h_all, reverse)
    assert ext.modes == [gru_mod.REDUCE_MODE] == ["auto"]

    # h_prev of step t: the neighbouring step's state, h0 at the boundary
    if reverse:
        h_prev = torch.cat([h_all[:, 1:], h0[:, None]], dim=1)
    else:
        h_prev = torch.cat([h0[:, None], h_all[:, :-1]], dim=1)
    for g, name in enumerate(["r", "z", "hhn"]):        # W_hr, W_hz, W_hn rows
        rows = slice(g * H, (g + 1) * H)
        # the op sums the per-sample GEMMs into fp32 whatever the input dtype
        torch.testing.assert_close(
            dw_hh[rows], torch.einsum("btcj,btck->jk", nat[name], h_prev),
            rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(db_hh[rows], nat[name].sum(dim=(0, 1, 2)),
                                   rtol=1e-10, atol=1e-10)
    for g, name in enumerate(GATES):
        cols = slice(g * H, (g + 1) * H)
        torch.testing.assert_close(dbeta[:, cols], nat[name].sum(dim=(0, 1)),
                                   rtol=1e-10, atol=1e-10)
        torch.testing.assert_close(
            dgamma[:, cols], torch.einsum("btcj,btj->cj", nat[name], xg[..., cols]),
            rtol=1e-10, atol=1e-10)
        torch.testing.assert_close(
            dxg[..., cols], torch.einsum("btcj,cj->btj", nat[name], gamma[:, cols]),
            rtol=1e-10, atol=1e-10)
    assert dw_hh.shape == (3 * H, H) and db_hh.shape == (3 * H,)
    assert dbeta.shape == (C, 3 * H)
    torch.testing.assert_close(dh0_out, dh0)
