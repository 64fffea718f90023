"""Pure-torch reference of the fused MLP's fragment-major weight image
(openembedding_amd/ops/csrc/mlp.hip). Tested without a GPU in
test_mlp_fraglayout_ref.py; the GPU tests compare the pack kernel to it.

A padded weight Wp [N, Kp] (N % 16 == 0, Kp % 32 == 0, KS = Kp/32, B =
W[n][k]) keeps element (n, k) at
    ((n/16 * KS + k/32) * 64 + ((k%32)/8) * 16 + n%16) * 8 + k%8
so that lane l of a wave finds its 8 elements of k-step s of column chunk c
at ((c*KS + s) * 64 + l) * 8."""

from __future__ import annotations

import torch


def pad(w: torch.Tensor, N: int, Kp: int) -> torch.Tensor:
    """Row-major zero-padded copy [N, Kp] of w [n, k]."""
    assert w.dim() == 2 and w.shape[0] <= N and w.shape[1] <= Kp
    wp = torch.zeros(N, Kp, dtype=w.dtype, device=w.device)
    wp[:w.shape[0], :w.shape[1]] = w
    return wp


def pack(wp: torch.Tensor) -> torch.Tensor:
    """Fragment-major image of a padded Wp [N, Kp]; same shape declared."""
    N, Kp = wp.shape
    assert N % 16 == 0 and Kp % 32 == 0
    KS = Kp // 32
    img = wp.view(N // 16, 16, KS, 4, 8).permute(0, 2, 3, 1, 4)
    return img.contiguous().view(N, Kp)


def unpack(img: torch.Tensor) -> torch.Tensor:
    """Inverse of pack."""
    N, Kp = img.shape
    KS = Kp // 32
    wp = img.contiguous().view(N // 16, KS, 4, 16, 8).permute(0, 3, 1, 2, 4)
    return wp.contiguous().view(N, Kp)


def image(w: torch.Tensor, N: int, Kp: int, trans: bool = False
          ) -> torch.Tensor:
    """What mlp3_pack_frag writes into a [N, Kp] destination from source w
    (of w's transpose when trans)."""
    return pack(pad(w.t() if trans else w, N, Kp))
