"""The fragment-major weight image, checked on the CPU: the view/permute
helper the GPU tests use as their reference must invert exactly and must
put every lane's fragment piece where the kernels' address formula reads
it."""

import pytest
import torch

import mlp_fraglayout_ref as ref

# (N, K) valid sizes; the last is the transposed-w1 case (source [400, 247])
SHAPES = [(16, 8), (48, 40), (400, 247), (256, 400)]


def _pads(N, K):
    return (N + 15) // 16 * 16, (K + 31) // 32 * 32


def _asym(n, k):
    # every element distinct and exactly representable: position = value
    return (torch.arange(n * k, dtype=torch.float32).view(n, k) + 1.0)


def _padded(N, K):
    Np, Kp = _pads(N, K)
    if (N, K) == (256, 400):
        w = _asym(400, 247)                      # w1; the image is of w1^T
        return ref.pad(w.t(), Np, Kp), w, True
    w = _asym(N, K)
    return ref.pad(w, Np, Kp), w, False


@pytest.mark.parametrize("N,K", SHAPES)
def test_round_trip(N, K):
    wp, w, trans = _padded(N, K)
    img = ref.pack(wp)
    assert img.shape == wp.shape
    assert torch.equal(ref.unpack(img), wp)
    assert torch.equal(ref.image(w, *wp.shape, trans=trans), img)
    if wp.shape[1] > 32 or wp.shape[0] > 16:
        assert not torch.equal(img, wp)          # it does permute


@pytest.mark.parametrize("N,K", SHAPES)
def test_lane_emulation(N, K):
    # the kernels' read: lane's 8 elements of k-step s of chunk c sit at
    # ((c*KS + s)*64 + lane)*8 and are Wp[16c + lane%16][32s + lane//16*8 + e]
    wp, _, _ = _padded(N, K)
    Np, Kp = wp.shape
    KS = Kp // 32
    flat = ref.pack(wp).reshape(-1)
    c, s, lane, e = torch.meshgrid(
        torch.arange(Np // 16), torch.arange(KS), torch.arange(64),
        torch.arange(8), indexing="ij")
    got = flat[((c * KS + s) * 64 + lane) * 8 + e]
    want = wp[16 * c + lane % 16, 32 * s + (lane // 16) * 8 + e]
    assert torch.equal(got, want)


@pytest.mark.parametrize("N,K", SHAPES)
def test_element_address(N, K):
    # the closed form of the layout, element by element
    wp, _, _ = _padded(N, K)
    Np, Kp = wp.shape
    KS = Kp // 32
    n, k = torch.meshgrid(torch.arange(Np), torch.arange(Kp), indexing="ij")
    addr = (((n // 16 * KS + k // 32) * 64 + (k % 32) // 8 * 16 + n % 16) * 8
            + k % 8)
    assert torch.equal(ref.pack(wp).reshape(-1)[addr], wp)
