"""Torch reference of the fused dense-parameter tail
(openembedding_amd/ops/csrc/mlp.hip: k_dense_tail). Tested without a GPU in
test_dense_tail_checkers.py; test_gpu_dense_tail.py builds its states here.

A state is a dict of CPU tensors:
    grad     bf16 [n]   the flat bf16 grads (views of the eight parameters)
    master   f32  [n]   fp32 master;  s1, s2: optimizer state or None
    flat     bf16 [n]   the working weights
    wscratch f32  [H*K0p + 2*H*H]   wgrad sums, w1's rows K0p wide
    bscratch f32  [4H + 1]          b1, b2, b3, w4, b4 sums
    w1p w2p w3p w1tp w2tp w3tp      the six fragment-major images
    p32, g32, s1_32, s2_32          the fp32 group (p32 may be empty)
    sc       f32 [3] step scalars (Adam)
The flat order is torch's parameter order: w1, b1, w2, b2, w3, b3, w4, b4.

`tail` does, per element and in this order of roundings:
    g = bf16(float(grad) + scratch);  scratch = 0      (the two finishers)
    m = flat_opt_step(master, float(g));  master = m   (fp32, one op at a time)
    flat = bf16(m);  grad = 0
    images = pack(pad(flat views))                     (mlp_fraglayout_ref)
"""

from __future__ import annotations

import torch

from mlp_fraglayout_ref import image

f32, bf16 = torch.float32, torch.bfloat16
SGD, ADAGRAD, ADAM = 0, 1, 2


def layout(H: int, K0: int):
    """name -> (offset, shape) in the flat bf16 group, and its size."""
    shapes = [("w1", (H, K0)), ("b1", (H,)), ("w2", (H, H)), ("b2", (H,)),
              ("w3", (H, H)), ("b3", (H,)), ("w4", (1, H)), ("b4", (1,))]
    out, off = {}, 0
    for name, shp in shapes:
        n = 1
        for d in shp:
            n *= d
        out[name] = (off, shp)
        off += n
    return out, off


def view(flat: torch.Tensor, lay, name: str) -> torch.Tensor:
    off, shp = lay[name]
    n = 1
    for d in shp:
        n *= d
    return flat[off:off + n].view(*shp)


def image_shapes(H: int, K0p: int):
    Hp = (H + 31) // 32 * 32
    return {"w1p": (H, K0p), "w2p": (H, Hp), "w3p": (H, Hp),
            "w1tp": (K0p, Hp), "w2tp": (H, Hp), "w3tp": (H, Hp)}


def images_of(flat: torch.Tensor, H: int, K0: int, K0p: int):
    """What a full mlp3_pack_frag writes for these weights, pads included."""
    lay, _ = layout(H, K0)
    shp = image_shapes(H, K0p)
    out = {}
    for l in ("w1", "w2", "w3"):
        w = view(flat, lay, l)
        out[l + "p"] = image(w, *shp[l + "p"])
        out[l + "tp"] = image(w, *shp[l + "tp"], trans=True)
    return out


def opt_step(opt: int, w, g, s1, s2, sc, lr, c0, c1, c2):
    """flat_opt_step (flat_opt.h) on fp32 tensors, one rounding per
    operation; updates s1 / s2 in place, returns the new weights."""
    lr, c0, c1, c2 = (torch.tensor(v, dtype=f32) for v in (lr, c0, c1, c2))
    if opt == ADAGRAD:
        a = s1 + g * g
        s1.copy_(a)
        return w - lr * g / (a.sqrt() + c0)
    if opt == SGD:
        if float(c0) == 0.0:
            return w - lr * g
        b = c0 * s1 + g
        s1.copy_(b)
        d = g + c0 * b if float(c1) != 0.0 else b
        return w - lr * d
    one = torch.tensor(1.0, dtype=f32)
    m = c0 * s1 + (one - c0) * g
    v = c1 * s2 + (one - c1) * g * g
    s1.copy_(m)
    s2.copy_(v)
    return w - lr * (m / sc[1]) / ((v / sc[2]).sqrt() + c2)


def step_scalars(sc, b1, b2):
    """k_flat_step_scalars: advance t and the two bias corrections."""
    t = sc[0] + 1.0
    sc[0] = t
    sc[1] = 1.0 - torch.tensor(b1, dtype=f32) ** t
    sc[2] = 1.0 - torch.tensor(b2, dtype=f32) ** t


def scratch_sums(st, H: int, K0: int, K0p: int) -> torch.Tensor:
    """The scratches' sums in the flat order of the parameters (fp32);
    zeroes both scratches, w1's pad columns included."""
    lay, n = layout(H, K0)
    sums = torch.zeros(n, dtype=f32)
    ws = st["wscratch"]
    view(sums, lay, "w1").copy_(ws[:H * K0p].view(H, K0p)[:, :K0])
    view(sums, lay, "w2").copy_(ws[H * K0p:H * K0p + H * H].view(H, H))
    view(sums, lay, "w3").copy_(ws[H * K0p + H * H:].view(H, H))
    for i, name in enumerate(("b1", "b2", "b3", "w4")):
        view(sums, lay, name).view(-1).copy_(
            st["bscratch"][i * H:(i + 1) * H])
    view(sums, lay, "b4").copy_(st["bscratch"][4 * H:])
    st["wscratch"].zero_()
    st["bscratch"].zero_()
    return sums


def fold(st, H: int, K0: int, K0p: int) -> torch.Tensor:
    """The finishers: bf16(float(grad) + scratch) for every parameter, as a
    flat bf16 tensor."""
    return (st["grad"].to(f32) + scratch_sums(st, H, K0, K0p)).to(bf16)


def tail(st, opt: int, H: int, K0: int, K0p: int, lr, c0, c1, c2):
    """The whole tail, in place on the state dict."""
    g = fold(st, H, K0, K0p)
    m = opt_step(opt, st["master"], g.to(f32), st["s1"], st["s2"], st["sc"],
                 lr, c0, c1, c2)
    st["master"].copy_(m)
    st["flat"].copy_(m.to(bf16))
    st["grad"].zero_()
    st.update(images_of(st["flat"], H, K0, K0p))
    if st["p32"].numel():
        st["p32"].copy_(opt_step(opt, st["p32"], st["g32"], st["s1_32"],
                                 st["s2_32"], st["sc"], lr, c0, c1, c2))
        st["g32"].zero_()
    return st


def make_state(H, K0, K0p, opt, n32=14, seed=0, momentum=True):
    """A random state: non-zero base grads (the accumulate case), random
    scratch with non-zero w1 pad columns, images of the current weights."""
    g = torch.Generator().manual_seed(seed)
    _, n = layout(H, K0)

    def rn(*s, scale=1.0):
        return torch.randn(*s, generator=g) * scale
    st = {"master": rn(n, scale=0.1)}
    st["flat"] = st["master"].to(bf16)
    st["grad"] = rn(n, scale=0.5).to(bf16)
    st["wscratch"] = rn(H * K0p + 2 * H * H)
    st["bscratch"] = rn(4 * H + 1)
    need1 = opt in (ADAGRAD, ADAM) or (opt == SGD and momentum)
    st["s1"] = rn(n).abs() if need1 else None
    st["s2"] = rn(n).abs() if opt == ADAM else None
    st["p32"], st["g32"] = rn(n32), rn(n32)
    st["s1_32"] = rn(n32).abs() if need1 else None
    st["s2_32"] = rn(n32).abs() if opt == ADAM else None
    st["sc"] = torch.zeros(3) if opt == ADAM else None
    st.update(images_of(st["flat"], H, K0, K0p))
    return st


def clone_state(st):
    return {k: (v.clone() if torch.is_tensor(v) else v)
            for k, v in st.items()}


def check(got, want):
    """Names of the entries of `got` that differ from `want` (bit-exact,
    every buffer in full: scratches with pads, images with pads)."""
    bad = []
    for k, w in want.items():
        if w is None:
            continue
        if not torch.equal(got[k], w):
            bad.append(k)
    return bad
