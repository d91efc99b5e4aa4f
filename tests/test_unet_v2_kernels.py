"""The kernels of csrc/unet_v2.hip one by one through their hip.py wrappers: GroupNorm statistics and apply, the 1x1
convolution over every source kind, the block tail (skip add, channel means, SE gate), LayerNorm, the attention core and
the three spectral kernels.

Each is held to e(hip) <= max(4 e(torch CPU float32 on the same inputs), 2^-20) against float64 torch ops on the CPU
(e(y) = max |y - y64| / max |y64|, unet_case.check).  Operands lie inside larger buffers (helpers/layouts.Guarded): NaN
around an input poisons a kernel that reads past it, a sentinel around an output shows a write past it."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import unet_v2_case as VC  # noqa: E402
from layouts import NAN, SENT, Guarded, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def rows_of(t):
    """planar [B, C, H, W] -> channels-last [B, H, W, C], contiguous."""
    return t.permute(0, 2, 3, 1).contiguous()


def planar_of(t):
    return t.permute(0, 3, 1, 2).contiguous()


def gin(t):
    """A device copy of t between NaN guards."""
    return Guarded(t.shape, fill=NAN, init=t.to(DEV)).view


# ---------------------------------------------------------------------------------------------------------------------
# GroupNorm
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,G", [(8, 8), (16, 8), (12, 6), (20, 5), (512, 8)])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (5, 7), (13, 22)])
def test_group_norm(hip, C, G, H, W):
    """Statistics and apply + GELU on 100 + randn: |mean| >> spread."""
    B = 2
    z = 100.0 + rnd(B, C, H, W, seed=C + H)
    gamma, beta = 0.75 + 0.5 * torch.rand(C, generator=torch.Generator().manual_seed(1)), rnd(C, seed=2, scale=0.2)
    gm, gi, gout = Guarded((B, G), fill=SENT), Guarded((B, G), fill=SENT), Guarded((B, H, W, C), fill=SENT)
    zd = gin(rows_of(z))
    hip.unet_v2_gn_stats(zd, G, EPS, gm.view, gi.view)
    hip.unet_v2_gn_gelu(zd, gin(gamma), gin(beta), gm.view, gi.view, gout.view)
    torch.cuda.synchronize()
    assert gm.untouched() and gi.untouched() and gout.untouched()
    z64 = z.double().view(B, G, -1)
    VC.check(gm.view, z64.mean(dim=2), z.view(B, G, -1).mean(dim=2), f"gn mean C {C} G {G} {H}x{W}")
    got = planar_of(gout.view.cpu())
    if C == G and H * W == 1:
        # one value per group: the variance is 0, the normalised value exactly 0, the output gelu(beta)
        assert same_bits(gm.view.cpu(), z.view(B, G))
        want = F.gelu(beta.double()).view(1, C, 1, 1).expand(B, C, 1, 1)
        assert float((got.double() - want).abs().max()) <= 2.0 ** -22, "gelu(beta) expected where the variance is 0"
        return
    i64 = 1.0 / torch.sqrt(z64.var(dim=2, unbiased=False) + EPS)
    i32 = 1.0 / torch.sqrt(z.view(B, G, -1).var(dim=2, unbiased=False) + EPS)
    VC.check(gi.view, i64, i32, f"gn invstd C {C} G {G} {H}x{W}")
    y64 = F.gelu(F.group_norm(z.double(), G, gamma.double(), beta.double(), EPS))
    y32 = F.gelu(F.group_norm(z, G, gamma, beta, EPS))
    VC.check(got, y64, y32, f"gn apply C {C} G {G} {H}x{W}")


# ---------------------------------------------------------------------------------------------------------------------
# The 1x1 convolution over a source
# ---------------------------------------------------------------------------------------------------------------------
def virtual_input(kind, a, b=None, size=None):
    if kind in ("planar", "rows"):
        return a
    if kind == "pool":
        return F.max_pool2d(a, 2)
    up = F.interpolate(b, scale_factor=2, mode="bilinear", align_corners=True)
    up = F.pad(up, [0, size[1] - up.shape[3], 0, size[0] - up.shape[2]])
    return torch.cat([a, up], dim=1)


def run_pw(hip, kind, a, b, w, H, W, ld=None, c0=0):
    B, Cout = a.shape[0], (w.shape[0] if w is not None else a.shape[1])
    Cin = w.shape[1] if w is not None else a.shape[1]
    ga = gin(a if kind == "planar" else rows_of(a))
    gb = gin(rows_of(b)) if b is not None else None
    K = {"planar": hip.UNET_PLANAR, "rows": hip.UNET_ROWS, "pool": hip.UNET_POOL, "upcat": hip.UNET_UPCAT}[kind]
    src = hip.unet_src(K, ga, gb)
    ld = Cout if ld is None else ld
    gy = Guarded((B, H, W, ld), fill=SENT)
    out = gy.view[..., c0:c0 + Cout]
    hip.unet_v2_conv1x1(src, None if w is None else gin(w), out, Cin)
    torch.cuda.synchronize()
    assert gy.untouched(), "a write outside the output"
    if ld != Cout:
        rest = torch.ones(ld, dtype=torch.bool)
        rest[c0:c0 + Cout] = False
        assert bool((gy.view[..., rest.to(DEV)] == SENT).all()), "a write outside the channel slice"
    return planar_of(out.cpu())


PW_CHANNELS = [(6, 8), (40, 64), (96, 8), (70, 132)]  # Cin, Cout: below / above a stage of 32, more than one channel tile


@pytest.mark.parametrize("kind", ["planar", "rows"])
@pytest.mark.parametrize("H,W", [(13, 22), (3, 5), (1, 2), (8, 9)])
def test_conv1x1_plain_sources(hip, kind, H, W):
    for k, (Cin, Cout) in enumerate(PW_CHANNELS):
        a, w = rnd(2, Cin, H, W, seed=10 + k), rnd(Cout, Cin, seed=20 + k, scale=Cin ** -0.5)
        got = run_pw(hip, kind, a, None, w, H, W)
        ref = lambda t: F.conv2d(a.to(t), w.to(t)[:, :, None, None])  # noqa: E731
        VC.check(got, ref(torch.float64), ref(torch.float32), f"1x1 {kind} {H}x{W} Cin {Cin} Cout {Cout}")


@pytest.mark.parametrize("Hs,Ws", [(13, 22), (6, 11), (3, 5), (27, 45)])
def test_conv1x1_pooled_source(hip, Hs, Ws):
    for k, (Cin, Cout) in enumerate(PW_CHANNELS):
        a, w = rnd(2, Cin, Hs, Ws, seed=30 + k), rnd(Cout, Cin, seed=40 + k, scale=Cin ** -0.5)
        got = run_pw(hip, "pool", a, None, w, Hs // 2, Ws // 2)
        ref = lambda t: F.conv2d(F.max_pool2d(a.to(t), 2), w.to(t)[:, :, None, None])  # noqa: E731
        VC.check(got, ref(torch.float64), ref(torch.float32), f"1x1 pool {Hs}x{Ws} Cin {Cin} Cout {Cout}")


@pytest.mark.parametrize("size,low", [((13, 22), (6, 11)), ((6, 11), (3, 5)), ((3, 5), (1, 2)), ((27, 45), (13, 22)),
                                      ((6, 10), (3, 5))])
def test_conv1x1_upsampled_concatenated_source(hip, size, low):
    H, W = size
    for k, (C1, C2, Cout) in enumerate([(3, 4, 8), (16, 24, 64), (32, 64, 8), (5, 2, 68)]):
        a, b = rnd(2, C1, H, W, seed=50 + k), rnd(2, C2, low[0], low[1], seed=60 + k)
        w = rnd(Cout, C1 + C2, seed=70 + k, scale=(C1 + C2) ** -0.5)
        got = run_pw(hip, "upcat", a, b, w, H, W)
        ref = lambda t: F.conv2d(virtual_input("upcat", a.to(t), b.to(t), size), w.to(t)[:, :, None, None])  # noqa: E731
        VC.check(got, ref(torch.float64), ref(torch.float32), f"1x1 upcat {H}x{W} C1 {C1} C2 {C2} Cout {Cout}")


def test_conv1x1_identity_slice_bias_and_residual(hip):
    """w None copies the source (the identity skip); a channel slice of wider rows as the output; bias and residual as
    the attention's projection uses them."""
    a = rnd(2, 8, 13, 22, seed=80)
    assert same_bits(run_pw(hip, "planar", a, None, None, 13, 22), a)
    assert same_bits(run_pw(hip, "pool", a, None, None, 6, 11), F.max_pool2d(a, 2))
    w = rnd(12, 8, seed=81, scale=0.4)
    whole = run_pw(hip, "rows", a, None, w, 13, 22)
    assert same_bits(run_pw(hip, "rows", a, None, w, 13, 22, ld=32, c0=16), whole)
    bias, res = rnd(12, seed=82), rnd(2, 13, 22, 12, seed=83)
    out = Guarded((2, 13, 22, 12), fill=SENT)
    ra = gin(rows_of(a))  # the descriptor holds a pointer only: the tensor has to outlive the launch
    hip.unet_v2_conv1x1(hip.unet_src(hip.UNET_ROWS, ra), gin(w), out.view, 8, bias=gin(bias), res=gin(res))
    torch.cuda.synchronize()
    assert out.untouched()
    assert same_bits(out.view.cpu(), res + (rows_of(whole) + bias)), "not res + (conv + bias), each sum rounded once"


# ---------------------------------------------------------------------------------------------------------------------
# The block tail
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,hid,G", [(4, 4, 4), (8, 4, 8), (12, 4, 6), (512, 64, 8)])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (13, 22)])
def test_block_tail(hip, C, hid, G, H, W):
    B = 2
    z, skip = rnd(B, C, H, W, seed=90 + C), rnd(B, C, H, W, seed=91 + C)
    gamma, beta = 0.75 + 0.5 * torch.rand(C, generator=torch.Generator().manual_seed(3)), rnd(C, seed=92, scale=0.2)
    w1, b1 = rnd(hid, C, seed=93, scale=1.5 * C ** -0.5), rnd(hid, seed=94)
    w2, b2 = rnd(C, hid, seed=95, scale=1.5 * hid ** -0.5), rnd(C, seed=96)
    zd = gin(rows_of(z))
    mean, invstd = hip.unet_v2_gn_stats(zd, G, EPS)
    gout = Guarded((B, H, W, C), fill=SENT)
    need = hip.unet_v2_tail_ws_bytes(B, H * W, C)
    ws = Guarded((need // 8,), dtype=torch.float64, fill=SENT)
    hip.unet_v2_block_tail(zd, gin(gamma), gin(beta), mean, invstd, gin(rows_of(skip)), gin(w1), gin(b1), gin(w2), gin(b2),
                           out=gout.view, ws=ws.view)
    torch.cuda.synchronize()
    assert gout.untouched() and ws.untouched()

    def ref(t):
        u = F.gelu(F.group_norm(z.to(t), G, gamma.to(t), beta.to(t), EPS)) + skip.to(t)
        gate = torch.sigmoid(F.linear(F.gelu(F.linear(u.mean(dim=(2, 3)), w1.to(t), b1.to(t))), w2.to(t), b2.to(t)))
        return u * gate[:, :, None, None]

    got = planar_of(gout.view.cpu())
    VC.check(got, ref(torch.float64), ref(torch.float32), f"tail C {C} hidden {hid} {H}x{W}")
    one = hip.unet_v2_block_tail(zd[1:].contiguous(), gin(gamma), gin(beta), mean[1:].contiguous(), invstd[1:].contiguous(),
                                 gin(rows_of(skip)[1:]), gin(w1), gin(b1), gin(w2), gin(b2))
    assert same_bits(one[0], gout.view[1]), "sample 1 alone differs from its row of B = 2"


# ---------------------------------------------------------------------------------------------------------------------
# Attention
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [32, 96, 520])
def test_layernorm(hip, C):
    x = 3.0 + rnd(2, 35, C, seed=C)
    gamma, beta = 0.75 + 0.5 * torch.rand(C, generator=torch.Generator().manual_seed(4)), rnd(C, seed=5, scale=0.2)
    out = Guarded((2, 35, C), fill=SENT)
    hip.unet_v2_layernorm(gin(x), gin(gamma), gin(beta), EPS, out.view)
    torch.cuda.synchronize()
    assert out.untouched()
    ref = lambda t: F.layer_norm(x.to(t), (C,), gamma.to(t), beta.to(t), EPS)  # noqa: E731
    VC.check(out.view, ref(torch.float64), ref(torch.float32), f"layernorm C {C}")


@pytest.mark.parametrize("N", [1, 2, 35, 320])
@pytest.mark.parametrize("D,heads", [(8, 4), (24, 2), (128, 1), (5, 3)])
def test_attention_core(hip, N, D, heads):
    """One query's scores are shifted by +80: the softmax needs its max-subtraction."""
    B, C = 2, heads * D
    qkv = rnd(B, N, 3, heads, D, seed=N + D)
    shift = rnd(D, seed=9)
    qkv[1, :, 1, 0] += shift  # every key of (sample 1, head 0) gains one vector, and query 0 enough of it
    qkv[1, 0, 0, 0] += shift * (80.0 * D ** 0.5 / float(shift @ shift))  # that its scores all move up by about 80
    out = Guarded((B, N, C), fill=SENT)
    hip.unet_v2_attention(gin(qkv.view(B, N, 3 * C)), heads, out.view)
    torch.cuda.synchronize()
    assert out.untouched()

    def ref(t):
        q, k, v = qkv.to(t).permute(2, 0, 3, 1, 4).unbind(0)
        s = (q @ k.transpose(-2, -1)) * D ** -0.5
        return (s.softmax(dim=-1) @ v).transpose(1, 2).reshape(B, N, C), s

    y64, s64 = ref(torch.float64)
    assert float(s64[1, 0, 0].mean()) > 50.0, "the test's shifted row is not shifted"
    VC.check(out.view, y64, ref(torch.float32)[0], f"attention N {N} D {D} heads {heads}")
    one = hip.unet_v2_attention(gin(qkv[1:].reshape(1, N, 3 * C)), heads)
    assert same_bits(one[0], out.view[1]), "sample 1 alone differs from its row of B = 2"


def test_attention_refuses_long_sequences(hip):
    with pytest.raises(ValueError, match="4096"):
        hip.unet_v2_attention(torch.zeros(1, 4097, 24, device=DEV), 2)


# ---------------------------------------------------------------------------------------------------------------------
# The spectral convolution
# ---------------------------------------------------------------------------------------------------------------------
GRIDS = [(1, 1), (1, 2), (1, 6), (2, 8), (3, 5), (4, 4), (5, 6), (5, 7), (8, 8)]


@pytest.mark.parametrize("Hb,Wb", GRIDS)
@pytest.mark.parametrize("C", [8, 64])
def test_spectral(hip, Hb, Wb, C):
    """Forward transform, mode mix and inverse, each against torch.fft (complex128 as the oracle, complex64 as the
    float32 CPU figure), then the three in a row against the layer."""
    B, M = 3, 4
    mh, mw = hip.spectral_modes(Hb, Wb, M, M)
    x = rnd(B, C, Hb, Wb, seed=Hb * 10 + Wb)
    w_re, w_im = rnd(C, C, M, M, seed=6, scale=C ** -0.5), rnd(C, C, M, M, seed=7, scale=C ** -0.5)
    packed = Guarded((mh * mw, C, C, 2), fill=SENT)
    hip.unet_v2_spectral_pack(gin(w_re), gin(w_im), mh, mw, out=packed.view)
    gX, gO = Guarded((B, mh * mw, C, 2), fill=SENT), Guarded((B, mh * mw, C, 2), fill=SENT)
    gy = Guarded((B, Hb, Wb, 2 * C), fill=SENT)
    hip.unet_v2_spectral_fwd(gin(rows_of(x)), mh, mw, gX.view)
    hip.unet_v2_spectral_mix(gX.view, packed.view, gO.view)
    hip.unet_v2_spectral_inv(gO.view, gy.view[..., C:], mh, mw)
    torch.cuda.synchronize()
    assert packed.untouched() and gX.untouched() and gO.untouched() and gy.untouched()
    assert bool((gy.view[..., :C] == SENT).all()), "a write outside the channel slice"
    wc = torch.complex(w_re, w_im)[:, :, :mh, :mw]
    assert same_bits(packed.view.cpu(), torch.view_as_real(wc.permute(2, 3, 0, 1).reshape(mh * mw, C, C).contiguous()))

    def modes_of(t):  # [B, mode, C] complex
        return torch.fft.rfft2(x.to(t), norm="ortho")[:, :, :mh, :mw].permute(0, 2, 3, 1).reshape(B, mh * mw, C)

    def cplx(g):
        return torch.view_as_complex(g.view.cpu().contiguous())

    def as_real(c):
        return torch.view_as_real(c)

    X64, X32 = modes_of(torch.float64), modes_of(torch.float32)
    VC.check(as_real(cplx(gX)), as_real(X64), as_real(X32), f"spectral fwd {Hb}x{Wb} C {C}")
    # the mix and the inverse from the kernel's own input, so that each step is judged alone
    Xg = cplx(gX)
    wm = wc.permute(2, 3, 0, 1).reshape(mh * mw, C, C)
    mix = lambda X, w: torch.einsum("bmi,mio->bmo", X, w)  # noqa: E731
    VC.check(as_real(cplx(gO)), as_real(mix(Xg.to(torch.complex128), wm.to(torch.complex128))), as_real(mix(Xg, wm)),
             f"spectral mix {Hb}x{Wb} C {C}")

    def inverse(O):  # [B, mode, C] complex -> [B, C, Hb, Wb]
        full = torch.zeros(B, C, Hb, Wb // 2 + 1, dtype=O.dtype)
        full[:, :, :mh, :mw] = O.reshape(B, mh, mw, C).permute(0, 3, 1, 2)
        return torch.fft.irfft2(full, s=(Hb, Wb), norm="ortho")

    Og = cplx(gO)
    got = planar_of(gy.view[..., C:].cpu())
    VC.check(got, inverse(Og.to(torch.complex128)), inverse(Og), f"spectral inverse {Hb}x{Wb} C {C}")
    VC.check(got, VC.spectral(w_re.double(), w_im.double(), x.double(), M, M), VC.spectral(w_re, w_im, x, M, M),
             f"spectral layer {Hb}x{Wb} C {C}")
    # five samples: the second pass over the weights (four samples per pass) gives sample 4 the bits it has alone
    x5 = rnd(5, C, Hb, Wb, seed=8)
    X5 = hip.unet_v2_spectral_fwd(rows_of(x5).to(DEV), mh, mw)
    O5 = hip.unet_v2_spectral_mix(X5, packed.view)
    O1 = hip.unet_v2_spectral_mix(X5[4:].contiguous(), packed.view)
    assert same_bits(O1[0], O5[4])
