"""The kernels of csrc/unet.hip one by one: every source kind of gcl_unet_conv3x3, gcl_unet_conv1x1_out, gcl_cascade_pack
and gcl_cascade_scores, with their value contracts.

Convolutions are held to e(hip) <= max(4 e(torch CPU float32 on the same inputs), 2^-20) against float64 on the CPU
(e(y) = max |y - y64| / max |y64|, unet_case.check).  Operands lie inside larger buffers (helpers/layouts.Guarded): NaN
around an input poisons a kernel that reads past it, a sentinel around an output shows a write past it.  The spatial
sizes are the levels of the 13 x 22 test shape (13x22, 6x11, 3x5, 1x2) and the 8 x 9 minimum: more than one block, tiles
cut by both edges, a single row, pools that drop a row or a column, pads in h only, in w only, in both and none."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import unet_case as UC  # noqa: E402
from layouts import NAN, SENT, Guarded, launched, same_bits, targs  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def norm_vectors(C, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.75 + 0.5 * torch.rand(C, generator=g), 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g),
            0.5 + torch.rand(C, generator=g))  # gamma, beta, mean, var


def virtual_input(kind, a, b=None, size=None):
    """The planar [B, Cin, H, W] tensor a source kind stands for, from its planar operands, by torch's own ops."""
    if kind in ("planar", "rows"):
        return a
    if kind == "pool":
        return F.max_pool2d(a, 2)
    up = F.interpolate(b, scale_factor=2, mode="bilinear", align_corners=True)
    up = F.pad(up, [0, size[1] - up.shape[3], 0, size[0] - up.shape[2]])
    return torch.cat([a, up], dim=1)


def conv_ref(xin, w, norm, dtype):
    y = F.conv2d(xin.to(dtype), w.to(dtype), padding=1)
    if norm is not None:
        g, bt, m, v = (t.to(dtype) for t in norm)
        y = F.gelu(F.batch_norm(y, m, v, g, bt, training=False, eps=EPS))
    return y


def rows_of(t):
    """planar [B, C, H, W] -> channels-last [B, H, W, C], contiguous."""
    return t.permute(0, 2, 3, 1).contiguous()


def run_conv(hip, kind, a, b, w, norm, H, W):
    """The kernel on guarded operands; returns the planar [B, Cout, H, W] output on the CPU."""
    B, Cout, Cin = a.shape[0], w.shape[0], w.shape[1]
    ga = Guarded(a.shape if kind == "planar" else rows_of(a).shape, fill=NAN, init=(a if kind == "planar" else rows_of(a)).to(DEV))
    gb = Guarded(rows_of(b).shape, fill=NAN, init=rows_of(b).to(DEV)) if b is not None else None
    K = {"planar": hip.UNET_PLANAR, "rows": hip.UNET_ROWS, "pool": hip.UNET_POOL, "upcat": hip.UNET_UPCAT}[kind]
    src = hip.unet_src(K, ga.view, gb.view if gb is not None else None)
    n = int(hip.lib().gcl_unet_packed_floats(Cin, Cout))
    gp = Guarded((n,), fill=SENT)
    hip.unet_pack_weights(w.to(DEV), out=gp.view)
    gy = Guarded((B, H, W, Cout), fill=SENT)
    nv = None if norm is None else tuple(Guarded(t.shape, fill=NAN, init=t.to(DEV)).view for t in norm)
    hip.unet_conv3x3(src, gp.view, nv, EPS, gy.view, Cin)
    torch.cuda.synchronize()
    assert gy.untouched() and gp.untouched(), "a write outside the output or the packed weights"
    return gy.view.permute(0, 3, 1, 2).cpu()


SIZES = [(13, 22), (6, 11), (3, 5), (1, 2), (8, 9)]
CHANNELS = [(7, 8, True), (40, 64, True), (96, 8, False), (96, 64, True), (7, 64, False)]  # Cin, Cout, norm


@pytest.mark.parametrize("kind", ["planar", "rows"])
@pytest.mark.parametrize("H,W", SIZES)
def test_conv_plain_sources(hip, kind, H, W):
    for k, (Cin, Cout, has_norm) in enumerate(CHANNELS):
        B = 2
        a = rnd(B, Cin, H, W, seed=100 + k)
        w = rnd(Cout, Cin, 3, 3, seed=200 + k, scale=1.5 / (9 * Cin) ** 0.5)
        norm = norm_vectors(Cout, 300 + k) if has_norm else None
        got = run_conv(hip, kind, a, None, w, norm, H, W)
        UC.check(got, conv_ref(a.double(), w, norm, torch.float64), conv_ref(a, w, norm, torch.float32),
                 f"{kind} {H}x{W} Cin {Cin} Cout {Cout} norm {has_norm}")


@pytest.mark.parametrize("Hs,Ws", [(13, 22), (6, 11), (3, 5), (16, 18), (2, 2)])
def test_conv_pooled_source(hip, Hs, Ws):
    H, W = Hs // 2, Ws // 2
    for k, (Cin, Cout, has_norm) in enumerate(CHANNELS):
        a = rnd(2, Cin, Hs, Ws, seed=400 + k)
        w = rnd(Cout, Cin, 3, 3, seed=500 + k, scale=1.5 / (9 * Cin) ** 0.5)
        norm = norm_vectors(Cout, 600 + k) if has_norm else None
        got = run_conv(hip, "pool", a, None, w, norm, H, W)
        xin = virtual_input("pool", a)
        UC.check(got, conv_ref(xin.double(), w, norm, torch.float64), conv_ref(xin, w, norm, torch.float32),
                 f"pool {Hs}x{Ws} Cin {Cin} Cout {Cout} norm {has_norm}")


# (H, W) of the skip, (h, w) of the low tensor: pad in h only, in w only, in both from a single row, in w at the minimum,
# none
UPCAT_SIZES = [((13, 22), (6, 11)), ((6, 11), (3, 5)), ((3, 5), (1, 2)), ((8, 9), (4, 4)), ((6, 10), (3, 5)), ((2, 2), (1, 1))]
UPCAT_CHANNELS = [(3, 4, 8, True), (16, 24, 64, True), (32, 64, 8, False), (32, 64, 64, True), (5, 2, 64, False)]


@pytest.mark.parametrize("size,low", UPCAT_SIZES)
def test_conv_upsampled_concatenated_source(hip, size, low):
    H, W = size
    for k, (C1, C2, Cout, has_norm) in enumerate(UPCAT_CHANNELS):
        a, b = rnd(2, C1, H, W, seed=700 + k), rnd(2, C2, low[0], low[1], seed=750 + k)
        w = rnd(Cout, C1 + C2, 3, 3, seed=800 + k, scale=1.5 / (9 * (C1 + C2)) ** 0.5)
        norm = norm_vectors(Cout, 900 + k) if has_norm else None
        got = run_conv(hip, "upcat", a, b, w, norm, H, W)
        x64 = virtual_input("upcat", a.double(), b.double(), size)
        x32 = virtual_input("upcat", a, b, size)
        UC.check(got, conv_ref(x64, w, norm, torch.float64), conv_ref(x32, w, norm, torch.float32),
                 f"upcat {H}x{W} from {low[0]}x{low[1]} C1 {C1} C2 {C2} Cout {Cout} norm {has_norm}")


@pytest.mark.parametrize("Cin", [252, 256, 258, 328])
def test_conv_long_contraction(hip, Cin):
    """From Cin = 256 on a block has eight waves and chunks of 64 channels: either side of the threshold, a Cin that is
    no multiple of the chunk (328) and one that is staged element by element (258), through every source kind."""
    Cout, norm = 8, norm_vectors(8, 40)
    w = rnd(Cout, Cin, 3, 3, seed=41, scale=1.5 / (9 * Cin) ** 0.5)
    a = rnd(2, Cin, 6, 11, seed=42)
    got = run_conv(hip, "rows", a, None, w, norm, 6, 11)
    UC.check(got, conv_ref(a.double(), w, norm, torch.float64), conv_ref(a, w, norm, torch.float32), f"rows 6x11 Cin {Cin}")
    assert same_bits(run_conv(hip, "rows", a[1:], None, w, norm, 6, 11)[0], got[1]), "sample 1 alone differs"
    got = run_conv(hip, "planar", a, None, w, None, 6, 11)
    UC.check(got, conv_ref(a.double(), w, None, torch.float64), conv_ref(a, w, None, torch.float32), f"planar 6x11 Cin {Cin}")
    xin = virtual_input("pool", a)
    got = run_conv(hip, "pool", a, None, w, norm, 3, 5)
    UC.check(got, conv_ref(xin.double(), w, norm, torch.float64), conv_ref(xin, w, norm, torch.float32), f"pool 6x11 Cin {Cin}")
    C1 = Cin // 8 * 3 // 4 * 4 if Cin % 4 == 0 else 97
    skip, low = rnd(2, C1, 3, 5, seed=43), rnd(2, Cin - C1, 1, 2, seed=44)
    got = run_conv(hip, "upcat", skip, low, w, norm, 3, 5)
    x64, x32 = virtual_input("upcat", skip.double(), low.double(), (3, 5)), virtual_input("upcat", skip, low, (3, 5))
    UC.check(got, conv_ref(x64, w, norm, torch.float64), conv_ref(x32, w, norm, torch.float32), f"upcat 3x5 Cin {Cin}")


def test_conv_refuses_bad_shapes(hip):
    a = torch.zeros(1, 4, 4, 8, device=DEV)
    y = torch.zeros(1, 4, 4, 6, device=DEV)
    p = torch.zeros(int(hip.lib().gcl_unet_packed_floats(8, 8)), device=DEV)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        hip.unet_conv3x3(hip.unet_src(hip.UNET_ROWS, a), p, None, EPS, y, 8)
    with pytest.raises(RuntimeError, match="does not halve"):
        hip.unet_conv3x3(hip.unet_src(hip.UNET_POOL, a), p, None, EPS, torch.zeros(1, 3, 2, 8, device=DEV), 8)
    with pytest.raises(RuntimeError, match="does not fit"):
        hip.unet_conv3x3(hip.unet_src(hip.UNET_UPCAT, a[..., :4].contiguous(), a[..., 4:].contiguous()), p, None, EPS,
                         torch.zeros(1, 4, 4, 8, device=DEV), 8)


def _call_entry(hip, entry, src, H, W, Cin):
    """`entry` reading `src` as the Cin channels of a 1 x H x W input, every other operand a valid one (Cout = 8)."""
    y = torch.zeros(1, H, W, 8, device=DEV)
    if entry == "unet_conv3x3":
        hip.unet_conv3x3(src, torch.zeros(int(hip.lib().gcl_unet_packed_floats(Cin, 8)), device=DEV), None, EPS, y, Cin)
    elif entry == "unet_conv3x3_wgrad":
        hip.unet_conv3x3_wgrad(src, y, Cin)
    else:
        hip.unet_v2_conv1x1(src, torch.zeros(8, Cin, device=DEV), y, Cin)


@pytest.mark.parametrize("entry", ["unet_conv3x3", "unet_conv3x3_wgrad", "unet_v2_conv1x1"])
def test_source_refusals_at_every_entry(hip, entry):
    """Every entry point that takes a gcl_unet_src_t refuses a descriptor that does not describe its input, names itself
    in the message, and launches nothing."""
    a = torch.zeros(1, 4, 4, 8, device=DEV)
    skip, low = a[..., :4].contiguous(), a[..., 4:].contiguous()
    cases = [("does not halve", hip.unet_src(hip.UNET_POOL, a), 3, 2, 8),
             ("does not fit", hip.unet_src(hip.UNET_UPCAT, skip, low), 4, 4, 8),
             (r"C1 \+ C2", hip.unet_src(hip.UNET_UPCAT, skip, low), 4, 4, 12),
             ("UPCAT needs b", hip.UnetSrc(skip.data_ptr(), None, hip.UNET_UPCAT, 4, 4, 2, 2), 4, 4, 8),
             ("source kind", hip.UnetSrc(a.data_ptr(), None, 7, 0, 0, 0, 0), 4, 4, 8)]
    counters = (hip.unet_launches, hip.unet_train_launches, hip.unet_v2_launches)
    before = [c() for c in counters]
    for fragment, src, H, W, Cin in cases:
        with pytest.raises(RuntimeError, match=f"gcl_{entry}: .*{fragment}"):
            _call_entry(hip, entry, src, H, W, Cin)
    assert [c() for c in counters] == before, "a refused call launched a kernel"


def _one_float_in(t):
    """A contiguous copy of t that starts one float into a flat buffer: 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=DEV)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("kind", ["rows", "pool", "upcat"])
def test_scalar_and_16_byte_staging_give_the_same_values(hip, kind):
    """A source whose channels come in fours is staged with 16-byte reads when its operands are 16-byte aligned and
    element by element when one of them is not.  ROWS and POOL reads do no arithmetic: the convolution and the weight
    gradient give the same bits either way.  The UPCAT read interpolates, and the compiler contracts the bilinear
    expression differently in the two loops: there both results are held to the bound of the other
    convolution tests against float64.  B = 2, 6 x 11: two tiles across, tiles cut by both edges."""
    B, H, W, Cin, Cout = 2, 6, 11, 8, 8
    if kind == "upcat":  # a 6 x 11 x 4 skip and a 3 x 5 x 4 low tensor (padded in w); only the low tensor moves
        cpu = [rnd(B, H, W, 4, seed=61), rnd(B, 3, 5, 4, seed=62)]
    else:
        cpu = [rnd(B, *((13, 22) if kind == "pool" else (H, W)), Cin, seed=60)]
    ops = [t.to(DEV) for t in cpu]
    K = {"rows": hip.UNET_ROWS, "pool": hip.UNET_POOL, "upcat": hip.UNET_UPCAT}[kind]
    aligned = hip.unet_src(K, *ops)
    moved = ops[:-1] + [_one_float_in(ops[-1])]
    shifted = hip.unet_src(K, *moved)
    assert all(t.data_ptr() % 16 == 0 for t in ops)
    w, dZ = rnd(Cout, Cin, 3, 3, seed=63, scale=0.2), rnd(B, H, W, Cout, seed=64)
    packed, dZd = hip.unet_pack_weights(w.to(DEV)), dZ.to(DEV)

    def conv(src):
        return hip.unet_conv3x3(src, packed, None, EPS, torch.empty(B, H, W, Cout, device=DEV), Cin).permute(0, 3, 1, 2)

    def conv_oracle(dtype):
        planar = [t.permute(0, 3, 1, 2).to(dtype) for t in cpu]
        return conv_ref(virtual_input(kind, *planar, size=(H, W)), w, None, dtype)

    def wgrad_oracle(dtype):
        planar = [t.permute(0, 3, 1, 2).to(dtype) for t in cpu]
        wz = torch.zeros(Cout, Cin, 3, 3, dtype=dtype, requires_grad=True)
        F.conv2d(virtual_input(kind, *planar, size=(H, W)), wz, padding=1).backward(dZ.permute(0, 3, 1, 2).to(dtype))
        return wz.grad

    for what, kern, run, oracle in (("conv3x3", "unet_conv3x3_kernel", conv, conv_oracle),
                                    ("wgrad", "unet_wgrad_kernel", lambda src: hip.unet_conv3x3_wgrad(src, dZd, Cin), wgrad_oracle)):
        (vec, one), names = launched(lambda: (run(aligned), run(shifted)))
        assert sorted(t[1] for t in targs(names, kern)) == ["1", "4"], f"{what}: both read widths were to run, got {names}"
        differ = int((vec != one).sum())
        print(f"[unet] {kind} {what}: {differ} of {vec.numel()} elements differ between the read widths, "
              f"max |difference| {float((vec - one).abs().max()):.3e}")
        if kind == "upcat":
            y64, y32 = oracle(torch.float64), oracle(torch.float32)
            UC.check(vec.cpu(), y64, y32, f"upcat {what}, 16-byte reads")
            UC.check(one.cpu(), y64, y32, f"upcat {what}, scalar reads")
        else:
            assert not vec.isnan().any() and same_bits(vec, one), f"{kind} {what}: the two read widths differ"


# ---------------------------------------------------------------------------------------------------------------------
# Value contracts of the convolution
# ---------------------------------------------------------------------------------------------------------------------
def _rows_conv(hip, a, w, norm):
    B, Cin, H, W = a.shape
    return run_conv(hip, "rows", a, None, w, norm, H, W)


def test_nan_stays_in_its_sample(hip):
    a = rnd(3, 40, 13, 22, seed=1)
    w, norm = rnd(64, 40, 3, 3, seed=2, scale=0.08), norm_vectors(64, 3)
    clean = _rows_conv(hip, a, w, norm)
    bad = a.clone()
    bad[1, 17, 5, 9] = NAN
    got = _rows_conv(hip, bad, w, norm)
    assert same_bits(got[0], clean[0]) and same_bits(got[2], clean[2])
    hit = got[1].isnan().any(dim=0)
    want = torch.zeros(13, 22, dtype=torch.bool)
    want[4:7, 8:11] = True  # the nine pixels whose taps read it, every output channel
    assert torch.equal(hit, want) and bool(got[1][:, 4:7, 8:11].isnan().all())


def test_sample_bits_do_not_depend_on_the_batch(hip):
    low = rnd(3, 24, 3, 5, seed=4)
    a = rnd(3, 16, 6, 11, seed=5)
    w, norm = rnd(64, 40, 3, 3, seed=6, scale=0.08), norm_vectors(64, 7)
    full = run_conv(hip, "upcat", a, low, w, norm, 6, 11)
    again = run_conv(hip, "upcat", a, low, w, norm, 6, 11)
    assert same_bits(full, again), "two calls differ"
    for b in range(3):
        one = run_conv(hip, "upcat", a[b:b + 1], low[b:b + 1], w, norm, 6, 11)
        assert same_bits(one[0], full[b]), f"sample {b} alone differs from its row of B = 3"


def test_pooled_read_nan_rule(hip):
    """A NaN in a 2x2 window gives NaN (wherever it stands in the window), as torch's max_pool2d; a NaN in the dropped
    last row or column is never read."""
    a = rnd(1, 8, 7, 9, seed=8)  # pooled: 3 x 4; row 6 and column 8 are dropped
    w = rnd(8, 8, 3, 3, seed=9, scale=0.1)
    clean = run_conv(hip, "pool", a, None, w, None, 3, 4)
    dropped = a.clone()
    dropped[0, :, 6, :] = NAN
    dropped[0, :, :, 8] = NAN
    assert same_bits(run_conv(hip, "pool", dropped, None, w, None, 3, 4), clean)
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        bad = a.clone()
        bad[0, 3, 2 + dy, 4 + dx] = NAN  # window (1, 2)
        got = run_conv(hip, "pool", bad, None, w, None, 3, 4)
        want = conv_ref(F.max_pool2d(bad, 2), w, None, torch.float32)
        assert bool(F.max_pool2d(bad, 2)[0, 3, 1, 2].isnan())
        assert torch.equal(got.isnan(), want.isnan()) and bool(got.isnan().any())
        assert torch.allclose(got.nan_to_num(0.0), want.nan_to_num(0.0), atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------------
# The output convolution
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cout", [3, 19])
@pytest.mark.parametrize("Fw", [8, 64])
def test_conv1x1_out(hip, Cout, Fw):
    B, H, W, Cx = 2, 13, 22, 2 * Cout + 2
    x = rnd(B, Fw, H, W, seed=10)
    w, bias = rnd(Cout, Fw, 1, 1, seed=11, scale=Fw ** -0.5), rnd(Cout, seed=12)
    gx = Guarded((B, H, W, Fw), fill=NAN, init=rows_of(x).to(DEV))
    gy = Guarded((B, Cout, H, W), fill=SENT)
    hip.unet_conv1x1_out(gx.view, w.view(Cout, Fw).to(DEV), bias.to(DEV), gy.view)
    torch.cuda.synchronize()
    assert gy.untouched()
    plain = gy.view.clone()
    UC.check(plain, F.conv2d(x.double(), w.double(), bias.double()), F.conv2d(x, w, bias), f"1x1 Cout {Cout} F {Fw}")
    xin = Guarded((B, Cx, H, W), fill=NAN, init=rnd(B, Cx, H, W, seed=13).to(DEV))
    res = xin.view[:, Cout:2 * Cout]  # the channel slice of a wider planar tensor
    gy2 = Guarded((B, Cout, H, W), fill=SENT)
    hip.unet_conv1x1_out(gx.view, w.view(Cout, Fw).to(DEV), bias.to(DEV), gy2.view, residual=res, res_bs=xin.view.stride(0))
    torch.cuda.synchronize()
    assert gy2.untouched()
    assert same_bits(gy2.view, plain + res), "the residual sum is not the float32 sum of the two, rounded once"


# ---------------------------------------------------------------------------------------------------------------------
# The cascade's glue and scores
# ---------------------------------------------------------------------------------------------------------------------
def _vectors(C, seed):
    r = np.random.default_rng(seed)
    return [(r.normal(size=C) * 10).astype(np.float32), (0.5 + r.random(C) * 5).astype(np.float32),
            (r.normal(size=C) * 10).astype(np.float32), (0.5 + r.random(C) * 5).astype(np.float32)]  # gm, gs, dm, ds


@pytest.mark.parametrize("Ns", [2, 0])
def test_cascade_pack_is_the_numpy_restatement(hip, Ns):
    B, H, W, C, obs = 3, 13, 22, 5, 2
    r = np.random.default_rng(21)
    coarse = r.normal(size=(B, H, W, C)).astype(np.float32)
    static = r.normal(size=(W, H, Ns)).astype(np.float32) if Ns else None
    gm, gs, dm, ds = _vectors(C, 22)
    gphys, gX = Guarded((B, H, W, C), fill=SENT), Guarded((B, obs * C + Ns, H, W), fill=SENT)
    dev = lambda v: None if v is None else torch.from_numpy(v).to(DEV)  # noqa: E731
    hip.cascade_pack(dev(coarse), dev(gm), dev(gs), dev(dm), dev(ds), dev(static), obs, coarse_phys=gphys.view, X=gX.view)
    torch.cuda.synchronize()
    assert gphys.untouched() and gX.untouched()
    for b in range(B):  # predict_cascade.py:346-354, one sample at a time as the reference runs it
        phys = coarse[b] * gs + gm
        assert phys.dtype == np.float32
        norm = (phys - dm) / ds
        stack = np.concatenate([norm] * obs, axis=-1).transpose(2, 0, 1)
        if Ns:
            stack = np.concatenate([stack, static.transpose(2, 1, 0)], axis=0)
        assert same_bits(gphys.view[b].cpu(), torch.from_numpy(phys)), f"coarse_phys of sample {b}"
        assert same_bits(gX.view[b].cpu(), torch.from_numpy(np.ascontiguousarray(stack))), f"X of sample {b}"


def _scores64(out, phys, fine, tf, tp, dm, ds):
    """predict_cascade.py:360-372 for one sample: float32 differences and squares as the reference forms them, the mean
    in float64.  [C, 3] = (gnn, cascade, persistence)."""
    C = out.shape[0]  # (the archive may hold more features than are scored)
    target = fine[tf].astype(np.float32).transpose(1, 0, 2)[..., :C]
    persist = fine[tp].astype(np.float32).transpose(1, 0, 2)[..., :C]
    casc = out.transpose(1, 2, 0) * ds + dm
    assert casc.dtype == np.float32
    sq = lambda d: np.mean(((d) ** 2).astype(np.float64), axis=(0, 1))  # noqa: E731
    return np.stack([sq(phys - target), sq(casc - target), sq(persist - target)], axis=1)


def test_cascade_scores(hip):
    B, H, W, C, T, AR, nf = 4, 13, 22, 5, 6, 3, 6
    r = np.random.default_rng(31)
    out = r.normal(size=(B, C, H, W)).astype(np.float32)
    phys = (r.normal(size=(B, H, W, C)) * 8).astype(np.float32)
    fine = (r.normal(size=(T, W, H, nf)) * 8).astype(np.float16)
    _, _, dm, ds = _vectors(C, 32)
    tf = np.array([2, 6, 5, -1], dtype=np.int64)  # sample 1 runs past the archive, sample 3 starts before it
    tp = np.array([1, 3, 0, 2], dtype=np.int64)
    state = torch.zeros(AR, C, 3, dtype=torch.float64, device=DEV)
    state[1] = 0.5
    count = torch.tensor([0, 10, 0], dtype=torch.int64, device=DEV)
    need = int(hip.lib().gcl_cascade_scores_ws_bytes(B, H, W, C))
    ws = Guarded((need // 8,), dtype=torch.float64, fill=SENT)
    dev = lambda v: torch.from_numpy(v).to(DEV)  # noqa: E731
    args = (dev(out), dev(phys), dev(fine), dev(tf), dev(tp), dev(dm), dev(ds))
    hip.cascade_scores(*args, state, count, 1, ws=ws.view)
    torch.cuda.synchronize()
    assert ws.untouched()
    want = np.full((C, 3), 0.5)
    for b in (0, 2):
        want = want + _scores64(out[b], phys[b], fine, tf[b], tp[b], dm, ds)
    got = state.cpu().numpy()
    assert count.tolist() == [0, 12, 0]
    assert (got[0] == 0).all() and (got[2] == 0).all()
    rel = np.abs(got[1] - want) / np.abs(want)
    print(f"[unet] cascade scores: worst relative error {rel.max():.3e} (bound {2.0 ** -22:.3e})")
    assert (rel <= 2.0 ** -22).all()
    # the batch does not reach the bits: one sample at a time gives the same state
    state1 = torch.zeros_like(state)
    state1[1] = 0.5
    count1 = torch.tensor([0, 10, 0], dtype=torch.int64, device=DEV)
    o_d, p_d, f_d, tf_d, tp_d, dm_d, ds_d = args
    for b in range(B):
        hip.cascade_scores(o_d[b:b + 1], p_d[b:b + 1], f_d, tf_d[b:b + 1], tp_d[b:b + 1], dm_d, ds_d, state1, count1, 1)
    assert same_bits(state1, state) and count1.tolist() == [0, 12, 0]
