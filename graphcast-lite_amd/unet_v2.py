"""The second regional U-Net of the reference (`src/unet/model_v2.py::WeatherUNetV2`) in eval mode on the HIP path.

The module tree, parameter names and shapes are the reference's, so `load_state_dict(torch.load("best_model.pth"))` of a
reference checkpoint works with `strict=True` (97 keys; 96 when `in_channels == base_filters`, where `inc.skip` is an
`nn.Identity`).

A forward is 72 launches, whatever B, H and W are:

    8 ResConvBlocks (inc, down1..3, bottleneck_mix, up1..3) x 9:
        conv3x3 (raw) . gn_stats . gn_gelu . conv3x3 (raw) . gn_stats . skip 1x1 . block tail (2 launches: u = gelu(GN) +
        skip with the channel sums; the SE gate and the in-place scale)
    attention x 4:   layernorm . qkv linear . softmax(q k^T) v . proj linear + bias + residual on the normalised tokens
    spectral x 3:    forward transform . per-mode channel mix . inverse transform
    out_conv x 1

17 of them are `csrc/unet.hip`'s (`gcl_unet_conv3x3` with gamma NULL, `gcl_unet_conv1x1_out`; counted by
`hip.unet_launches`), 55 are `csrc/unet_v2.hip`'s (`hip.unet_v2_launches`).  MaxPool2d, the bilinear Upsample, the pad and
both concatenations are not launches: the pooled / upsampled input is how a block's first convolution and its skip read
their source, and the attention and spectral branches write the two channel halves of one buffer.  Activations are
channels-last `[B, H, W, C]` float32 tensors of a per-shape workspace the module holds.  Training V2 is not provided.
"""
import torch
import torch.nn as nn

from . import hip
from .unet import _levels, _pack_cached, _Part, _UNetBase

MAX_TOKENS = 4096  # bottleneck pixels the attention kernel takes


class SEBlock(_Part):
    """Squeeze-and-excitation (model_v2.py:22-37)."""

    def __init__(self, ch: int, reduction: int = 8):
        super().__init__()
        hid = max(ch // reduction, 4)
        self.fc = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(ch, hid), nn.GELU(), nn.Linear(hid, ch),
                                nn.Sigmoid())


class ResConvBlock(_Part):
    """Conv3x3 -> GN -> GELU -> Conv3x3 -> GN -> GELU, + skip, SE (model_v2.py:40-60)."""

    def __init__(self, in_ch: int, out_ch: int, num_groups: int = 8):
        super().__init__()
        g = min(num_groups, out_ch)
        while out_ch % g != 0 and g > 1:
            g -= 1
        self.conv = nn.Sequential(
            nn.Conv2d(in_ch, out_ch, 3, padding=1, bias=False), nn.GroupNorm(g, out_ch), nn.GELU(),
            nn.Conv2d(out_ch, out_ch, 3, padding=1, bias=False), nn.GroupNorm(g, out_ch), nn.GELU())
        self.skip = nn.Conv2d(in_ch, out_ch, 1, bias=False) if in_ch != out_ch else nn.Identity()
        self.se = SEBlock(out_ch)
        self.in_ch, self.out_ch = in_ch, out_ch


class SelfAttention2D(_Part):
    """Multi-head self-attention over the pixels (model_v2.py:63-92)."""

    def __init__(self, dim: int, heads: int = 4):
        super().__init__()
        self.heads, self.head_dim = heads, dim // heads
        self.scale = self.head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=False)
        self.proj = nn.Linear(dim, dim)
        self.norm = nn.LayerNorm(dim)


class SpectralConv2d(_Part):
    """The Fourier layer (model_v2.py:95-122)."""

    def __init__(self, in_ch: int, out_ch: int, modes_h: int = 4, modes_w: int = 4):
        super().__init__()
        self.modes_h, self.modes_w = modes_h, modes_w
        scale = 1 / (in_ch * out_ch)
        self.weights_re = nn.Parameter(scale * torch.randn(in_ch, out_ch, modes_h, modes_w))
        self.weights_im = nn.Parameter(scale * torch.randn(in_ch, out_ch, modes_h, modes_w))


class Down(_Part):
    def __init__(self, in_ch: int, out_ch: int):
        super().__init__()
        self.pool = nn.MaxPool2d(2)
        self.conv = ResConvBlock(in_ch, out_ch)


class Up(_Part):
    def __init__(self, in_ch: int, out_ch: int):
        super().__init__()
        self.up = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True)
        self.conv = ResConvBlock(in_ch, out_ch)


class _Workspace:
    """The activations of one (device, B, H, W): per level the scratch of a block (raw convolution output z, the first
    activation a, the skip s), per block its output and its GroupNorm statistics, the bottleneck's buffers."""

    def __init__(self, f, groups, nmodes, B, H, W, device):
        sizes = _levels(H, W)
        self.sizes = sizes

        def new(*shape, dtype=torch.float32):
            return torch.empty(*shape, dtype=dtype, device=device)

        def rows(lv, c):
            return new(B, sizes[lv][0], sizes[lv][1], c)

        width = [f, 2 * f, 4 * f, 8 * f]
        self.z = [rows(lv, width[lv]) for lv in range(4)]
        self.a = [rows(lv, width[lv]) for lv in range(4)]
        self.s = [rows(lv, width[lv]) for lv in range(4)]
        self.x = [rows(lv, width[lv]) for lv in range(4)]      # x1 .. x4
        self.cat = rows(3, 16 * f)                              # [attention | spectral]
        self.mix = rows(3, 8 * f)
        self.u = [rows(2, 4 * f), rows(1, 2 * f), rows(0, f)]  # up1 .. up3
        self.stats = [[new(B, g) for _ in range(4)] for g in groups]  # per block: mean1, invstd1, mean2, invstd2
        tail = max(hip.unet_v2_tail_ws_bytes(B, sizes[lv][0] * sizes[lv][1], width[lv]) for lv in range(4))
        self.tail = new(tail // 8, dtype=torch.float64)
        Hb, Wb = sizes[3]
        N, C = Hb * Wb, 8 * f
        self.tokens, self.qkv, self.heads_out = new(B, N, C), new(B, N, 3 * C), new(B, N, C)
        self.X, self.O = new(B, nmodes, C, 2), new(B, nmodes, C, 2)


class WeatherUNetV2(_UNetBase):
    """`WeatherUNetV2(in_channels, out_channels, base_filters=64, attn_heads=4, spectral_modes=4)` of
    model_v2.py:153-224, forward in eval mode only: 72 launches (see the module's docstring)."""

    LAUNCHES = 72
    _INFERENCE_ONLY = ("WeatherUNetV2: the HIP path is inference-only (no backward through GroupNorm, the attention or "
                       "the spectral layer); call .eval()")

    def __init__(self, in_channels: int, out_channels: int, base_filters: int = 64, attn_heads: int = 4,
                 spectral_modes: int = 4):
        super().__init__()
        f = int(base_filters)
        if f < 4 or f % 4:
            raise ValueError(f"WeatherUNetV2: base_filters must be a positive multiple of 4, got {base_filters}")
        if in_channels < 1 or out_channels < 1:
            raise ValueError(f"WeatherUNetV2: in_channels {in_channels}, out_channels {out_channels}")
        if attn_heads < 1 or (8 * f) % attn_heads:
            raise ValueError(f"WeatherUNetV2: attn_heads {attn_heads} must divide the bottleneck width {8 * f}")
        if spectral_modes < 1:
            raise ValueError(f"WeatherUNetV2: spectral_modes must be at least 1, got {spectral_modes}")
        self.in_channels, self.out_channels, self.base_filters = int(in_channels), int(out_channels), f
        self.inc = ResConvBlock(in_channels, f)
        self.down1 = Down(f, f * 2)
        self.down2 = Down(f * 2, f * 4)
        self.down3 = Down(f * 4, f * 8)
        self.bottleneck_attn = SelfAttention2D(f * 8, heads=attn_heads)
        self.bottleneck_spectral = SpectralConv2d(f * 8, f * 8, modes_h=spectral_modes, modes_w=spectral_modes)
        self.bottleneck_mix = ResConvBlock(f * 8 * 2, f * 8)
        self.up1 = Up(f * 8 + f * 4, f * 4)
        self.up2 = Up(f * 4 + f * 2, f * 2)
        self.up3 = Up(f * 2 + f, f)
        self.out_conv = nn.Conv2d(f, out_channels, 1)
        self._packed = {}       # conv index -> (stamp, packed weights) of _pack_cached
        self._packed_spec = {}  # (mh, mw) -> (stamp, packed complex weights) of _pack_cached

    def _blocks(self):
        return [self.inc, self.down1.conv, self.down2.conv, self.down3.conv, self.bottleneck_mix, self.up1.conv,
                self.up2.conv, self.up3.conv]

    def _pack_spectral(self, mh, mw):
        sp = self.bottleneck_spectral
        return _pack_cached(self._packed_spec, (mh, mw), (sp.weights_re, sp.weights_im),
                            lambda re, im, out: hip.unet_v2_spectral_pack(re, im, mh, mw, out=out))

    def _ensure_packed(self, modes=None):
        """Packed copies of the 16 convolution weights and of the spectral weights for every mode count in use (and for
        `modes` = (mh, mw)), rebuilt for every weight that changed since its last pack."""
        out = [_pack_cached(self._packed, 2 * i + (j == 3), (blk.conv[j].weight,), hip.unet_pack_weights)
               for i, blk in enumerate(self._blocks()) for j in (0, 3)]
        for m in list(self._packed_spec):
            self._pack_spectral(*m)
        spec = self._pack_spectral(*modes) if modes is not None else None
        return out, spec

    def _workspace(self, B, H, W, device, nmodes):
        groups = [blk.conv[1].num_groups for blk in self._blocks()]
        return self._workspace_for((str(device), B, H, W),
                                   lambda: _Workspace(self.base_filters, groups, nmodes, B, H, W, device))

    def _check_shape(self, x):
        H, W = x.shape[2:]
        if (H // 8) * (W // 8) > MAX_TOKENS:
            raise ValueError(f"WeatherUNetV2: the attention takes at most {MAX_TOKENS} bottleneck pixels, "
                             f"{H} x {W} gives {(H // 8) * (W // 8)}")

    def _block_plan(self, plan, name, k, blk, src, cin, lv, out, packed, ws):
        """The 9 launches of ResConvBlock k reading `src` (cin channels) into `out` at level lv."""
        z, a, s = ws.z[lv], ws.a[lv], ws.s[lv]
        m1, i1, m2, i2 = ws.stats[k]
        gn1, gn2 = blk.conv[1], blk.conv[4]
        C = blk.out_ch
        fc1, fc2 = blk.se.fc[2], blk.se.fc[4]
        S = hip.unet_src
        plan.append((name + ".conv.0", lambda: hip.unet_conv3x3(src, packed[2 * k], None, gn1.eps, z, cin)))
        plan.append((name + ".gn1_stats", lambda: hip.unet_v2_gn_stats(z, gn1.num_groups, gn1.eps, m1, i1)))
        plan.append((name + ".gn1_gelu", lambda: hip.unet_v2_gn_gelu(z, gn1.weight.detach(), gn1.bias.detach(), m1, i1, a)))
        plan.append((name + ".conv.3", lambda: hip.unet_conv3x3(S(hip.UNET_ROWS, a), packed[2 * k + 1], None, gn2.eps, z, C)))
        plan.append((name + ".gn2_stats", lambda: hip.unet_v2_gn_stats(z, gn2.num_groups, gn2.eps, m2, i2)))
        skip_w = blk.skip.weight.detach().view(C, cin) if isinstance(blk.skip, nn.Conv2d) else None
        plan.append((name + ".skip", lambda: hip.unet_v2_conv1x1(src, skip_w, s, cin)))
        plan.append((name + ".tail", lambda: hip.unet_v2_block_tail(
            z, gn2.weight.detach(), gn2.bias.detach(), m2, i2, s, fc1.weight.detach(), fc1.bias.detach(),
            fc2.weight.detach(), fc2.bias.detach(), out=out, ws=ws.tail)))

    def launch_plan(self, x, y, residual_from=None):
        """The entry-point calls of a forward of the contiguous x into y, in order: [(name, callable)]; `.tail` is two
        launches, every other entry one.  (tools/bench_unet_v2.py times them one by one.)"""
        B, _, H, W = x.shape
        f = self.base_filters
        Hb, Wb = H // 8, W // 8
        sp, at = self.bottleneck_spectral, self.bottleneck_attn
        mh, mw = hip.spectral_modes(Hb, Wb, sp.modes_h, sp.modes_w)
        packed, spec = self._ensure_packed((mh, mw))
        ws = self._workspace(B, H, W, x.device, mh * mw)
        S = hip.unet_src
        b = self._blocks()
        x1, x2, x3, x4 = ws.x
        u1, u2, u3 = ws.u
        C = 8 * f
        plan = []
        self._block_plan(plan, "inc", 0, b[0], S(hip.UNET_PLANAR, x), self.in_channels, 0, x1, packed, ws)
        self._block_plan(plan, "down1", 1, b[1], S(hip.UNET_POOL, x1), f, 1, x2, packed, ws)
        self._block_plan(plan, "down2", 2, b[2], S(hip.UNET_POOL, x2), 2 * f, 2, x3, packed, ws)
        self._block_plan(plan, "down3", 3, b[3], S(hip.UNET_POOL, x3), 4 * f, 3, x4, packed, ws)
        # attention: the tokens are x4's pixels; the residual goes on the normalised tokens (model_v2.py:79,91)
        tok = ws.tokens.view(B, Hb, Wb, C)
        plan.append(("attn.norm", lambda: hip.unet_v2_layernorm(x4, at.norm.weight.detach(), at.norm.bias.detach(),
                                                                at.norm.eps, tok)))
        plan.append(("attn.qkv", lambda: hip.unet_v2_conv1x1(S(hip.UNET_ROWS, tok), at.qkv.weight.detach(),
                                                             ws.qkv.view(B, Hb, Wb, 3 * C), C)))
        plan.append(("attn.core", lambda: hip.unet_v2_attention(ws.qkv, at.heads, ws.heads_out)))
        plan.append(("attn.proj", lambda: hip.unet_v2_conv1x1(
            S(hip.UNET_ROWS, ws.heads_out.view(B, Hb, Wb, C)), at.proj.weight.detach(), ws.cat[..., :C], C,
            bias=at.proj.bias.detach(), res=tok)))
        plan.append(("spectral.fwd", lambda: hip.unet_v2_spectral_fwd(x4, mh, mw, ws.X)))
        plan.append(("spectral.mix", lambda: hip.unet_v2_spectral_mix(ws.X, spec, ws.O)))
        plan.append(("spectral.inv", lambda: hip.unet_v2_spectral_inv(ws.O, ws.cat[..., C:], mh, mw)))
        self._block_plan(plan, "bottleneck_mix", 4, b[4], S(hip.UNET_ROWS, ws.cat), 2 * C, 3, ws.mix, packed, ws)
        self._block_plan(plan, "up1", 5, b[5], S(hip.UNET_UPCAT, x3, ws.mix), 12 * f, 2, u1, packed, ws)
        self._block_plan(plan, "up2", 6, b[6], S(hip.UNET_UPCAT, x2, u1), 6 * f, 1, u2, packed, ws)
        self._block_plan(plan, "up3", 7, b[7], S(hip.UNET_UPCAT, x1, u2), 3 * f, 0, u3, packed, ws)
        oc = self.out_conv
        res = x[:, residual_from[0]:residual_from[1]] if residual_from is not None else None
        plan.append(("out_conv", lambda: hip.unet_conv1x1_out(u3, oc.weight.detach().view(self.out_channels, f),
                                                              oc.bias.detach(), y, residual=res, res_bs=x.stride(0))))
        return plan
