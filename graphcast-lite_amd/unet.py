"""The U-Net downscaler of the reference (`src/unet/model.py::WeatherUNet`) in eval mode on the HIP path.

The module tree, parameter and buffer names are the reference's, so `load_state_dict(torch.load("best_model.pth"))` of a
reference checkpoint works with `strict=True`.  The forward is 15 launches of `csrc/unet.hip`: 14 `gcl_unet_conv3x3`
(3x3 convolution + BatchNorm on the running statistics + erf GELU) and one `gcl_unet_conv1x1_out`.  MaxPool2d, the
bilinear Upsample, the pad to the skip's size and the concatenation are not launches: they are how the next convolution
reads its input.  Activations are channels-last `[B, H, W, C]` float32 tensors of a per-shape workspace the module holds.

The HIP path is inference-only: there is no backward and no BatchNorm in training mode.  Training runs the reference's
torch module through `downscale.fit_downscaler`.
"""
import torch
import torch.nn as nn

from . import hip
from .capture import Captured, graph_enabled

MIN_GRID = 8  # three poolings: below 8 the third has nothing left


class _Part(nn.Module):
    def forward(self, *args, **kw):
        raise NotImplementedError(f"{type(self).__name__} holds parameters only: it runs as part of WeatherUNet.forward")


class DoubleConv(_Part):
    """Conv3x3 -> BN -> GELU -> Conv3x3 -> BN -> GELU (model.py:11-25)."""

    def __init__(self, in_ch: int, out_ch: int):
        super().__init__()
        self.net = nn.Sequential(
            nn.Conv2d(in_ch, out_ch, 3, padding=1, bias=False), nn.BatchNorm2d(out_ch), nn.GELU(),
            nn.Conv2d(out_ch, out_ch, 3, padding=1, bias=False), nn.BatchNorm2d(out_ch), nn.GELU())

    def convs(self):
        return [(self.net[0], self.net[1]), (self.net[3], self.net[4])]


class Down(_Part):
    """MaxPool -> DoubleConv (model.py:28-38)."""

    def __init__(self, in_ch: int, out_ch: int):
        super().__init__()
        self.net = nn.Sequential(nn.MaxPool2d(2), DoubleConv(in_ch, out_ch))

    def convs(self):
        return self.net[1].convs()


class Up(_Part):
    """Upsample -> cat skip -> DoubleConv (model.py:41-56)."""

    def __init__(self, in_ch: int, out_ch: int):
        super().__init__()
        self.up = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True)
        self.conv = DoubleConv(in_ch, out_ch)

    def convs(self):
        return self.conv.convs()


class WeatherUNet(nn.Module):
    """`WeatherUNet(in_channels, out_channels, base_filters=64)` of model.py:59-102, forward in eval mode only."""

    def __init__(self, in_channels: int, out_channels: int, base_filters: int = 64):
        super().__init__()
        f = int(base_filters)
        if f < 4 or f % 4:
            raise ValueError(f"WeatherUNet: base_filters must be a positive multiple of 4, got {base_filters}")
        if in_channels < 1 or out_channels < 1:
            raise ValueError(f"WeatherUNet: in_channels {in_channels}, out_channels {out_channels}")
        self.in_channels, self.out_channels, self.base_filters = int(in_channels), int(out_channels), f
        self.inc = DoubleConv(in_channels, f)
        self.down1 = Down(f, f * 2)
        self.down2 = Down(f * 2, f * 4)
        self.down3 = Down(f * 4, f * 8)
        self.up1 = Up(f * 8 + f * 4, f * 4)
        self.up2 = Up(f * 4 + f * 2, f * 2)
        self.up3 = Up(f * 2 + f, f)
        self.out_conv = nn.Conv2d(f, out_channels, 1)
        self._packed = {}  # conv index -> (data_ptr, _version, packed weights)
        self._acts = {}    # (device, B, H, W) -> the activations of the 14 convolutions

    @property
    def num_params(self):
        return sum(p.numel() for p in self.parameters() if p.requires_grad)

    def _conv_list(self):
        return [cb for blk in (self.inc, self.down1, self.down2, self.down3, self.up1, self.up2, self.up3)
                for cb in blk.convs()]

    def _ensure_packed(self):
        """Packed copies of the 14 convolution weights, rebuilt for every weight that changed since its last pack."""
        out = []
        for i, (conv, _) in enumerate(self._conv_list()):
            w = conv.weight
            key = (w.data_ptr(), w._version)
            cur = self._packed.get(i)
            if cur is None or cur[0] != key:
                buf = cur[1] if cur is not None and cur[1].device == w.device else None  # same place: a graph may hold it
                cur = (key, hip.unet_pack_weights(w.detach().contiguous(), out=buf))
                self._packed[i] = cur
            out.append(cur[1])
        return out

    def _activations(self, B, H, W, device):
        key = (str(device), B, H, W)
        acts = self._acts.get(key)
        if acts is None:
            f = self.base_filters
            sizes = [(H, W)]
            for _ in range(3):
                sizes.append((sizes[-1][0] // 2, sizes[-1][1] // 2))
            plan = [(0, f), (0, f), (1, 2 * f), (1, 2 * f), (2, 4 * f), (2, 4 * f), (3, 8 * f), (3, 8 * f),
                    (2, 4 * f), (2, 4 * f), (1, 2 * f), (1, 2 * f), (0, f), (0, f)]
            acts = [torch.empty(B, sizes[lv][0], sizes[lv][1], c, dtype=torch.float32, device=device) for lv, c in plan]
            self._acts[key] = acts
        return acts

    def forward(self, x, residual_from=None):
        """x float32 [B, in_channels, H, W] on the GPU -> [B, out_channels, H, W].  residual_from = (c0, c1): the channel
        slice x[:, c0:c1] is added to the output in the last launch (the x_last of predict_cascade.py:357-359)."""
        if self.training:
            raise NotImplementedError(
                "WeatherUNet: the HIP path is inference-only (no backward, no BatchNorm in training mode); call .eval(), "
                "and train with the reference's torch module through downscale.fit_downscaler")
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise ValueError(f"WeatherUNet: input [B, {self.in_channels}, H, W] expected, got {tuple(x.shape)}")
        B, _, H, W = x.shape
        if H < MIN_GRID or W < MIN_GRID:
            raise ValueError(f"WeatherUNet: the grid must be at least {MIN_GRID} x {MIN_GRID} (three poolings), got {H} x {W}")
        if B < 1:
            raise ValueError("WeatherUNet: empty batch")
        if residual_from is not None:
            c0, c1 = residual_from
            if not (0 <= c0 < c1 <= self.in_channels and c1 - c0 == self.out_channels):
                raise ValueError(f"WeatherUNet: residual_from {residual_from} is not a slice of {self.out_channels} of the "
                                 f"{self.in_channels} input channels")
        if x.dtype != torch.float32:
            raise RuntimeError(f"WeatherUNet needs float32 tensors, got {x.dtype} (there is no CPU fallback)")
        if not x.is_cuda:
            raise RuntimeError("WeatherUNet needs GPU tensors (there is no CPU fallback)")
        with torch.no_grad():
            x = x.detach().contiguous()
            y = torch.empty(B, self.out_channels, H, W, dtype=torch.float32, device=x.device)
            for _, launch in self.launch_plan(x, y, residual_from):
                launch()
        return y

    def launch_plan(self, x, y, residual_from=None):
        """The 15 launches of a forward of the contiguous x into y, in order: [(name, callable)].  (tools/bench_unet.py
        times them one by one.)"""
        B, _, H, W = x.shape
        packed = self._ensure_packed()
        a = self._activations(B, H, W, x.device)
        convs = self._conv_list()
        S, f = hip.unet_src, self.base_filters
        sources = [("inc.0", S(hip.UNET_PLANAR, x), self.in_channels), ("inc.3", S(hip.UNET_ROWS, a[0]), f),
                   ("down1.0", S(hip.UNET_POOL, a[1]), f), ("down1.3", S(hip.UNET_ROWS, a[2]), 2 * f),
                   ("down2.0", S(hip.UNET_POOL, a[3]), 2 * f), ("down2.3", S(hip.UNET_ROWS, a[4]), 4 * f),
                   ("down3.0", S(hip.UNET_POOL, a[5]), 4 * f), ("down3.3", S(hip.UNET_ROWS, a[6]), 8 * f),
                   ("up1.0", S(hip.UNET_UPCAT, a[5], a[7]), 12 * f), ("up1.3", S(hip.UNET_ROWS, a[8]), 4 * f),
                   ("up2.0", S(hip.UNET_UPCAT, a[3], a[9]), 6 * f), ("up2.3", S(hip.UNET_ROWS, a[10]), 2 * f),
                   ("up3.0", S(hip.UNET_UPCAT, a[1], a[11]), 3 * f), ("up3.3", S(hip.UNET_ROWS, a[12]), f)]
        plan = []
        for i, (name, src, cin) in enumerate(sources):
            bn = convs[i][1]
            norm = (bn.weight, bn.bias, bn.running_mean, bn.running_var)  # read at the call: no folded copy to go stale
            plan.append((name, lambda src=src, i=i, norm=norm, eps=bn.eps, cin=cin: hip.unet_conv3x3(
                src, packed[i], norm, eps, a[i], cin)))
        oc = self.out_conv
        # the residual is a channel slice of the contiguous planar input: sample stride in_channels * H * W
        res = x[:, residual_from[0]:residual_from[1]] if residual_from is not None else None
        plan.append(("out_conv", lambda: hip.unet_conv1x1_out(a[13], oc.weight.view(self.out_channels, f), oc.bias, y,
                                                              residual=res, res_bs=x.stride(0))))
        return plan


class CapturedUNet(Captured):
    """`model(x, residual_from=...)` replayed from a hipGraph (capture.Captured): the bits of the eager forward.  The
    packed weights are refreshed before a replay when a weight has changed; the graph keeps pointing at them."""

    def __init__(self, model: WeatherUNet, use_graph=None, residual_from=None, required: bool = False):
        super().__init__(use_graph=graph_enabled(use_graph), required=required)
        self.model, self.residual_from = model, residual_from

    def _work(self, x):
        return self.model(x, residual_from=self.residual_from)

    def __call__(self, x):
        if x.is_cuda and not self.model.training:
            self.model._ensure_packed()
        return self._run(x)
