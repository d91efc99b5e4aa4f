"""The U-Net downscaler of the reference (`src/unet/model.py::WeatherUNet`) in eval mode on the HIP path.

The module tree, parameter and buffer names are the reference's, so `load_state_dict(torch.load("best_model.pth"))` of a
reference checkpoint works with `strict=True`.  The forward is 15 launches of `csrc/unet.hip`: 14 `gcl_unet_conv3x3`
(3x3 convolution + BatchNorm on the running statistics + erf GELU) and one `gcl_unet_conv1x1_out`.  MaxPool2d, the
bilinear Upsample, the pad to the skip's size and the concatenation are not launches: they are how the next convolution
reads its input.  Activations are channels-last `[B, H, W, C]` float32 tensors of a per-shape workspace the module holds.

`WeatherUNet` is inference-only: its forward refuses training mode.  `TrainableUNet` is the same module tree with a
training forward (BatchNorm on batch statistics, running buffers updated) and a backward on `csrc/unet_train.hip`, one
`torch.autograd.Function` over the 44 parameters: what `downscale_train.fit_downscaler` trains.
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


# The 14 convolutions in forward order: their names, the pooling level they run at (output width f << level), and how
# the ones that do not read the previous activation find their input
_NAMES = ["inc.0", "inc.3", "down1.0", "down1.3", "down2.0", "down2.3", "down3.0", "down3.3", "up1.0", "up1.3", "up2.0",
          "up2.3", "up3.0", "up3.3"]
_LEVEL = [0, 0, 1, 1, 2, 2, 3, 3, 2, 2, 1, 1, 0, 0]
_UPCAT = {8: (5, 7), 10: (3, 9), 12: (1, 11)}  # convolution -> (skip activation, low activation)
_POOL = {2: 1, 4: 3, 6: 5}                      # convolution -> pooled activation
_SKIP_OF = {5: 8, 3: 10, 1: 12}                 # activation -> the UPCAT convolution that also read it


def _levels(H, W):
    sizes = [(H, W)]
    for _ in range(3):
        sizes.append((sizes[-1][0] // 2, sizes[-1][1] // 2))
    return sizes


def _conv_outputs(f, B, H, W, device):
    """One channels-last float32 buffer per convolution output."""
    sizes = _levels(H, W)
    return [torch.empty(B, *sizes[lv], f << lv, dtype=torch.float32, device=device) for lv in _LEVEL]


def _pack_cached(cache, key, weights, pack):
    """cache[key]: pack(*weights, out=...) of the detached contiguous weights, redone when the (data_ptr, _version) of one
    of them changed - into the old buffer while the device stays, because a captured graph may hold it."""
    stamp = tuple((w.data_ptr(), w._version) for w in weights)
    cur = cache.get(key)
    if cur is None or cur[0] != stamp:
        buf = cur[1] if cur is not None and cur[1].device == weights[0].device else None
        cur = cache[key] = (stamp, pack(*(w.detach().contiguous() for w in weights), out=buf))
    return cur[1]


class _UNetBase(nn.Module):
    """What `WeatherUNet` and `unet_v2.WeatherUNetV2` share: the input checks, the per-shape workspaces and the
    inference forward over `launch_plan`.  A subclass sets in_channels / out_channels, `_INFERENCE_ONLY` (its refusal of
    training mode) and `launch_plan(x, y, residual_from)`."""

    _INFERENCE_ONLY = ""

    def __init__(self):
        super().__init__()
        self._ws = {}  # (what, device, B, H, W) -> the buffers of that shape

    @property
    def num_params(self):
        return sum(p.numel() for p in self.parameters() if p.requires_grad)

    def _workspace_for(self, key, make):
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = make()
        return ws

    def _check_shape(self, x):
        """A subclass's own conditions on the [B, in_channels, H, W] input (ValueError)."""

    def _check_input(self, x, residual_from=None):
        who = type(self).__name__
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise ValueError(f"{who}: input [B, {self.in_channels}, H, W] expected, got {tuple(x.shape)}")
        B, _, H, W = x.shape
        if H < MIN_GRID or W < MIN_GRID:
            raise ValueError(f"{who}: the grid must be at least {MIN_GRID} x {MIN_GRID} (three poolings), got {H} x {W}")
        self._check_shape(x)
        if B < 1:
            raise ValueError(f"{who}: empty batch")
        if residual_from is not None:
            c0, c1 = residual_from
            if not (0 <= c0 < c1 <= self.in_channels and c1 - c0 == self.out_channels):
                raise ValueError(f"{who}: residual_from {residual_from} is not a slice of {self.out_channels} of the "
                                 f"{self.in_channels} input channels")
        if x.dtype != torch.float32:
            raise RuntimeError(f"{who} needs float32 tensors, got {x.dtype} (there is no CPU fallback)")
        if not x.is_cuda:
            raise RuntimeError(f"{who} needs GPU tensors (there is no CPU fallback)")

    def forward(self, x, residual_from=None):
        """x float32 [B, in_channels, H, W] on the GPU -> [B, out_channels, H, W].  residual_from = (c0, c1): the channel
        slice x[:, c0:c1] is added to the output in the last launch (the x_last of predict_cascade.py:357-359 and
        predict_v2.py:137-139)."""
        if self.training:
            raise NotImplementedError(self._INFERENCE_ONLY)
        self._check_input(x, residual_from)
        with torch.no_grad():
            x = x.detach().contiguous()
            y = torch.empty(x.shape[0], self.out_channels, *x.shape[2:], dtype=torch.float32, device=x.device)
            for _, launch in self.launch_plan(x, y, residual_from):
                launch()
        return y


class WeatherUNet(_UNetBase):
    """`WeatherUNet(in_channels, out_channels, base_filters=64)` of model.py:59-102, forward in eval mode only."""

    _INFERENCE_ONLY = ("WeatherUNet: the HIP path is inference-only (no backward, no BatchNorm in training mode); call "
                       ".eval(), and train with the reference's torch module through downscale.fit_downscaler")

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
        self._packed = {}  # conv index -> (stamp, packed weights) of _pack_cached

    def _conv_list(self):
        return [cb for blk in (self.inc, self.down1, self.down2, self.down3, self.up1, self.up2, self.up3)
                for cb in blk.convs()]

    def _ensure_packed(self):
        """Packed copies of the 14 convolution weights, rebuilt for every weight that changed since its last pack."""
        return [_pack_cached(self._packed, i, (conv.weight,), hip.unet_pack_weights)
                for i, (conv, _) in enumerate(self._conv_list())]

    def _activations(self, B, H, W, device):
        return self._workspace_for(("acts", str(device), B, H, W),
                                   lambda: _conv_outputs(self.base_filters, B, H, W, device))

    def _sources(self, x, a):
        """[(name, source, Cin)] of the 14 convolutions reading the planar x and the activations a."""
        S = hip.unet_src
        out = []
        for i, name in enumerate(_NAMES):
            if i == 0:
                src, cin = S(hip.UNET_PLANAR, x), x.shape[1]
            elif i in _UPCAT:
                skip, low = a[_UPCAT[i][0]], a[_UPCAT[i][1]]
                src, cin = S(hip.UNET_UPCAT, skip, low), skip.shape[3] + low.shape[3]
            else:
                t = a[_POOL.get(i, i - 1)]
                src, cin = S(hip.UNET_POOL if i in _POOL else hip.UNET_ROWS, t), t.shape[3]
            out.append((name, src, cin))
        return out

    def launch_plan(self, x, y, residual_from=None):
        """The 15 launches of a forward of the contiguous x into y, in order: [(name, callable)].  (tools/bench_unet.py
        times them one by one.)"""
        B, _, H, W = x.shape
        packed = self._ensure_packed()
        a = self._activations(B, H, W, x.device)
        convs = self._conv_list()
        f = self.base_filters
        plan = []
        for i, (name, src, cin) in enumerate(self._sources(x, a)):
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


class _TrainWorkspace:
    """What one training step of one shape keeps between forward and backward: per convolution the raw output z, the
    activation a, the batch mean and invstd and the gradient buffer dA (dZ overwrites it); per pooled or concatenated
    convolution the data gradient at the convolution's own input size.  `step` counts the forwards that wrote it."""

    def __init__(self, f, B, H, W, device):
        self.z, self.a, self.dA = (_conv_outputs(f, B, H, W, device) for _ in range(3))
        self.mean = [torch.empty(f << lv, dtype=torch.float32, device=device) for lv in _LEVEL]
        self.invstd = [torch.empty(f << lv, dtype=torch.float32, device=device) for lv in _LEVEL]
        # the data gradients that are not a dA: POOL layers 2, 4, 6 (at the pooled size), UPCAT layers 8, 10, 12; each has
        # its convolution's output size and the channels of the activations the convolution read
        self.dX = {i: torch.empty(*self.a[i].shape[:3], sum(self.a[k].shape[3] for k in reads), dtype=torch.float32,
                                  device=device)
                   for i, reads in [(i, (k,)) for i, k in _POOL.items()] + list(_UPCAT.items())}
        self.step = 0


class _UNetTrainStep(torch.autograd.Function):
    """The training forward and the backward of `TrainableUNet` as one node over its parameters."""

    @staticmethod
    def forward(ctx, model, x, *params):
        B, _, H, W = x.shape
        ws = model._train_workspace(B, H, W, x.device)
        y = torch.empty(B, model.out_channels, H, W, dtype=torch.float32, device=x.device)
        for _, launch in model.train_launch_plan(x, y, ws):
            launch()
        ws.step += 1
        ctx.model, ctx.ws, ctx.step, ctx.x = model, ws, ws.step, x
        return y

    @staticmethod
    def backward(ctx, g):
        model, ws = ctx.model, ctx.ws
        if ws.step != ctx.step:
            raise RuntimeError("TrainableUNet: another training forward of the same shape has run since this one; its "
                               "saved activations are gone (run backward before the next forward)")
        params = list(model.parameters())
        need = {id(p): ctx.needs_input_grad[2 + k] for k, p in enumerate(params)}
        grads = {}
        for _, launch in model.backward_launch_plan(ctx.x, g.to(torch.float32).contiguous(), ws, need, grads):
            launch()
        return (None, None) + tuple(grads.get(id(p)) if need[id(p)] else None for p in params)


class TrainableUNet(WeatherUNet):
    """`WeatherUNet` that also trains on the HIP path.  Same module tree, names, state dict and `num_params`.

    Eval mode: the parent's forward, bit for bit.  Training mode: `forward(x)` is the forward of model.py:87-98 with
    BatchNorm on the batch statistics (running_mean, running_var and num_batches_tracked updated as nn.BatchNorm2d does)
    and returns y with a grad_fn; `y.backward(g)` leaves `.grad` on the 14 convolution weights, the 28 BatchNorm affine
    vectors and out_conv's weight and bias.  There is no gradient with respect to x.  Per convolution the forward is
    three entry points (`gcl_unet_conv3x3` with gamma NULL, `gcl_unet_bn_stats`, `gcl_unet_bn_gelu`) and the backward
    `gcl_unet_bn_gelu_bwd`, `gcl_unet_conv3x3_wgrad` and, as the data gradient, `gcl_unet_conv3x3` on the transposed
    tap-flipped weight, routed through `gcl_unet_pool_bwd` / `gcl_unet_upsample_bwd` where the input was pooled or
    upsampled.  A backward must run before the next training forward of the same shape.  The module keeps the training
    workspace of the most recent input shape only; `release_workspaces()` drops it."""

    def __init__(self, in_channels: int, out_channels: int, base_filters: int = 64):
        super().__init__(in_channels, out_channels, base_filters)
        self._packed_dgrad = {}  # conv index -> (stamp, transposed tap-flipped pack) of _pack_cached

    def _ensure_packed_dgrad(self):
        """The data-gradient packs of convolutions 1 .. 13, rebuilt for every weight that changed since its last pack."""
        return {i: _pack_cached(self._packed_dgrad, i, (conv.weight,), hip.unet_pack_weights_dgrad)
                for i, (conv, _) in enumerate(self._conv_list()) if i}

    def _train_workspace(self, B, H, W, device):
        key = ("train", str(device), B, H, W)
        if key not in self._ws:
            # one shape at a time (about 0.55 GB at 41 x 61, f = 64, B = 32): a new shape replaces the old one, whose
            # memory is freed once no pending backward holds it
            self._ws = {k: v for k, v in self._ws.items() if k[0] != "train"}
        return self._workspace_for(key, lambda: _TrainWorkspace(self.base_filters, B, H, W, device))

    def release_workspaces(self):
        """Drop the training workspace and the inference activations (they are rebuilt on the next forward)."""
        self._ws = {}

    def _check_shape(self, x):
        if not self.training:
            return
        B, _, H, W = x.shape
        if B * (H // 8) * (W // 8) < 2:
            raise ValueError(f"TrainableUNet: expected more than 1 value per channel when training, got "
                             f"{B} x {H // 8} x {W // 8} at the deepest level")
        if x.requires_grad:
            raise ValueError("TrainableUNet: an input that requires grad is not supported (there is no gradient with "
                             "respect to x)")

    def forward(self, x, residual_from=None):
        """Eval mode: `WeatherUNet.forward`.  Training mode: x float32 [B, in_channels, H, W] on the GPU (not requiring
        grad) -> y [B, out_channels, H, W] with a grad_fn; residual_from is refused (the loss adds x_last itself:
        `downscaler_loss(..., X=X, residual=True)`)."""
        if not self.training:
            return super().forward(x, residual_from)
        if residual_from is not None:
            raise ValueError("TrainableUNet: residual_from is an inference option; in training the loss adds x_last "
                             "(downscaler_loss(..., X=X, residual=True))")
        self._check_input(x)
        for _, bn in self._conv_list():
            if bn.momentum is None or not bn.track_running_stats:
                raise ValueError("TrainableUNet: BatchNorm2d with a momentum and running statistics expected")
        return _UNetTrainStep.apply(self, x.detach().contiguous(), *self.parameters())

    def train_launch_plan(self, x, y, ws):
        """The entry-point calls of a training forward of the contiguous x into y, in order: [(name, callable)]."""
        packed = self._ensure_packed()
        convs = self._conv_list()
        plan = []
        for i, (name, src, cin) in enumerate(self._sources(x, ws.a)):
            bn = convs[i][1]
            plan.append((name, lambda src=src, i=i, eps=bn.eps, cin=cin: hip.unet_conv3x3(src, packed[i], None, eps, ws.z[i], cin)))
            plan.append((name + ".bn_stats", lambda i=i, bn=bn: hip.unet_bn_stats(
                ws.z[i], bn.eps, bn.momentum, ws.mean[i], ws.invstd[i], bn.running_mean, bn.running_var,
                bn.num_batches_tracked)))
            plan.append((name + ".bn_gelu", lambda i=i, bn=bn: hip.unet_bn_gelu(
                ws.z[i], bn.weight.detach(), bn.bias.detach(), ws.mean[i], ws.invstd[i], ws.a[i])))
        oc, f = self.out_conv, self.base_filters
        plan.append(("out_conv", lambda: hip.unet_conv1x1_out(ws.a[13], oc.weight.detach().view(self.out_channels, f),
                                                              oc.bias.detach(), y)))
        return plan

    def backward_launch_plan(self, x, g, ws, need=None, grads=None):
        """The entry-point calls of the backward of the last training forward on `ws`, given the planar g = d loss / d y,
        in order: [(name, callable)].  grads (a dict) receives id(parameter) -> gradient, fresh tensors; need: id ->
        bool (None: every parameter); only a convolution weight that needs none saves work (its wgrad)."""
        grads = {} if grads is None else grads
        wanted = (lambda p: True) if need is None else (lambda p: need[id(p)])
        convs, f, dev = self._conv_list(), self.base_filters, x.device
        packed_t = self._ensure_packed_dgrad()
        sources = self._sources(x, ws.a)
        oc = self.out_conv
        plan = []

        def new(*shape):
            return torch.empty(*shape, dtype=torch.float32, device=dev)

        def out_bwd():
            dW, db = new(self.out_channels, f, 1, 1), new(self.out_channels)
            hip.unet_conv1x1_out_bwd(g, ws.a[13], oc.weight.detach().view(self.out_channels, f), ws.dA[13], dW, db)
            grads[id(oc.weight)], grads[id(oc.bias)] = dW, db

        plan.append(("out_conv.bwd", out_bwd))
        for i in range(13, -1, -1):
            name, src, cin = sources[i]
            conv, bn = convs[i]

            def bn_bwd(i=i, bn=bn):
                dg, db = new(bn.num_features), new(bn.num_features)
                hip.unet_bn_gelu_bwd(ws.z[i], ws.dA[i], bn.weight.detach(), bn.bias.detach(), ws.mean[i], ws.invstd[i],
                                     ws.dA[i], dg, db)
                grads[id(bn.weight)], grads[id(bn.bias)] = dg, db

            plan.append((name + ".bn_gelu_bwd", bn_bwd))
            if wanted(conv.weight):
                def wgrad(i=i, src=src, conv=conv, cin=cin):
                    grads[id(conv.weight)] = hip.unet_conv3x3_wgrad(src, ws.dA[i], cin)

                plan.append((name + ".wgrad", wgrad))
            if i == 0:
                break
            target = ws.dX[i] if i in ws.dX else ws.dA[i - 1]
            plan.append((name + ".dgrad", lambda i=i, target=target, eps=bn.eps: hip.unet_conv3x3(
                hip.unet_src(hip.UNET_ROWS, ws.dA[i]), packed_t[i], None, eps, target, ws.dA[i].shape[3])))
            if i in _UPCAT:
                skip, low = _UPCAT[i]
                plan.append((name + ".upsample_bwd", lambda i=i, skip=skip, low=low: hip.unet_upsample_bwd(
                    ws.dX[i], ws.a[skip].shape[3], ws.dA[low])))
            elif i in _POOL:
                act = _POOL[i]
                up = _SKIP_OF[act]
                plan.append((name + ".pool_bwd", lambda i=i, act=act, up=up: hip.unet_pool_bwd(
                    ws.a[act], ws.dX[i], ws.dA[act], skip=ws.dX[up][..., :ws.a[act].shape[3]])))
        return plan


class CapturedUNet(Captured):
    """`model(x, residual_from=...)` replayed from a hipGraph (capture.Captured): the bits of the eager forward.  The
    packed weights are refreshed before a replay when a weight has changed; the graph keeps pointing at them.  `model`: a
    `WeatherUNet` or a `unet_v2.WeatherUNetV2`."""

    def __init__(self, model: nn.Module, use_graph=None, residual_from=None, required: bool = False):
        super().__init__(use_graph=graph_enabled(use_graph), required=required)
        self.model, self.residual_from = model, residual_from

    def _work(self, x):
        return self.model(x, residual_from=self.residual_from)

    def __call__(self, x):
        if x.is_cuda and not self.model.training:
            self.model._ensure_packed()
        return self._run(x)
