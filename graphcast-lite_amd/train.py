"""Training-step semantics of the reference's `src/train.py`, on the HIP path.

`weighted_mse_loss`, `get_lat_weights`, `build_boundary_mask`, `update_attention_threshold` and
`train_epoch` keep the reference's names, arguments and results (src/train.py:53-136,138-239).
`TrainStep` is the data-parallel fast path used by `bench.py`: one flat parameter / gradient /
Adam-state buffer, gradients accumulated in place by the backward kernels, ONE RCCL all-reduce of
the flat gradient bucket per optimiser step, one grouped Adam update (per-parameter lr, active
flag and step on the device).  `build_optimizer` and `train` restate the reference's fine-tuning optimiser and
training driver (src/main.py:190-211, src/train.py:311-524) on `TrainStep`.  `Evaluator` is `test` as one captured
step per batch (csrc/eval_step.hip), with its scores kept on the device until the end of a pass.
"""
import os

import torch
import torch.distributed as dist

from . import hip
from .capture import Captured, graph_enabled
from .functional import ARStepLossFn, WeightedMSEFn, const_one


class FileNames:
    """File names of an experiment directory (src/constants.py:5-15)."""

    EXPERIMENT_CONFIG = "config.json"
    TRAIN_X = "X_train.pt"
    TRAIN_Y = "y_train.pt"
    TEST_X = "X_test.pt"
    TEST_Y = "y_test.pt"
    SAVED_MODEL = "best_model.pth"
    SAVED_RESULTS = "results.json"
    CHECKPOINT = "checkpoint.pth"


def save_checkpoint(path, model, optimiser, epoch, ar_steps, best_val_loss, patience_counter, train_losses,
                    val_losses):
    """Same dictionary layout as the reference (src/train.py:22-34), so either side can resume the
    other's `checkpoint.pth`; `best_model.pth` is a bare `model.state_dict()` (src/train.py:496)."""
    torch.save({
        "epoch": epoch,
        "ar_steps": ar_steps,
        "best_val_loss": best_val_loss,
        "patience_counter": patience_counter,
        "train_losses": train_losses,
        "val_losses": val_losses,
        "model_state_dict": model.state_dict(),
        "optimizer_state_dict": optimiser.state_dict(),
    }, path)


def load_checkpoint(path, model, optimiser, device):
    """src/train.py:37-49.  `weights_only=True`: nothing from the file is executed."""
    ckpt = torch.load(path, map_location=device, weights_only=True)
    model.load_state_dict(ckpt["model_state_dict"])
    optimiser.load_state_dict(ckpt["optimizer_state_dict"])
    return {
        "start_epoch": ckpt["epoch"] + 1,
        "ar_steps": ckpt["ar_steps"],
        "best_val_loss": ckpt["best_val_loss"],
        "patience_counter": ckpt["patience_counter"],
        "train_losses": ckpt["train_losses"],
        "val_losses": ckpt["val_losses"],
    }


def get_lat_weights(lat_dim, lon_dim, device, flat_lats=None):
    """cos(lat)/mean laid out as the reference lays it out (src/train.py:53-72), `[1, G, 1]`."""
    if flat_lats is not None:
        w = torch.cos(torch.deg2rad(torch.from_numpy(flat_lats.copy()).float()))
        w = w / w.mean()
        return w.view(1, -1, 1).to(device)
    w = torch.cos(torch.deg2rad(torch.linspace(-90, 90, lat_dim)))
    w = w / w.mean()
    return w.view(1, -1).expand(lon_dim, lat_dim).reshape(-1).view(1, -1, 1).to(device)


def build_boundary_mask(n_lon, n_lat, width, device):
    """src/train.py:74-82."""
    m = torch.zeros(n_lon, n_lat)
    m[width:n_lon - width, width:n_lat - width] = 1.0
    return m.reshape(1, -1, 1).to(device)


def combine_spatial_masks(*masks):
    out = None
    for m in masks:
        if m is not None:
            out = m if out is None else out * m
    return out


_lw_cache = {}


def _loss_weights(G: int, C: int, lat_weights, channel_mask, spatial_mask, device):
    """Per-node and per-channel factors of the reference's broadcast weight tensor and sum(w) for
    ONE sample (the caller multiplies by the batch size).  Cached per mask set: building it needs a
    host read-back, which must not happen every step (nor inside a hipGraph capture)."""
    key = (G, C, str(device)) + tuple((id(t), t._version) if t is not None else None
                                      for t in (lat_weights, channel_mask, spatial_mask))
    hit = _lw_cache.get(key)
    if hit is not None:
        return hit[0]
    node_w = None
    for t in (spatial_mask, lat_weights):
        if t is not None:
            t = t.reshape(-1).to(device=device, dtype=torch.float32)
            node_w = t if node_w is None else node_w * t
    chan_w = channel_mask.reshape(-1).to(device=device, dtype=torch.float32) if channel_mask is not None else None
    s_node = node_w.double().sum().item() if node_w is not None else float(G)
    s_chan = chan_w.double().sum().item() if chan_w is not None else float(C)
    out = (node_w.contiguous() if node_w is not None else None,
           chan_w.contiguous() if chan_w is not None else None, s_node * s_chan)
    if len(_lw_cache) > 64:
        _lw_cache.clear()
    _lw_cache[key] = (out, lat_weights, channel_mask, spatial_mask)  # keep the keys' tensors alive
    return out


def weighted_mse_loss(pred, target, lat_weights=None, channel_mask=None, spatial_mask=None, x_last=None):
    """src/train.py:85-102 as one kernel: sum(w (pred-target)^2) / max(sum(w), 1e-12).
    `x_last` (extension) folds the residual add `pred = x_last + delta` into the same pass."""
    if pred.dim() == 2:
        pred, target = pred.unsqueeze(0), target.unsqueeze(0)
    B, G, C = pred.shape
    node_w, chan_w, wsum1 = _loss_weights(G, C, lat_weights, channel_mask, spatial_mask, pred.device)
    inv = 1.0 / max(wsum1 * B, 1e-12)
    return WeightedMSEFn.apply(pred, x_last, target, node_w, chan_w, inv)


def update_attention_threshold(epoch, max_epochs=30, start_epoch=5, final_threshold=0.1356):
    """src/train.py:132-136."""
    if epoch < start_epoch:
        return 0.0
    if epoch > max_epochs + start_epoch:
        return final_threshold
    return min(final_threshold, (epoch - start_epoch) * final_threshold / (max_epochs - start_epoch))


_kind_cache = {}


def _channel_kinds(C, static_channels, forcing_channels, device):
    """Device int32 [C] (0 predicted, 1 static, 2 forcing), cached: uploading it needs a host -> device copy that
    must not happen on every step (nor inside a hipGraph capture)."""
    from .predict import channel_kinds

    key = (C, tuple(static_channels or ()), tuple(forcing_channels or ()), str(device))
    k = _kind_cache.get(key)
    if k is None:
        k = _kind_cache[key] = channel_kinds(C, static_channels, forcing_channels, device)
    return k


def batch_loss(model, X, y, threshold=0.0, epoch=0, batch_num=1, lat_weights=None, current_ar_steps=1,
               channel_mask=None, spatial_mask=None, static_channels=None, forcing_channels=None,
               use_residual=True):
    """Loss of one batch as the reference's inner loop builds it (src/train.py:173-231): per AR step the model
    predicts a delta, the (residual) prediction is scored against that step's target, static / forcing channels are
    overwritten and the window shifts; the step losses are averaged.  Each step is one `ARStepLossFn` (loss + window
    advance fused, 1/steps folded into the loss normaliser, the running sum kept on the device)."""
    N, G, _ = X.shape
    obs = model.obs_window
    C = X.shape[-1] // obs
    steps_total = y.shape[-1] // C
    y_steps = y.view(N, G, steps_total, C)
    state = X.view(N, G, obs, C)
    steps = min(current_ar_steps, steps_total)
    node_w, chan_w, wsum1 = _loss_weights(G, C, lat_weights, channel_mask, spatial_mask, X.device)
    inv = 1.0 / (max(wsum1 * N, 1e-12) * steps)
    kinds = _channel_kinds(C, static_channels, forcing_channels, X.device) if steps > 1 else None
    loss = None
    for s in range(steps):
        delta = model(X=state.reshape(N, G, -1), attention_threshold=threshold, epoch=epoch, batch_num=batch_num)
        if delta.dim() == 2:
            delta = delta.unsqueeze(0)
        loss, state = ARStepLossFn.apply(state, delta, y_steps[:, :, s, :], loss, node_w, chan_w, inv, kinds,
                                         bool(use_residual), s + 1 < steps)
    return loss


def train_epoch(model, train_dataloader, optimiser, loss_fn, device, threshold, epoch, lat_weights=None,
                current_ar_steps=1, channel_mask=None, spatial_mask=None, static_channels=None,
                forcing_channels=None, use_residual=True):
    """src/train.py:138-239 (same signature; `loss_fn` is unused there as well)."""
    model.train()
    total = 0.0
    for i, (X, y) in enumerate(train_dataloader):
        y = y.squeeze(0) if y.dim() == 4 else y
        X, y = X.to(device), y.to(device)
        optimiser.zero_grad()
        loss = batch_loss(model, X, y, threshold, epoch, i, lat_weights, current_ar_steps, channel_mask,
                          spatial_mask, static_channels, forcing_channels, use_residual)
        loss.backward()
        optimiser.step()
        total += loss.detach().item()
    return total / max(len(train_dataloader), 1)


def spatial_corr(pred: torch.Tensor, true: torch.Tensor, exclude_channels=None) -> float:
    """Spatial anomaly correlation (src/train.py:114-130): per feature, the mean over nodes of the
    product of the standardised fields (std unbiased, + 1e-8); per sample, then averaged."""
    if pred.dim() == 3:
        accs = [spatial_corr(pred[b], true[b], exclude_channels) for b in range(pred.shape[0])]
        return sum(accs) / max(len(accs), 1)
    p = (pred - pred.mean(dim=0, keepdim=True)) / (pred.std(dim=0, keepdim=True) + 1e-8)
    t = (true - true.mean(dim=0, keepdim=True)) / (true.std(dim=0, keepdim=True) + 1e-8)
    acc = (p * t).mean(dim=0)
    if exclude_channels:
        keep = [i for i in range(acc.shape[0]) if i not in exclude_channels]
        if keep:
            return acc[keep].mean().item()
    return acc.mean().item()


def test(model, test_dataloader, loss_fn, device, lat_weights=None, spatial_mask=None, channel_mask=None,
         static_channels=None, forcing_channels=None, use_residual=True):
    """One-step evaluation, same signature and return value as the reference's `test` (src/train.py:241-308):
    (mean weighted MSE, mean spatial ACC, RMSE of the unweighted errors).  The prediction step with its
    static / forcing carry-forward is the device-side rollout of `predict.py` (one step)."""
    from .predict import rollout

    model.eval()
    total, accs, raw = 0.0, [], []
    with torch.no_grad():
        for X, y in test_dataloader:
            y = y.squeeze(0) if y.dim() == 4 else y
            X, y = X.to(device), y.to(device)
            C = X.shape[-1] // model.obs_window
            steps = y.shape[-1] // C if C > 0 else 1
            y0 = y.view(y.shape[0], y.shape[1], steps, C)[:, :, 0, :].contiguous() if steps > 1 else y
            outs = rollout(model, X, 1, y=y0, static_channels=static_channels, forcing_channels=forcing_channels,
                           use_residual=use_residual)
            total += weighted_mse_loss(outs, y0, lat_weights, channel_mask, spatial_mask).item()
            raw.append(((outs - y0) ** 2).mean().item())
            skip = sorted(set(static_channels or []) | set(forcing_channels or []))
            accs.append(spatial_corr(outs, y0, exclude_channels=skip if skip else None))
    n = max(len(raw), 1)
    return total / max(len(test_dataloader), 1), sum(accs) / n, (sum(raw) / n) ** 0.5


class Evaluator(Captured):
    """`test` (src/train.py:241-309) as a fused, captured step: per batch the model forward, `gcl_eval_colstats` (the
    one-step prediction with its static / forcing carry-forward formed on the fly, never stored, and the sums behind
    the three scores in one pass) and `gcl_eval_accumulate` (the batch's scores added to a float64 state on the
    device).  `update` synchronises nothing and reads nothing back; `results` is the one host read of a pass.

    The first `warmup` full batches run eagerly (the first of a shape also builds the cached weight vectors, which
    reads their sums back once), the next is captured into a hipGraph and later ones replay it: `use_graph` as for
    `TrainStep`.  A batch smaller than the largest seen so far (the last of a pass) and a sparse-GAT model run eagerly."""

    def __init__(self, model, lat_weights=None, channel_mask=None, spatial_mask=None, static_channels=None,
                 forcing_channels=None, use_residual=True, use_graph=None):
        self.model = model
        self.lat_weights, self.channel_mask, self.spatial_mask = lat_weights, channel_mask, spatial_mask
        self.static_channels, self.forcing_channels = static_channels, forcing_channels
        self.use_residual = bool(use_residual)
        self._state, self._stats, self._full = None, {}, None
        super().__init__(graph_enabled(use_graph), required=use_graph is True)

    def _buffers(self, B, C, device):
        """The state and the [B, C, 7] sums: made on the first eager call for a shape, never inside a capture."""
        if self._state is None or self._state.device != device:
            self._state = torch.zeros(4, dtype=torch.float64, device=device)
            self._stats = {}
        stats = self._stats.get((B, C))
        if stats is None:
            stats = self._stats[(B, C)] = torch.empty(B, C, hip.EVAL_NS, dtype=torch.float64, device=device)
        return self._state, stats

    def _work(self, X, y):
        B, G, _ = X.shape
        obs = self.model.obs_window
        C = X.shape[-1] // obs
        delta = self.model(X=X, attention_threshold=0.0)
        if delta.dim() == 2:
            delta = delta.unsqueeze(0)
        node_w, chan_w, wsum1 = _loss_weights(G, C, self.lat_weights, self.channel_mask, self.spatial_mask, X.device)
        kinds = _channel_kinds(C, self.static_channels, self.forcing_channels, X.device)
        state, stats = self._buffers(B, C, X.device)
        x_last = X.view(B, G, obs, C)[:, :, obs - 1, :]
        hip.eval_colstats(delta, x_last, y[:, :, :C], node_w, kinds, self.use_residual, stats)
        hip.eval_accumulate(stats, chan_w, kinds, 1.0 / max(wsum1 * B, 1e-12), G, state)

    @torch.no_grad()
    def update(self, X, y):
        """Add one batch (X [B, G, obs*C], y [B, G, P*C] on the GPU; step 0 of y is scored) to the running scores."""
        self.model.eval()
        if X.dim() == 2:
            X, y = X.unsqueeze(0), y.unsqueeze(0)
        if not X.is_contiguous():
            X = X.contiguous()
        shape = (tuple(X.shape), tuple(y.shape))
        if self._full is None or X.shape[0] > self._full[0][0] or (X.shape[0] == self._full[0][0] and shape != self._full):
            self._full = shape
            self.reset_graph()
        if shape != self._full or getattr(self.model, "using_sparse_gat", False):
            self._work(X, y)
        else:
            self._run(X, y)

    def input_buffers(self):
        """(X, y) the captured graph reads a full batch from, or None before the capture / on the eager path: a batch
        written into them (`DeviceLoader(buffers=evaluator.input_buffers)`) is scored without a copy."""
        return tuple(self._static) if self.graph_active else None

    def results(self, num_batches=None):
        """`test`'s triple (mean loss, mean ACC, sqrt(mean raw MSE)) over the batches since the last call - the one
        host read - and a reset.  num_batches: the reference's `len(test_dataloader)` for the loss mean (default:
        the batches seen)."""
        if self._state is None:
            return 0.0, 0.0, 0.0
        loss, acc, raw, n = self._state.cpu().tolist()
        self._state.zero_()
        n = max(n, 1.0)
        return loss / max(num_batches if num_batches is not None else n, 1), acc / n, (raw / n) ** 0.5

    def evaluate(self, batches, device=None):
        """`update` over an iterable of (X, y), then `results`; `device`: where to move host batches."""
        count = 0
        for X, y in batches:
            y = y.squeeze(0) if y.dim() == 4 else y
            if device is not None:
                X, y = X.to(device), y.to(device)
            self.update(X, y)
            count += 1
        return self.results(len(batches) if hasattr(batches, "__len__") else count)


_ADAM_DEFAULTS = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)
# the keys of a torch.optim.Adam param_groups entry besides `params` (its state_dict layout), in torch's order
_TORCH_GROUP_KEYS = ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "foreach", "capturable",
                     "differentiable", "fused", "decoupled_weight_decay")


def _group_params(g):
    ps = g["params"]
    return [ps] if isinstance(ps, torch.Tensor) else list(ps)


class FlatParams:
    """All trainable parameters of a module re-pointed into ONE flat fp32 buffer, with a flat
    gradient buffer whose slices are installed as `.grad` (so the backward kernels accumulate
    straight into the all-reduce bucket).

    `param_groups` (torch.optim.Adam's form: dicts with `params`, optionally `lr`, `betas`, `eps`, `weight_decay`):
    the bucket holds exactly the union of the groups' parameters, frozen ones included, so that an unfreeze needs no
    new bucket; parameters outside every group are not optimised.  Without groups the bucket holds the module's
    trainable parameters, in `module.parameters()` order."""

    def __init__(self, module: torch.nn.Module, param_groups=None):
        # `index[i]`: the index torch.optim.Adam gives params[i] in its state_dict - without groups its position in
        # module.parameters() (frozen parameters keep their slot), with groups its position in group order
        seen, self.params, self.index, pos = set(), [], [], 0
        if param_groups is None:
            for p in module.parameters():
                if id(p) in seen:
                    continue
                seen.add(id(p))
                if p.requires_grad:
                    self.params.append(p)
                    self.index.append(pos)
                pos += 1
            self.groups = [{"params": list(range(len(self.params)))}]  # bucket positions
        else:
            if isinstance(param_groups, dict):
                param_groups = [param_groups]
            self.groups = []
            for g in param_groups:
                members = []
                for p in _group_params(g):
                    if id(p) in seen:
                        raise ValueError("some parameters appear in more than one parameter group")
                    seen.add(id(p))
                    members.append(len(self.params))
                    self.params.append(p)
                    self.index.append(pos)
                    pos += 1
                self.groups.append(dict({k: v for k, v in g.items() if k != "params"}, params=members))
            if not self.params:
                raise ValueError("param_groups holds no parameters")
        self.num_module_params = pos
        dev = self.params[0].device
        # every parameter starts on a 256-byte boundary (the dense kernels read weight rows as
        # 16-byte vectors); the padding stays zero in the weights, the gradients and Adam's moments
        self.offsets, total = [], 0
        for p in self.params:
            self.offsets.append(total)
            total += (p.numel() + 63) // 64 * 64
        self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(total, dtype=torch.float32, device=dev)
        for p, off in zip(self.params, self.offsets):
            k = p.numel()
            self.flat[off:off + k].copy_(p.data.reshape(-1))
            p.data = self.flat[off:off + k].view(p.shape)
            p.grad = self.grad[off:off + k].view(p.shape)
        self.numel = total  # bucket length (with alignment padding)
        self.num_params = sum(p.numel() for p in self.params)
        # owner of every 64-float chunk of the bucket (the grouped Adam kernel's parameter lookup)
        owner = torch.empty(total // 64, dtype=torch.int32)
        for i, (p, off) in enumerate(zip(self.params, self.offsets)):
            owner[off // 64:(off + (p.numel() + 63) // 64 * 64) // 64] = i
        self.chunk_param = owner.to(dev)

    def zero_grad(self):
        if self.grad.is_cuda:
            hip.zero_(self.grad)  # stream memset through the C ABI (no torch fill kernel on the step)
        else:
            self.grad.zero_()     # (CPU buckets exist only in the gloo rehearsal tests of the sharding logic)


def shard_batch(X, y, rank: int, world: int):
    """Contiguous equal shards of the batch dimension: rank r owns samples
    [r*B_local, (r+1)*B_local).  The global batch must divide evenly."""
    B = X.shape[0]
    if B % world != 0:
        raise ValueError(f"global batch {B} is not divisible by world size {world}")
    k = B // world
    return X[rank * k:(rank + 1) * k], y[rank * k:(rank + 1) * k]


def allreduce_gradients(flat: "FlatParams", world: int) -> float:
    """C1, the only collective on the path: ONE all-reduce (sum) of the flat gradient bucket.
    Returns the factor the optimiser must apply (1/world: the reference loss is a mean over the
    batch, src/train.py:101-102, so the global gradient is the mean of the per-rank gradients
    when every rank holds the same number of samples)."""
    if world > 1:
        dist.all_reduce(flat.grad, op=dist.ReduceOp.SUM)
    return 1.0 / world


class FusedAdam:
    """torch.optim.Adam(param_groups) semantics (no amsgrad, no maximize) over a FlatParams bucket: one
    `gcl_adam_step_groups` for the whole bucket, with a learning rate, an active flag and a step counter per
    parameter, all on the device so that the update can sit inside a captured hipGraph.

    A parameter whose `requires_grad` is False is skipped as torch skips a parameter whose grad is None: its weights,
    moments and step stay untouched, and after an unfreeze its bias correction starts from its own step.
    `param_groups` mirrors torch's list (change a group's `lr` there); `beta1`, `beta2`, `eps` and `weight_decay`
    must be the same in every group."""

    def __init__(self, flat: FlatParams, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, param_groups=None):
        self.flat = flat
        dev = flat.flat.device
        given = flat.groups
        if param_groups is not None:
            if isinstance(param_groups, dict):
                param_groups = [param_groups]
            if len(param_groups) != len(flat.groups) or any(
                    [id(p) for p in _group_params(g)] != [id(flat.params[k]) for k in f["params"]]
                    for g, f in zip(param_groups, flat.groups)):
                raise ValueError("param_groups differ from the groups the FlatParams bucket was built with")
            given = param_groups
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        self.param_groups = []
        for g, f in zip(given, flat.groups):
            group = {k: g.get(k, defaults[k]) for k in ("lr", "betas", "eps", "weight_decay")}
            group["betas"] = tuple(group["betas"])
            if g.get("amsgrad", False) or g.get("maximize", False):
                raise ValueError("FusedAdam implements plain Adam only (amsgrad / maximize are not supported)")
            group["params"] = list(f["params"])  # bucket positions
            self.param_groups.append(group)
        self._check_uniform(self.param_groups)
        P = len(flat.params)
        self._group_of = [0] * P
        for gi, g in enumerate(self.param_groups):
            for k in g["params"]:
                self._group_of[k] = gi
        self.m = torch.zeros_like(flat.flat)
        self.v = torch.zeros_like(flat.flat)
        self.step_dev = torch.zeros(P, dtype=torch.int32, device=dev)
        self.bc_dev = torch.zeros(P, 2, dtype=torch.float32, device=dev)
        self.active_dev = torch.zeros(P, dtype=torch.int32, device=dev)
        self.lr_dev = torch.zeros(P, dtype=torch.float32, device=dev)
        self._flags = self._lrs = None
        self.sync()

    @staticmethod
    def _check_uniform(groups):
        for key in ("betas", "eps", "weight_decay"):
            vals = {tuple(g[key]) if key == "betas" else g[key] for g in groups}
            if len(vals) > 1:
                raise ValueError(f"FusedAdam needs one `{key}` for every parameter group, got {sorted(vals)}")

    # the hyper-parameters shared by all groups (and the first group's lr, the only one without groups)
    @property
    def lr(self):
        return self.param_groups[0]["lr"]

    @lr.setter
    def lr(self, value):
        for g in self.param_groups:
            g["lr"] = value

    @property
    def betas(self):
        return self.param_groups[0]["betas"]

    @property
    def eps(self):
        return self.param_groups[0]["eps"]

    @property
    def wd(self):
        return self.param_groups[0]["weight_decay"]

    @property
    def t(self) -> int:
        """The largest per-parameter step (all of them, while every parameter has been active)."""
        return int(self.step_dev.max().item()) if self.step_dev.numel() else 0

    def steps(self):
        """Per-parameter step counters (host list, bucket order)."""
        return [int(x) for x in self.step_dev.cpu()]

    def _upload(self, dst, values, dtype):
        src = torch.tensor(values, dtype=dtype)
        if dst.is_cuda:
            dst.copy_(src.pin_memory(), non_blocking=True)  # stream-ordered; the host does not wait
        else:
            dst.copy_(src)

    def sync(self) -> bool:
        """Bring the device tables in line with the host: the parameters' `requires_grad` (active flags) and the
        groups' `lr`.  Host-side comparisons only; a table is uploaded (without a device sync) only when it changed.
        Returns True when the active flags changed (a captured step must then be captured again)."""
        self._check_uniform(self.param_groups)
        flags = tuple(bool(p.requires_grad) for p in self.flat.params)
        changed = flags != self._flags
        if changed:
            self._upload(self.active_dev, [int(f) for f in flags], torch.int32)
            self._flags = flags
        lrs = tuple(float(g["lr"]) for g in self.param_groups)
        if lrs != self._lrs:
            self._upload(self.lr_dev, [lrs[gi] for gi in self._group_of], torch.float32)
            self._lrs = lrs
        return changed

    def step(self, grad_scale: float = 1.0):
        self.sync()
        b1, b2 = self.betas
        hip.adam_step_groups(self.flat.flat, self.flat.grad, self.m, self.v, self.flat.chunk_param, self.active_dev,
                             self.lr_dev, self.step_dev, self.bc_dev, b1, b2, self.eps, self.wd, grad_scale)

    def zero_grad(self):
        self.flat.zero_grad()

    def _torch_groups(self):
        """Each group's torch.optim.Adam state_dict indices."""
        if len(self.param_groups) == 1 and self.flat.num_module_params != len(self.flat.params):
            return [list(range(self.flat.num_module_params))]  # no groups: frozen module parameters keep their slot
        return [[self.flat.index[k] for k in g["params"]] for g in self.param_groups]

    def state_dict(self):
        """The dictionary `torch.optim.Adam(param_groups)` (without groups: `torch.optim.Adam(model.parameters())`)
        would hold after the same steps: indices in group order, one `param_groups` entry per group, a per-parameter
        `step / exp_avg / exp_avg_sq`, and no state for a parameter that was never stepped.  So `save_checkpoint`
        files written from the fused optimiser resume under the reference's `load_checkpoint` (src/train.py:37-49)."""
        steps, state = self.steps(), {}
        for p, i, off, t in zip(self.flat.params, self.flat.index, self.flat.offsets, steps):
            k = p.numel()
            if t > 0:
                state[i] = {"step": torch.tensor(float(t)), "exp_avg": self.m[off:off + k].view(p.shape).clone(),
                            "exp_avg_sq": self.v[off:off + k].view(p.shape).clone()}
        groups = []
        for g, idx in zip(self.param_groups, self._torch_groups()):
            group = {"lr": g["lr"], "betas": tuple(g["betas"]), "eps": g["eps"], "weight_decay": g["weight_decay"],
                     "amsgrad": False, "maximize": False, "foreach": None, "capturable": False,
                     "differentiable": False, "fused": None, "decoupled_weight_decay": False}
            group["params"] = idx
            groups.append(group)
        return {"state": {i: state[i] for i in sorted(state)}, "param_groups": groups}

    def load_state_dict(self, sd):
        """Inverse of `state_dict`; also accepts what torch.optim.Adam wrote for the same parameter groups (per-
        parameter steps included).  Restores each group's lr; raises on a group-count or size mismatch, as torch."""
        saved = sd["param_groups"]
        own = self._torch_groups()
        if len(saved) != len(own):
            raise ValueError("loaded state dict has a different number of parameter groups")
        if any(len(s["params"]) != len(o) for s, o in zip(saved, own)):
            raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
        for s in saved:
            if s.get("amsgrad", False) or s.get("maximize", False):
                raise ValueError("FusedAdam implements plain Adam only (amsgrad / maximize are not supported)")
        new_groups = [dict(g, lr=s["lr"], betas=tuple(s["betas"]), eps=s["eps"], weight_decay=s.get("weight_decay", 0.0))
                      for g, s in zip(self.param_groups, saved)]
        self._check_uniform(new_groups)
        # torch matches saved and current parameters by position within the groups
        saved_of = {}
        for s, o in zip(saved, own):
            for si, oi in zip(s["params"], o):
                saved_of[oi] = si
        steps = []
        m, v = torch.zeros_like(self.m), torch.zeros_like(self.v)
        for p, i, off in zip(self.flat.params, self.flat.index, self.flat.offsets):
            k = p.numel()
            si = saved_of[i]
            st = sd["state"].get(si, sd["state"].get(str(si)))
            if st is None:
                steps.append(0)
                continue
            if tuple(st["exp_avg"].shape) != tuple(p.shape):
                raise ValueError(f"optimizer state {si}: shape {tuple(st['exp_avg'].shape)} != {tuple(p.shape)}")
            m[off:off + k].copy_(st["exp_avg"].reshape(-1))
            v[off:off + k].copy_(st["exp_avg_sq"].reshape(-1))
            steps.append(int(float(st["step"])))
        self.m.copy_(m), self.v.copy_(v)
        self.step_dev.copy_(torch.tensor(steps, dtype=torch.int32))
        for g, n in zip(self.param_groups, new_groups):
            g.update({k: n[k] for k in ("lr", "betas", "eps", "weight_decay")})
        self.sync()


_DEFER_REDUCTIONS = os.environ.get("GCL_NO_DEFER", "0") in ("0", "")


class TrainStep(Captured):
    """One optimiser step on a local batch: forward, loss, backward, [all-reduce], Adam.

    With `use_graph` (default) the launch-heavy part of the step - ~160 kernel launches - is captured
    once into a hipGraph (via torch.cuda.CUDAGraph on the stream the kernels are enqueued on) and
    replayed; inputs are copied into static buffers first.  One GPU: the whole step including Adam
    is in the graph.  Several GPUs (or `split_finish`): zero-grad + forward + loss + backward are in
    the graph and the RCCL all-reduce + Adam stay ordinary stream operations after the replay, so
    no collective is ever captured.  A step then costs the host one graph launch instead of ~160
    kernel launches, which keeps it GPU-bound on hosts with slow launch paths."""

    def __init__(self, model, lr=1e-3, lat_weights=None, channel_mask=None, spatial_mask=None, use_residual=True,
                 ar_steps=1, world_size=1, use_graph=None, split_finish=None, static_channels=None,
                 forcing_channels=None, param_groups=None):
        self.model = model
        # param_groups (torch.optim.Adam's form, e.g. `optimiser.param_groups`): per-group lr; the bucket holds every
        # grouped parameter, frozen ones included, and a change of `requires_grad` between calls just works
        self.flat = FlatParams(model, param_groups)
        self.opt = FusedAdam(self.flat, lr=lr, param_groups=param_groups)
        self.lat_weights, self.channel_mask, self.spatial_mask = lat_weights, channel_mask, spatial_mask
        self._ar_steps, self.world = ar_steps, world_size
        self.use_residual = use_residual
        self.static_channels, self.forcing_channels = static_channels, forcing_channels
        # use_graph=True: the caller REQUIRES the hipGraph path (a failed capture raises);
        # use_graph=None: replay when the capture works, fall back to eager launches with a warning
        super().__init__(graph_enabled(use_graph), required=use_graph is True)
        self._sparse = bool(getattr(model, "using_sparse_gat", False))
        self.split_finish = (world_size > 1) if split_finish is None else bool(split_finish or world_size > 1)
        if world_size > 1:
            if not (dist.is_available() and dist.is_initialized()):
                raise RuntimeError(f"TrainStep(world_size={world_size}) needs an initialised torch.distributed process group")
            if dist.get_world_size() != world_size:
                raise RuntimeError(f"TrainStep(world_size={world_size}) but the process group has {dist.get_world_size()} ranks")
            self.sync_from_rank0()

    @property
    def ar_steps(self) -> int:
        return self._ar_steps

    @ar_steps.setter
    def ar_steps(self, value):
        """The autoregressive depth is baked into the captured graph: a new value drops it (the AR curriculum)."""
        if int(value) != self._ar_steps:
            self._ar_steps = int(value)
            self.reset_graph()

    def sync_from_rank0(self):
        """Only gradients are all-reduced, so replicas stay identical only if they START identical: rank 0's
        parameters and Adam state (per-parameter step counters included) are broadcast once (ranks built from
        different seeds or checkpoints would otherwise diverge silently)."""
        for t in (self.flat.flat, self.opt.m, self.opt.v, self.opt.step_dev):
            dist.broadcast(t, src=0)

    @property
    def launch_mode(self) -> str:
        if self.graph_active and self.split_finish:
            return "hipGraph replay (fwd+bwd; all-reduce + Adam eager)"
        return super().launch_mode

    def _fwd_bwd(self, X, y, threshold=0.0, epoch=0, batch_num=1):
        self.flat.zero_grad()
        loss = batch_loss(self.model, X, y, threshold, epoch, batch_num, self.lat_weights, self.ar_steps,
                          self.channel_mask, self.spatial_mask, self.static_channels, self.forcing_channels,
                          self.use_residual)
        # every parameter gradient lands in the flat bucket (preinstalled .grad slices) and is only read after the whole
        # backward, so the small final passes of the fused dense backward are queued and run in one launch per 16 layers
        defer = _DEFER_REDUCTIONS and loss.is_cuda
        if defer:
            hip.defer_begin()
        try:
            loss.backward(self._loss_root(loss))
        except BaseException:
            if defer:
                hip.defer_flush(drop=True)  # a failed backward: forget what it queued, launch nothing
            raise
        if defer:
            hip.defer_flush()
        return loss.detach()

    def _loss_root(self, loss):
        """The gradient of the loss with respect to itself: the constant one of functional.const_one (made once per device,
        never inside a capture, only ever read) instead of the fill launch autograd would issue in every step - and the
        loss's backward, which knows that tensor, multiplies nothing by it.  None: autograd's own."""
        if loss.dim() != 0 or not loss.is_cuda or loss.dtype != torch.float32:
            return None
        return const_one(loss)

    def _finish(self):
        scale = allreduce_gradients(self.flat, self.world)
        self.opt.step(grad_scale=scale)

    def _eager(self, X, y, threshold=0.0, epoch=0, batch_num=1):
        loss = self._fwd_bwd(X, y, threshold, epoch, batch_num)
        self._finish()
        return loss

    def _work(self, X, y, threshold=0.0, epoch=0, batch_num=1):
        if self.split_finish:  # the all-reduce + Adam run after the replay, outside the graph
            return self._fwd_bwd(X, y, threshold, epoch, batch_num)
        return self._eager(X, y, threshold, epoch, batch_num)

    def __call__(self, X, y, threshold=0.0, epoch=0, batch_num=1):
        if self.opt.sync():
            # a parameter was frozen or unfrozen since the last call (host-side check, no device sync): the captured
            # graph skips or computes the wrong dW work, so drop it; the next calls warm up and capture again
            self.reset_graph()
        if self._sparse and batch_num == 0:
            # SparseGATConv prunes the mesh graph on this step (src/models.py:138-149): run it eagerly and
            # drop the captured graph, which was recorded over the old edge list; two eager steps follow so
            # that the CSR of the pruned list (and of its loop-completed form) exists before re-capturing
            self.reset_graph()
            return self._eager(X, y, threshold, epoch, batch_num)
        loss = self._run(X, y, threshold=threshold, epoch=epoch, batch_num=batch_num)
        if self.split_finish:
            self._finish()
        return loss.detach()

    def input_buffers(self):
        """(X, y) the captured graph reads its batch from, or None before the capture / on the eager path: fill them
        in place and pass them to the step to skip its per-step copy of the batch."""
        return tuple(self._static) if self.graph_active else None


def build_optimizer(model, config, pretrained: bool):
    """The optimiser of src/main.py:190-211: when fine-tuning a pretrained model with `freeze_processor_epochs > 0`
    the processor is frozen (`requires_grad = False`) and gets its own group at `learning_rate *
    finetune_processor_lr_factor`; otherwise one group over `model.parameters()`.  A torch.optim.Adam, as in the
    reference: `train()` runs its groups on the fused step."""
    freeze_proc = getattr(config, "freeze_processor_epochs", 0)
    proc_lr_factor = getattr(config, "finetune_processor_lr_factor", 0.1)
    base_lr = config.learning_rate
    if pretrained and freeze_proc > 0:
        proc_params = list(model.processor.parameters())
        proc_ids = {id(p) for p in proc_params}
        other_params = [p for p in model.parameters() if id(p) not in proc_ids]
        for p in proc_params:
            p.requires_grad = False
        return torch.optim.Adam([{"params": other_params, "lr": base_lr},
                                 {"params": proc_params, "lr": base_lr * proc_lr_factor}])
    return torch.optim.Adam(params=model.parameters(), lr=base_lr)


def loss_masks(config, dataset_metadata, device):
    """The loss weights and channel roles `train()` derives from the configuration and the dataset's metadata
    (src/train.py:333-377), as the keyword arguments `TrainStep`, `test` and `Evaluator` share: latitude weights,
    the channel mask that takes static / forcing channels out of the loss, the boundary and ROI node masks."""
    device = torch.device(device)
    lat_weights = None
    if getattr(config, "use_latitude_weighting", False) and dataset_metadata:
        if getattr(dataset_metadata, "flat_grid", False) and hasattr(dataset_metadata, "cordinates"):
            lat_weights = get_lat_weights(0, 0, device, flat_lats=dataset_metadata.cordinates[0])
        else:
            lat_weights = get_lat_weights(dataset_metadata.num_latitudes, dataset_metadata.num_longitudes, device)

    static_ch = getattr(config, "static_channels", [])
    forcing_ch = getattr(config, "forcing_channels", [])
    no_loss_ch = sorted(set(static_ch) | set(forcing_ch))
    channel_mask = None
    if no_loss_ch:
        C_total = config.data.num_features_used
        channel_mask = torch.ones(C_total, device=device)
        for ch in no_loss_ch:
            if 0 <= ch < C_total:
                channel_mask[ch] = 0.0

    spatial_mask = None
    bmw = getattr(config, "boundary_mask_width", 0)
    if bmw > 0 and dataset_metadata is not None:
        n_lon = getattr(dataset_metadata, "num_longitudes", None)
        n_lat = getattr(dataset_metadata, "num_latitudes", None)
        if n_lon and n_lat and not getattr(dataset_metadata, "flat_grid", False):
            spatial_mask = build_boundary_mask(n_lon, n_lat, bmw, device)
    roi_spatial_mask = None
    if getattr(config, "roi_only_loss", False) and dataset_metadata is not None:
        roi = getattr(dataset_metadata, "is_regional", None)
        if roi is not None:
            roi_spatial_mask = torch.as_tensor(roi, dtype=torch.float32, device=device).view(1, -1, 1)
    spatial_mask = combine_spatial_masks(spatial_mask, roi_spatial_mask)
    return dict(lat_weights=lat_weights, channel_mask=channel_mask, spatial_mask=spatial_mask,
                static_channels=static_ch, forcing_channels=forcing_ch,
                use_residual=getattr(config, "use_residual", True))


def train(model, train_dataloader, val_dataloader, test_dataloader, optimiser, num_epochs, device, config,
          results_save_dir, dataset_metadata=None, print_losses=True, wandb_log=False, resume_checkpoint=None, *,
          world_size=1, use_graph=None, evaluator=None):
    """src/train.py:311-524 on the fused step: the same masks, AR curriculum, attention-threshold schedule, processor
    unfreeze, early stopping, `training_log.txt`, best model, `checkpoint.pth` and results JSON, with every batch one
    `TrainStep` call (captured and replayed; dropped and captured again at an unfreeze or an AR change).

    `optimiser` is the reference's torch.optim.Adam (e.g. from `build_optimizer`): its `param_groups` become the fused
    step's groups and its state, if any, is carried over; the fused state is written back into it at the end.
    Checkpoints hold the optimiser state in torch's layout, so the reference's `train()` resumes them and this one
    resumes the reference's.  `dataset_metadata` and `config` are duck-typed (the attributes the reference reads);
    batches are `(X, y)` pairs of CPU or device tensors from any iterable.  `test_dataloader` is unused, as in the
    reference.  With `world_size > 1` each rank passes its own shard of the batches and rank 0 writes the files.
    `evaluator`: an `Evaluator` built from `loss_masks(config, dataset_metadata, device)`; validation then runs on the
    fused, captured step instead of `test` (one host read per pass)."""
    import json
    from datetime import datetime

    if wandb_log:
        raise NotImplementedError("wandb logging is not provided by this package (see README, 'What is not provided')")
    if not isinstance(optimiser, torch.optim.Adam) or any(g.get("amsgrad") or g.get("maximize")
                                                          for g in optimiser.param_groups):
        raise ValueError("train() runs torch.optim.Adam (no amsgrad, no maximize) on the fused step; "
                         f"got {type(optimiser).__name__}")
    device = torch.device(device)
    main = world_size == 1 or dist.get_rank() == 0
    say = print if (print_losses and main) else (lambda *a, **k: None)

    masks = loss_masks(config, dataset_metadata, device)
    lat_weights, channel_mask, spatial_mask = masks["lat_weights"], masks["channel_mask"], masks["spatial_mask"]
    static_ch, forcing_ch, use_residual = masks["static_channels"], masks["forcing_channels"], masks["use_residual"]

    ar_steps = 1
    max_ar = config.max_ar_steps
    epochs_per_stage = num_epochs // max_ar if max_ar > 0 else num_epochs

    step = TrainStep(model, lr=optimiser.defaults["lr"], lat_weights=lat_weights, channel_mask=channel_mask,
                     spatial_mask=spatial_mask, use_residual=use_residual, ar_steps=ar_steps, world_size=world_size,
                     use_graph=use_graph, static_channels=static_ch, forcing_channels=forcing_ch,
                     param_groups=optimiser.param_groups)
    if optimiser.state:
        step.opt.load_state_dict(optimiser.state_dict())

    train_losses, val_losses = [], []
    best_val_loss, patience_counter, start_epoch = float("inf"), 0, 0
    resumed = bool(resume_checkpoint) and os.path.exists(resume_checkpoint)
    if resumed:
        st = load_checkpoint(resume_checkpoint, model, step.opt, device)
        start_epoch, ar_steps = st["start_epoch"], st["ar_steps"]
        best_val_loss, patience_counter = st["best_val_loss"], st["patience_counter"]
        train_losses, val_losses = st["train_losses"], st["val_losses"]
        say(f"\n>>> Resuming at epoch {start_epoch + 1}, AR={ar_steps}, best_val_loss={best_val_loss:.5f}, "
            f"patience={patience_counter} <<<\n")

    log_path = os.path.join(results_save_dir, "training_log.txt")

    def _log(msg):
        if main:
            with open(log_path, "a") as f:
                f.write(msg + "\n")

    _log(f"=== Training started: {datetime.now().isoformat()} ===")
    _log(f"epochs={num_epochs}  max_ar={max_ar}  epochs_per_stage={epochs_per_stage}")
    if resumed:
        _log(f">>> Resumed from epoch {start_epoch}, AR={ar_steps}, best_vl={best_val_loss:.5f}")
    _log(f"{'epoch':>5}  {'ar':>2}  {'train_loss':>10}  {'val_loss':>10}  {'val_ACC':>8}  {'best_vl':>10}  "
         f"{'patience':>8}  timestamp")
    _log("-" * 90)

    def _validate():
        if evaluator is not None:
            return evaluator.evaluate(val_dataloader, device=device)
        return test(model, val_dataloader, None, device, lat_weights, spatial_mask=spatial_mask,
                    channel_mask=channel_mask, static_channels=static_ch, forcing_channels=forcing_ch,
                    use_residual=use_residual)

    if start_epoch == 0:
        v_loss, v_acc, v_rmse = _validate()
        say(f"[Init] val_loss={v_loss:.5f} val_acc={v_acc:.4f} raw_RMSE={v_rmse:.4f}")
        _log(f"{'init':>5}  {'--':>2}  {'--':>10}  {v_loss:10.5f}  {v_acc:8.4f}  {'--':>10}  {'--':>8}  "
             f"{datetime.now().strftime('%H:%M:%S')}")

    freeze_proc_epochs = getattr(config, "freeze_processor_epochs", 0)
    total = torch.zeros((), dtype=torch.float64, device=device)
    for epoch in range(start_epoch, num_epochs):
        if freeze_proc_epochs > 0 and epoch == freeze_proc_epochs:
            for p in model.processor.parameters():
                p.requires_grad = True  # the next step sees it: new active flags, graph captured again
            say(f"\n>>> Processor unfrozen (epoch {epoch}), lr = {optimiser.param_groups[-1]['lr']:.1e} <<<\n")
        correct_ar = min(1 + epoch // epochs_per_stage, max_ar)
        if correct_ar > ar_steps:
            ar_steps = correct_ar
            patience_counter = 0
            say(f"\n>>> Curriculum: training {ar_steps} autoregressive steps ahead <<<\n")
        step.ar_steps = ar_steps
        threshold = update_attention_threshold(epoch)
        say(f"Epoch {epoch} (AR={ar_steps}) with attention threshold {threshold}")

        model.train()
        total.zero_()
        n = 0
        for i, (X, y) in enumerate(train_dataloader):
            y = y.squeeze(0) if y.dim() == 4 else y
            loss = step(X.to(device), y.to(device), threshold, epoch, i)
            total += loss  # before the next call: a replayed step returns the same static tensor
            n += 1
        epoch_train_loss = total.item() / max(n, 1)  # the one host read of the epoch
        epoch_val_loss, epoch_val_acc, epoch_raw_rmse = _validate()
        say(f"[Epoch {epoch + 1}] train_loss={epoch_train_loss:.5f}  val_loss={epoch_val_loss:.5f}  "
            f"val_ACC={epoch_val_acc:.4f}  raw_RMSE={epoch_raw_rmse:.4f}")
        train_losses.append(epoch_train_loss)
        val_losses.append(epoch_val_loss)

        if best_val_loss - epoch_val_loss > config.early_stopping_delta:
            best_val_loss = epoch_val_loss
            if main:
                torch.save(model.state_dict(), os.path.join(results_save_dir, FileNames.SAVED_MODEL))
            patience_counter = 0
        else:
            patience_counter += 1
        _log(f"{epoch + 1:5d}  {ar_steps:2d}  {epoch_train_loss:10.5f}  {epoch_val_loss:10.5f}  {epoch_val_acc:8.4f}  "
             f"{best_val_loss:10.5f}  {patience_counter:8d}  {datetime.now().strftime('%H:%M:%S')}")
        if main:
            save_checkpoint(os.path.join(results_save_dir, FileNames.CHECKPOINT), model, step.opt, epoch, ar_steps,
                            best_val_loss, patience_counter, train_losses, val_losses)
        if patience_counter >= config.early_stopping_patience:
            say("Early stopping.")
            _log(f">>> Early stopping at epoch {epoch + 1}")
            break

    _log(f"=== Training finished: {datetime.now().isoformat()} ===")
    results = {"train_losses": train_losses, "val_losses": val_losses}
    if main:
        with open(os.path.join(results_save_dir, FileNames.SAVED_RESULTS), "w") as fh:
            json.dump(results, fh)
    optimiser.load_state_dict(step.opt.state_dict())  # the caller's optimiser ends where the fused one did
    return results
