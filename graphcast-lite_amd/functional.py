"""Module-level autograd Functions over the C ABI (one Function per MLP / conv stack).

Each Function runs a whole reference module (`MLP.forward` src/models.py:106-109; the GCN / GAT /
SparseGAT / SimpleConv branches of `GraphLayer.forward` src/models.py:406-440) as a sequence of
`libgcl_hip` launches and keeps only what its backward needs.  Buffers passed between layers hold
PRE-activation values (see include/gcl.h, "Activation chaining").

Gradient delivery: when a parameter already has a `.grad` tensor the backward ACCUMULATES into it
in place on the device and returns None for that input (fused accumulation - no extra add kernel
per parameter, and gradients land directly in the flat bucket that the data-parallel all-reduce
uses); otherwise it returns a fresh gradient tensor and autograd stores it as usual.
"""
from typing import List, NamedTuple, Optional

import os

import torch

from . import hip
from .stack_plan import Layout, StackPlan, Switches, plan_gcn_stack


def _grad_slot(p: Optional[torch.Tensor], needs: bool):
    """(tensor to write into, accumulate?, return_value_is_none?)"""
    if p is None or not needs:
        return None, False, True
    if p.grad is not None:
        return p.grad, True, True
    return torch.zeros_like(p), False, False


class _Grads:
    """Collects per-parameter gradient destinations for one backward call."""

    def __init__(self, params: List[Optional[torch.Tensor]], needs: List[bool]):
        self.dst, self.acc, self.ret_none = [], [], []
        for p, nd in zip(params, needs):
            d, a, r = _grad_slot(p, nd)
            self.dst.append(d)
            self.acc.append(a)
            self.ret_none.append(r)

    def out(self):
        return tuple(None if r else d for d, r in zip(self.dst, self.ret_none))


_ZERO = {}  # device -> the zero scalar every token expands: written once, when it is made, and never again


def _token(like: torch.Tensor, shape):  # a stride-0 zero: stands in autograd's graph for rows that travel through a GradLanding
    """No launch: the zero is made once per device.  Nothing writes through a token - autograd adds gradients out of place
    when a tensor overlaps itself - so all tokens may share it.  The first use on a device inside a stream capture makes
    a zero of its own instead (memory of the capture's pool must not outlive it)."""
    z = _ZERO.get(like.device)
    if z is None:
        if like.is_cuda and torch.cuda.is_current_stream_capturing():
            return like.new_zeros(()).expand(shape)
        with torch.inference_mode(False):
            z = _ZERO[like.device] = torch.zeros((), dtype=torch.float32, device=like.device)
    return z.expand(shape)


_ONE = {}  # device -> the constant one that stands for d loss / d loss (const_one): never written after it is made


def const_one(like: torch.Tensor):
    """The upstream gradient of a scalar loss as ONE tensor per device, made outside any capture and only ever read (like
    the zero of _token).  ARStepLossFn.backward recognises it by its address and then has nothing to multiply.  None when
    the first use on a device falls inside a stream capture (the caller then lets autograd make its own)."""
    one = _ONE.get(like.device)
    if one is None:
        if like.is_cuda and torch.cuda.is_current_stream_capturing():
            return None
        with torch.inference_mode(False):
            one = _ONE[like.device] = torch.ones((), dtype=torch.float32, device=like.device)
    return one


def _loss_grad_inplace() -> bool:
    """GCL_NO_LOSS_GRAD_INPLACE=1 (read per call): the loss gradient is born dense, scaled by gcl_ar_step_bwd and widened
    by gcl_pad_rows again."""
    return os.environ.get("GCL_NO_LOSS_GRAD_INPLACE", "0") != "1"


def _wide_in_place(dy: torch.Tensor, Fp: int):
    """dy [B, rows, Fo] (Fo <= Fp) as the [B, rows, Fp] tensor it is a column slice of, when it can be read so where it
    lies: unit channel stride, rows Fp apart, samples rows * Fp apart, a 16-byte aligned base and a storage that holds all
    B * rows * Fp floats behind it (a foreign view may end inside the last row's padding).  None otherwise.  The columns
    Fo.. must hold finite values, as gcl_linear_bwd_all asks of padded rows; the library's own producers write zeros."""
    if dy.dim() != 3 or dy.dtype != torch.float32 or not dy.is_cuda:
        return None
    B, rows, Fo = dy.shape
    if Fo > Fp or rows == 0 or dy.stride(2) != 1 or dy.stride(1) != Fp or dy.stride(0) != rows * Fp or dy.data_ptr() % 16:
        return None
    off = dy.storage_offset()
    if (off + B * rows * Fp) * 4 > dy.untyped_storage().nbytes():
        return None
    return torch.as_strided(dy, (B, rows, Fp), (rows * Fp, Fp, 1), off)


def _flat3(x: torch.Tensor):
    """[B,n,F] (or [n,F]) -> contiguous [B,n,F]."""
    if x.dim() == 2:
        x = x.unsqueeze(0)
    if not x.is_contiguous():
        x = x.contiguous()
    return x


# ------------------------------------------------------------------------------------------------
# MLP: Linear -> PReLU -> ... -> Linear (-> LayerNorm node)
# params layout: [W1, b1, a1, W2, b2, a2, ..., WL, bL] (+ [gamma, beta])
# ------------------------------------------------------------------------------------------------
class MLPFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, owner, has_ln: bool, eps: float, *params):
        L = (len(params) - (2 if has_ln else 0) + 1) // 3
        shape = x.shape
        x2 = hip.rows2d(x.detach())
        zs = []
        cur, slope = x2, None
        out = stats = None
        for k in range(L):
            # the last two or three Linear layers, and the LayerNorm where it fits, in one launch when the chained kernel
            # takes them (hip.mlp_fwd_chain: the same z_k, output and statistics, bit for bit); the layers in front of
            # such a run, and every other MLP, layer by layer
            if 2 <= L - k <= 3:
                tail = hip.mlp_fwd_chain(cur, [params[3 * j].detach() for j in range(k, L)],
                                         [params[3 * j + 1].detach() for j in range(k, L)],
                                         [params[3 * j + 2].detach() for j in range(k, L - 1)], slope,
                                         ln=(params[-2].detach(), params[-1].detach(), eps) if has_ln else None)
                if tail is not None:
                    zs.extend(tail[0])
                    cur, out, stats = tail[0][-1], tail[1], tail[2]
                    break
            W, b = params[3 * k], params[3 * k + 1]
            z = hip.linear_fwd(cur, W.detach(), b.detach(), slope)
            zs.append(z)
            cur = z
            slope = params[3 * k + 2].detach() if k < L - 1 else None
        if out is None:
            out = cur
            if has_ln:
                out, stats = hip.layernorm_fwd(cur, params[-2].detach(), params[-1].detach(), eps)
        ctx.owner, ctx.has_ln, ctx.L = owner, has_ln, L
        ctx.x2, ctx.zs, ctx.stats = x2, zs, stats
        ctx.params = params
        return out.view(shape[:-1] + (out.shape[-1],))

    @staticmethod
    def backward(ctx, dy):
        params, L = ctx.params, ctx.L
        needs = list(ctx.needs_input_grad[4:])
        G = _Grads(list(params), needs)
        dy2 = hip.rows2d(dy)
        zs = ctx.zs
        if ctx.has_ln:
            gi, bi = len(params) - 2, len(params) - 1
            dgam = G.dst[gi] if G.dst[gi] is not None else torch.zeros_like(params[gi])
            dbet = G.dst[bi] if G.dst[bi] is not None else torch.zeros_like(params[bi])
            dz = hip.layernorm_bwd(dy2, zs[-1], params[gi].detach(), ctx.stats, dgam, dbet, G.acc[gi] and G.acc[bi])
        else:
            dz = dy2
        dx = None
        for k in range(L - 1, -1, -1):
            W = params[3 * k].detach()
            inp = ctx.x2 if k == 0 else zs[k - 1]
            slope = None if k == 0 else params[3 * k - 1].detach()
            wi, bi = 3 * k, 3 * k + 1
            dW = G.dst[wi] if G.dst[wi] is not None else torch.zeros_like(params[wi])
            db = G.dst[bi]
            if k > 0:
                # one fused launch: dz_{k-1}, dW_k, db_k, d(slope_{k-1})
                dz = hip.linear_bwd_all(dz, W, inp, slope, G.dst[3 * k - 1], dW, db, None, G.acc[wi], acc_db=G.acc[bi])
            elif ctx.needs_input_grad[0]:
                # first layer with a differentiable input: dx, dW and db from one read of dz
                dx = hip.linear_bwd_all(dz, W, inp, None, None, dW, db, None, G.acc[wi], acc_db=G.acc[bi],
                                        act=hip.ACT_NONE)
            elif db is not None and G.acc[bi] != G.acc[wi]:  # the dW kernel shares one flag between dW and db
                hip.linear_bwd_dw(dz, inp, None, dW, None, G.acc[wi])
                hip.colsum(dz, db, G.acc[bi])
            else:
                hip.linear_bwd_dw(dz, inp, None, dW, db, G.acc[wi])
        if dx is not None:
            dx = dx.view(dy.shape[:-1] + (dx.shape[-1],))
        return (dx, None, None, None) + G.out()


# ------------------------------------------------------------------------------------------------
# GCN stack: conv -> PReLU(shared) -> conv -> ... -> conv (-> LayerNorm node)
# params layout: [W1, b1, ..., WL, bL, slope] (+ [gamma, beta]);  slope may be None when L == 1
# ------------------------------------------------------------------------------------------------
_LN_COLSUM = os.environ.get("GCL_NO_LN_COLSUM", "0") in ("0", "")
_ROWS_OUT = os.environ.get("GCL_NO_ROWS_OUT", "0") in ("0", "")


def _row_skip() -> bool:
    """Rows that a stage boundary drops are neither written nor read (GCL_NO_ROW_SKIP=1: today's dense launches).  Read
    per call, so a test can compare the two."""
    return os.environ.get("GCL_NO_ROW_SKIP", "0") in ("0", "")


def _split_grad() -> bool:
    """The encoder stack's backward reads its incoming gradient where its two producers left it (GCL_NO_SPLIT_GRAD=1:
    they copy it into one buffer first).  Read per call."""
    return os.environ.get("GCL_NO_SPLIT_GRAD", "0") in ("0", "")


def _split_out() -> bool:
    """The encoder's last conv stores its output where the two readers take it from (GCL_NO_SPLIT_OUT=1: it writes one
    tensor and each reader copies its rows).  Read per call."""
    return os.environ.get("GCL_NO_SPLIT_OUT", "0") in ("0", "")


def _compact_store() -> bool:
    """The first processor layer's transposed aggregation stores the batch-dependent rows of its output compact
    (GCL_NO_COMPACT_STORE=1: it writes them in place and a gather launch copies them).  Read per call."""
    return os.environ.get("GCL_NO_COMPACT_STORE", "0") in ("0", "")


def _fold_sum(g3, inv_fold, r: int, B: int, dst):
    """The batch sums of g3's folded rows (MeshLatFn: inv_fold) land r to a sample in dst [B, r, F]."""
    if r > 1:
        hip.gather2_rows(g3, inv_fold, None, None, B * r, B, sum_batch=True, out=dst, deal=r)
    elif r == 1:
        tmp = hip.gather2_rows(g3, inv_fold, None, None, B * r, B, sum_batch=True)
        hip.copy_rows(tmp.view(B, r, g3.shape[-1]), dst)


def _lat_first_layer_bwd(lat, enc3, dz3, W, dW, acc_dw: bool, want_dx: bool, Pc=None, enc_shape=None, dzc=None):
    """Dense backward of a first processor layer whose input was read through a LatSource: dz3 [B, M, D'] is the
    gradient of the layer's transformed mesh rows (GCN: A^T dp, GAT: dh).  Returns the gradient of the encoder output
    [B, ne, D] (or None when the shared landing buffer took it / no gradient is wanted); dW is written / accumulated in
    place.  Pc: the compact encoder rows [B, Md + r, D] when the forward already copied them.  dzc: the compact gradient
    rows [B, Md + r, D'] with the Md dependent rows already in place (hip.aggregate_compact stored them there: those rows
    of dz3 are then unwritten), the folded rows still to be summed from dz3."""
    _, _, inv_a, inv_fold = lat.maps
    B, ne, D = enc_shape if enc3 is None else enc3.shape  # (enc3 may be None when Pc is given: only its shape is needed)
    G, Md, r = lat.G, lat.Md, lat.r
    nc = Md + r
    Fo = dz3.shape[-1]
    dz3 = dz3 if dz3.is_contiguous() else dz3.contiguous()
    # compact gradient rows [B, Md + r, Fo]: dependent rows gathered, folded rows summed over the batch
    if dzc is None:
        dzc = torch.empty(B, nc, Fo, dtype=torch.float32, device=dz3.device)
        if Md > 0:
            hip.gather2_rows(dz3, inv_a[G: G + Md], None, None, Md, B, out=dzc[:, :Md])
    _fold_sum(dz3, inv_fold, r, B, dzc[:, Md:])
    if Pc is None:  # the encoder rows behind the mesh latents
        Pc = hip.copy_rows(enc3[:, G:, :], torch.empty(B, nc, D, dtype=torch.float32, device=dz3.device))
    if not want_dx:
        hip.linear_bwd_dw(dzc.view(B * nc, Fo), Pc.view(B * nc, D), None, dW, None, acc_dw)
        dxc = None
    else:
        dxc = hip.linear_bwd_all(dzc.view(B * nc, Fo), W, Pc.view(B * nc, D), None, None, dW, None, None, acc_dw,
                                 act=hip.ACT_NONE).view(B, nc, D)
    if GradLanding.keep_tail(lat.landing, dxc):  # the encoder stack's backward reads dxc where it is
        return None
    buf, _ = GradLanding.tail(lat.landing)
    if dxc is None:
        return None
    out = buf if buf is not None else torch.zeros(B, ne, D, dtype=torch.float32, device=dz3.device)
    hip.copy_rows(dxc, out[:, G:])  # (shared buffer: the head rows were written by the decoder-input gather's backward)
    return None if buf is not None else out


class LatSource:
    """The mesh latents of the compact pipeline as a VIEW of the encoder output enc [B, ne, D] (rows per sample:
    [G grid | Md batch-dependent mesh | r folded batch-invariant mesh rows], see MeshLatFn): mesh row i of sample b is
    enc[b, tab[i]] (tab[i] >= 0) or the flat row ~tab[i] of enc viewed as [B * ne, D] (tab[i] < 0).  A GCN stack given
    one reads its first layer's input through the table (gcl_gcn_layer_fwd_tab) - the [B, M, D] latents are never
    written - and runs that layer's dense backward on the COMPACT rows: by linearity the gradient of a folded row is
    (sum_b dz[b, i]) W and its dW term (sum_b dz[b, i])^T enc_row, so 81 % of the rows (64x32 grid) cost one batch sum
    instead of B dense rows.  maps = MeshLatFn's (map_a, map_b, inv_a, inv_fold)."""

    def __init__(self, tab, maps, M: int, G: int, Md: int, r: int, landing=None, smap=None, tab_c=None, tail=None):
        """smap: int32 [M], mesh row -> its row among the Md dependent rows of the compact gradient, or -1 (the inverse of
        inv_a[G: G + Md]; None when that is no one-to-one map).  tab_c = (ne, table): compact_tab(ne), made by the owner once.
        tail: the rows enc[:, G:, :] as a tensor [B, Md + r, D] of their own, where the encoder stored them there
        (GradLanding.split_out) - `enc` itself is then a stride-0 token, and readers take `tail` through compact_tab."""
        self.tab, self.maps, self.M, self.G, self.Md, self.r, self.landing = tab, maps, M, G, Md, r, landing
        self.smap, self.tail = smap, tail
        self._compact = {} if tab_c is None else {tab_c[0]: tab_c[1]}

    def compact_tab(self, ne: int):
        """The table relative to the COMPACT rows enc[:, G:, :] copied to [B, Md + r, D] (a GAT layer transforms those
        first): own rows shift by G, flat row b' * ne + G + k becomes b' * (Md + r) + k."""
        t = self._compact.get(ne)
        if t is None:
            tab = self.tab.to(torch.int64)
            f = -tab - 1
            bq = torch.div(f, ne, rounding_mode="floor")
            flat_c = bq * (self.Md + self.r) + (f - bq * ne - self.G)
            t = torch.where(tab >= 0, tab - self.G, -flat_c - 1).to(torch.int32).contiguous()
            self._compact[ne] = t
        return t


def stack_switches() -> Switches:
    """What plan_gcn_stack obeys, read here and nowhere else in GCNStackFn.forward: the two module attributes as the import
    (or a test) left them, the environment per call."""
    return Switches(ln_colsum=_LN_COLSUM, rows_out=_ROWS_OUT, row_skip=_row_skip(), split_grad=_split_grad())


def _expect_dense(t, B: int, n: int, F: int, aligned: bool = True):
    """The plan took `t` for a fresh contiguous [B, n, F] tensor when it asked the kernels' gates: anything else is an error,
    never another path.  aligned=False: the gate asked looks at strides alone."""
    if tuple(t.shape) != (B, n, F) or not t.is_contiguous() or (aligned and t.data_ptr() % 16):
        raise RuntimeError(f"GCN stack: a layer received {tuple(t.shape)} with strides {t.stride()} where its plan assumed a "
                           f"dense 16-byte aligned [{B}, {n}, {F}]")


def _stack_act(owner, slope_p):
    """Activation between the convs: learnable PReLU slope (params[2L]), SiLU, or ReLU as a PReLU with the owner's constant
    zero slope (src/models.py:154-163, :316)."""
    return getattr(owner, "act_kind", hip.ACT_PRELU), (slope_p.detach() if slope_p is not None
                                                       else getattr(owner, "const_slope", None))


class _StackIO(NamedTuple):
    """What the steps of one forward call reach beside their operands."""
    plan: StackPlan
    graph: object
    lat: object
    split: object
    out_head: Optional[torch.Tensor]
    present: Optional[torch.Tensor]


# One function per ConvStep.kind: (step, io, input, activation, slope, W, b) -> (what the backward keeps, the next input)
def _conv_tab(st, io, cur, act, slope, W, b):
    tab = io.lat.tab if io.plan.enc_shape is None else io.lat.compact_tab(io.plan.enc_shape[1])
    p = hip.gcn_layer_fwd_tab(io.graph, cur, tab, act, slope, W, b)
    return p, p


def _conv_split(st, io, cur, act, slope, W, b):
    # the encoder output: grid rows straight into the decoder's input, mesh rows compact; nobody reads it whole
    B, n = io.plan.B, io.plan.n
    tail = torch.empty(B, n - io.out_head.shape[1], st.Fout, dtype=torch.float32, device=cur.device)
    hip.gcn_layer_fwd_split(io.graph, cur, act, slope, W, b, io.out_head, tail)
    io.split.keep_split_out(tail)
    return None, _token(cur, (B, n, st.Fout))  # (the backward of a stack without LayerNorm never reads its last output)


def _conv_fused(st, io, cur, act, slope, W, b):
    # ONE kernel (csrc/gcn_layer.hip): gather-aggregate the activated input rows, then the dense transform; an output width
    # that is not a multiple of 4 (33 / 19 variables) is stored ldh wide with zero padding columns
    p = hip.gcn_layer_fwd(io.graph, cur, act, slope, W, b, rows_out=st.rows_out, present=io.present if st.present else None)
    return p, p


def _conv_two_kernel_padded(st, io, cur, act, slope, W, b):
    # two-kernel path of the padded last layer: zero weight rows / bias entries for the extra columns
    B, n = io.plan.B, io.plan.n
    Wp = torch.nn.functional.pad(W, (0, 0, 0, st.ldh - st.Fout))
    bp = torch.nn.functional.pad(b, (0, st.ldh - st.Fout))
    h = hip.linear_fwd(cur.view(B * n, -1), Wp, None, slope, act=act)
    p = hip.aggregate(io.graph, h.view(B, n, st.ldh), bp)
    return p, p[..., :st.Fout]


def _conv_two_kernel(st, io, cur, act, slope, W, b):
    B, n = io.plan.B, io.plan.n
    h = hip.linear_fwd(cur.view(B * n, -1), W, None, slope, ld_out=st.ldh, act=act)  # padded scratch: 16-B loads in the gather
    p = hip.aggregate(io.graph, torch.as_strided(h, (B, n, st.Fout), (n * st.ldh, st.ldh, 1)), b)
    return p, p


_CONV = {"tab": _conv_tab, "split": _conv_split, "fused": _conv_fused, "two_kernel_padded": _conv_two_kernel_padded,
         "two_kernel": _conv_two_kernel}


class _Incoming(NamedTuple):
    """The gradient a stack's backward received (_incoming_grad)."""
    kind: str  # dense | mapped | parts | wide
    dy: torch.Tensor  # dense: contiguous [B, rows, F]; wide: as it came; mapped / parts: the token (only its shape is used)
    dy_map: Optional[tuple]  # mapped: (source, row map) for hip.layernorm_bwd
    parts: Optional[tuple]  # parts: (head rows [B, head, F], tail rows [B, n - head, F])
    wide: Optional[torch.Tensor]  # wide: dy as the [B, rows, ldh] tensor it is a column slice of
    compact: bool  # the first layer's transposed aggregation stores the batch-dependent rows compact


def _incoming_grad(plan: StackPlan, split, land, lat, graph, dy) -> _Incoming:
    """Claims what the landings hold for this stack and says which of the four forms the gradient has; the only reader of
    GCL_NO_LOSS_GRAD_INPLACE and GCL_NO_COMPACT_STORE in the backward."""
    dy, parts = GradLanding.claim_parts(split, dy)
    dy, dy_map = GradLanding.claim(land, dy)
    kind, wide = "parts" if parts is not None else "mapped" if dy_map is not None else "dense", None
    if kind == "dense" and plan.padded_last is not None and _loss_grad_inplace():
        # a gradient that already lies in the padded layout of the last conv (the loss writes it so) is read where it is: no
        # widened copy, the rows that were not returned are the zero tail of gcl_aggregate_head
        wide = _wide_in_place(dy, plan.padded_last[0])
        kind = "dense" if wide is None else "wide"
    if kind == "dense":
        dy = _flat3(dy)
    # The Md batch-dependent rows of a row-table first layer's gradient go straight into the compact gradient of
    # _lat_first_layer_bwd, the others (their batch sums are taken from there) to their usual place: every row is written
    # once.  The aggregation's input there is a fresh dense tensor; in a stack of one conv it is the last conv's too, and a
    # form of its own (present rows, wide) goes first.
    one = len(plan.convs) == 1
    F0 = plan.padded_last[0] if one and plan.padded_last is not None else plan.convs[0].Fout
    compact = (plan.convs[0].kind == "tab" and lat.smap is not None and lat.Md > 0 and _compact_store()
               and not (one and (plan.ln == "mapped_skip" or kind == "wide"))
               and hip.aggregate_compact_ok(graph, Layout.dense(plan.B, plan.n, F0), transpose=True))
    return _Incoming(kind, dy, dy_map, parts, wide, compact)


class GCNStackFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, owner, graph, L: int, has_ln: bool, eps: float, out_rows: int, land, lat, split, *params):
        """land: GradLanding or None.  lat: LatSource or None (x is then the encoder output).
        split: GradLanding or None - this stack's OUTPUT is the encoder output whose gradient arrives in two parts (head
        rows from the decoder-input gather, the rest from the mesh side): its backward reads both where they are.
        out_rows > 0: only the first `out_rows` rows are returned (the decoder keeps the grid rows,
        src/models.py:870-872); the slice is part of this Function so that its backward receives the gradient of
        the slice and widens it with ONE pass of gcl_pad_rows (no zero-fill + copy by autograd).
        Everything is decided by plan_gcn_stack before the first launch; the backward reads ctx.plan."""
        enc_shape = None
        if lat is not None and lat.tail is not None:
            # x is the token of an encoder output stored in two parts: the mesh rows are in lat.tail [B, Md + r, D]
            enc_shape, x3 = tuple(x.shape), lat.tail
        else:
            x3 = _flat3(x.detach())
        if lat is not None and not x3.is_contiguous():
            x3 = x3.contiguous()  # x is the encoder output [B, ne, D]; the stack runs on the M mesh rows it is read into
        plan, out_head, present = plan_gcn_stack(Layout.of(x3), enc_shape, x.dim() == 2, [params[2 * k].shape for k in range(L)],
                                                 graph, has_ln, out_rows, land, lat, split, stack_switches())
        B, n = plan.B, plan.n
        if lat is not None:
            GradLanding.expect_tail(lat.landing)  # this Function's backward fills the shared buffer's tail rows (as MeshLatFn)
        if plan.split_reader:
            split.expect_split_reader()
        if plan.landing:
            land.expect_mapped_reader()
        io = _StackIO(plan, graph, lat, split, out_head, present)
        akind, slope_t = _stack_act(owner, params[2 * L])
        ps, cur = [], x3  # ps: pre-activation outputs of every conv
        for k, st in enumerate(plan.convs):
            if k > 0:
                _expect_dense(cur, B, n, st.Fin)
            act_k, slope_k = (akind, slope_t) if k > 0 else (hip.ACT_NONE, None)
            p, cur = _CONV[st.kind](st, io, cur, act_k, slope_k, params[2 * k].detach(), params[2 * k + 1].detach())
            if st.dense_after:
                p = cur = p.contiguous()
            ps.append(p)
        out, stats = cur, None
        if plan.ln in ("mapped", "mapped_skip"):
            # the rows the decoder-input gather takes go straight into the decoder's input, the others nowhere
            stats = land.ln_write(cur.view(B * n, -1), params[-2].detach(), params[-1].detach(), eps, plan.ln == "mapped_skip")
            out = _token(cur, (B, n, cur.shape[2]))
        elif plan.ln == "dense":
            o2, stats = hip.layernorm_fwd(cur.view(B * n, -1), params[-2].detach(), params[-1].detach(), eps)
            out = o2.view(B, n, -1)
        ctx.plan, ctx.x3, ctx.ps, ctx.stats, ctx.params, ctx.present = plan, x3, ps, stats, params, present
        ctx.owner, ctx.graph, ctx.lat = owner, graph, lat
        ctx.land, ctx.split = (land if plan.landing else None), (split if plan.split_reader else None)
        if plan.out_rows:
            out = out[:, :plan.out_rows, :]
        return out[0] if plan.squeeze else out

    @staticmethod
    def backward(ctx, dy):
        plan, params, graph, ps = ctx.plan, ctx.params, ctx.graph, ctx.ps
        L, B, n, pad = len(plan.convs), plan.B, plan.n, plan.padded_last
        G = _Grads(list(params), list(ctx.needs_input_grad[10:]))
        g = _incoming_grad(plan, ctx.split, ctx.land, ctx.lat, graph, dy)
        b_src = dy3 = g.dy  # b_src: what the last conv's bias gradient sums - without a LayerNorm, the rows that were returned
        if plan.out_rows and pad is None:
            dy3 = hip.pad_rows(dy3, n, dy3.shape[2])  # rows that were not returned carry a zero gradient
        Fo = plan.convs[-1].Fout
        bi_last = 2 * L - 1
        cs = None
        if plan.ln is not None:
            gi, bi = len(params) - 2, len(params) - 1
            dgam = G.dst[gi] if G.dst[gi] is not None else torch.zeros_like(params[gi])
            dbet = G.dst[bi] if G.dst[bi] is not None else torch.zeros_like(params[bi])
            # the LayerNorm backward also sums its dx over the rows: that IS the bias gradient of the last conv
            cs = G.dst[bi_last] if plan.ln_colsum else None
            if plan.ln == "mapped_skip" and g.kind != "mapped":
                raise RuntimeError("the processor's output received a gradient from outside the decoder-input gather, but its "
                                   "dropped rows were not kept (set GCL_NO_ROW_SKIP=1 to keep them)")
            dp = hip.layernorm_bwd(None if g.kind == "mapped" else dy3.view(B * n, -1), ps[-1].view(B * n, -1),
                                   params[gi].detach(), ctx.stats, dgam, dbet, G.acc[gi] and G.acc[bi], colsum_dx=cs,
                                   acc_colsum=bool(cs is not None and G.acc[bi_last]), dy_map=g.dy_map,
                                   skip=plan.ln == "mapped_skip").view(B, n, -1)
            b_src = dp
        elif pad is not None:
            # The last conv ran ldh = roundup(Fout, 4) wide (zero padding columns).  Its gradient is widened to that
            # layout (extra rows / columns 0) in one pass; the dense backward then reads it Fout wide with row stride ldh
            # - the padding columns only ever meet zero weights - so dW / dX need no padded weight copy.
            dp = hip.pad_rows(g.dy, n, pad[0]) if g.kind != "wide" else None
        else:
            dp = dy3  # (with parts: the token - only aggregate_split may read "it", through g.parts)
        if G.dst[bi_last] is not None and cs is None:  # bias of the last conv: its dp comes from outside this stack
            if g.kind == "parts":
                hip.colsum_split(g.parts[0], g.parts[1], G.dst[bi_last], G.acc[bi_last])
            elif g.kind == "wide":  # the same rows, ldh apart (a reshape would copy them)
                hip.colsum(torch.as_strided(g.dy, (B * g.dy.shape[1], Fo), (pad[0], 1), g.dy.storage_offset()), G.dst[bi_last],
                           G.acc[bi_last])
            else:
                hip.colsum(b_src.reshape(-1, Fo), G.dst[bi_last], G.acc[bi_last])
        si = 2 * L
        dsl = G.dst[si] if params[si] is not None else None
        akind, slope_t = _stack_act(ctx.owner, params[si])
        dx = dzc = None
        for k in range(L - 1, -1, -1):
            st, last = plan.convs[k], k == L - 1
            W, wi = params[2 * k].detach(), 2 * k
            inp = ctx.x3 if k == 0 else ps[k - 1]
            inp = inp.view(-1, inp.shape[-1])
            if last and plan.ln == "mapped_skip":
                # the dropped rows of dp were not written: their zeros come from the table
                dh3 = hip.aggregate_present(graph, dp, ctx.present, transpose=True)
            elif last and g.kind == "parts":
                dh3 = hip.aggregate_split(graph, g.parts[0], g.parts[1], transpose=True)
            elif last and g.kind == "wide":
                dh3 = hip.aggregate_head(graph, g.wide, transpose=True)
            elif k == 0 and g.compact:
                _expect_dense(dp, B, n, dp.shape[2], aligned=False)
                dzc = torch.empty(B, ctx.lat.Md + ctx.lat.r, dp.shape[2], dtype=torch.float32, device=dp.device)
                dh3 = hip.aggregate_compact(graph, dp, ctx.lat.smap, dzc, transpose=True)
            else:
                dh3 = hip.aggregate(graph, dp, None, transpose=True)
            dh2 = dh3.view(B * n, -1)
            if last and pad is not None:
                dh2 = dh2[:, :Fo]  # [rows, Fout] view with row stride ldh
            dW = G.dst[wi] if G.dst[wi] is not None else torch.zeros_like(params[wi])
            if k > 0:
                # one fused launch: dp_{k-1} (with PReLU'), dW_k, d(slope) and the bias gradient of
                # conv k-1 (= column sums of dp_{k-1}), which accumulates by ITS parameter's state
                dp = hip.linear_bwd_all(dh2, W, inp, slope_t, dsl, dW, None, G.dst[2 * k - 1], G.acc[wi],
                                        acc_colsum=G.acc[2 * k - 1], act=akind).view(B, n, -1)
            elif st.kind == "tab":
                # with enc_shape the forward read the compact rows themselves (LatSource.tail): x3 IS Pc
                dx = _lat_first_layer_bwd(ctx.lat, None if plan.enc_shape else ctx.x3, dh2.reshape(B, n, -1), W, dW, G.acc[wi],
                                          ctx.needs_input_grad[0], Pc=ctx.x3 if plan.enc_shape else None,
                                          enc_shape=plan.enc_shape, dzc=dzc)
            elif ctx.needs_input_grad[0]:
                dx = hip.linear_bwd_all(dh2, W, inp, None, None, dW, None, None, G.acc[wi],
                                        act=hip.ACT_NONE).view(B, n, -1)
            else:
                hip.linear_bwd_dw(dh2, inp, None, dW, None, G.acc[wi])
        if dx is not None and plan.squeeze:
            dx = dx[0]
        return (dx,) + (None,) * 9 + G.out()


# ------------------------------------------------------------------------------------------------
# GATConv / SparseGATConv layer.  alpha_edges (second output, non-differentiable) is the attention
# of sample 0 in PyG edge order [E', H] - what SparseGATConv thresholds (src/models.py:136-149).
# ------------------------------------------------------------------------------------------------
class GATLayerFn(torch.autograd.Function):
    """One GATConv (with the shared PReLU applied to its input on load)."""

    @staticmethod
    def forward(ctx, x, owner, graph, H: int, want_alpha: bool, act, lat, slope, W, att_src, att_dst, bias):
        """act: kind of the activation applied to x on load (None: PReLU when a slope is given); lat: LatSource or None."""
        squeeze = x.dim() == 2
        tail = lat.tail if lat is not None else None
        x3 = x.detach() if tail is not None else _flat3(x.detach())  # (with a tail x is a token: only its shape is used)
        B, n, _ = x3.shape
        Cc = W.shape[0] // H
        sl = slope.detach() if slope is not None else None
        ctx.lat = ctx.tab = None
        if lat is not None:
            # x is the encoder output [B, ne, D] (LatSource): only its compact mesh rows are transformed, the attention
            # kernels read the transformed rows through the table - no [B, M, D] latents, no [B, M, H*C] transform
            assert sl is None, "a LatSource feeds the first layer of a stack (no input activation)"
            if tail is None and not x3.is_contiguous():
                x3 = x3.contiguous()
            ne, D = x3.shape[1], x3.shape[2]
            nc = lat.Md + lat.r
            # the compact rows: where the encoder stored them, else copied out of its one output tensor
            Pc = tail if tail is not None else \
                hip.copy_rows(x3[:, lat.G:, :], torch.empty(B, nc, D, dtype=torch.float32, device=x3.device))
            h = hip.linear_fwd(Pc.view(B * nc, D), W.detach(), None, None, act=act).view(B, nc, H * Cc)
            ctx.lat, ctx.tab, ctx.enc_shape = lat, lat.compact_tab(ne), x3.shape
            x3 = Pc
            GradLanding.expect_tail(lat.landing)
        else:
            h = hip.linear_fwd(x3.view(B * n, -1), W.detach(), None, sl, act=act).view(B, n, H * Cc)
        ctx.act = act
        y, a_s, a_d, alpha = hip.gat_fwd(graph, h, att_src.detach().reshape(-1), att_dst.detach().reshape(-1),
                                         bias.detach(), H, Cc, tab=ctx.tab)
        alpha_edges = hip.gat_alpha_edge_order(graph, alpha[0], H) if want_alpha else torch.empty(0, device=x3.device)
        ctx.owner, ctx.graph, ctx.H, ctx.Cc, ctx.squeeze = owner, graph, H, Cc, squeeze
        ctx.x3, ctx.h, ctx.a_s, ctx.a_d, ctx.alpha = x3, h, a_s, a_d, alpha
        ctx.params = (slope, W, att_src, att_dst, bias)
        ctx.mark_non_differentiable(alpha_edges)
        return (y[0] if squeeze else y), alpha_edges

    @staticmethod
    def backward(ctx, dy, _dalpha):
        slope, W, att_src, att_dst, bias = ctx.params
        needs = list(ctx.needs_input_grad[7:])
        G = _Grads([slope, W, att_src, att_dst, bias], needs)
        graph, H, Cc = ctx.graph, ctx.H, ctx.Cc
        dy3 = _flat3(dy)
        B, n, _ = dy3.shape
        d_as = G.dst[2] if G.dst[2] is not None else torch.zeros_like(att_src)
        d_ad = G.dst[3] if G.dst[3] is not None else torch.zeros_like(att_dst)
        acc = G.acc[2] and G.acc[3] and (G.dst[4] is None or G.acc[4])
        if not acc:
            # mixed accumulate states: run non-accumulating into temporaries and add
            t_as, t_ad = torch.zeros_like(att_src), torch.zeros_like(att_dst)
            t_b = torch.zeros_like(bias) if G.dst[4] is not None else None
            dh = hip.gat_bwd(graph, dy3, ctx.h, att_src.detach().reshape(-1), att_dst.detach().reshape(-1), ctx.a_s,
                             ctx.a_d, ctx.alpha, t_as.view(-1), t_ad.view(-1), t_b, False, H, Cc, tab=ctx.tab)
            for dst, t, a in ((G.dst[2], t_as, G.acc[2]), (G.dst[3], t_ad, G.acc[3]), (G.dst[4], t_b, G.acc[4])):
                if dst is not None:
                    dst.add_(t) if a else dst.copy_(t)
        else:
            dh = hip.gat_bwd(graph, dy3, ctx.h, att_src.detach().reshape(-1), att_dst.detach().reshape(-1), ctx.a_s,
                             ctx.a_d, ctx.alpha, d_as.view(-1), d_ad.view(-1), G.dst[4], True, H, Cc, tab=ctx.tab)
        if ctx.lat is not None:
            # fold dh [B, M, H*C] back onto the compact rows and run the dense backward there (LatSource)
            dW = G.dst[1] if G.dst[1] is not None else torch.zeros_like(W)
            dx = _lat_first_layer_bwd(ctx.lat, None, dh, W.detach(), dW, G.acc[1], ctx.needs_input_grad[0], Pc=ctx.x3,
                                      enc_shape=tuple(ctx.enc_shape))
            return (dx,) + (None,) * 6 + G.out()
        dh2 = dh.view(B * n, -1)
        inp = ctx.x3.view(B * n, -1)
        sl = slope.detach() if slope is not None else None
        dx = None
        if G.dst[1] is not None and ctx.needs_input_grad[0]:
            # one launch for dx (with the activation's derivative), dW and the slope gradient
            dx = hip.linear_bwd_all(dh2, W.detach(), inp, sl, G.dst[0] if sl is not None else None, G.dst[1], None, None,
                                    G.acc[1], act=ctx.act)
        else:
            if G.dst[1] is not None:
                hip.linear_bwd_dw(dh2, inp, sl, G.dst[1], None, G.acc[1], act=ctx.act)
            if ctx.needs_input_grad[0]:
                dx = hip.linear_bwd_dx(dh2, W.detach(), inp, sl, G.dst[0] if sl is not None else None, act=ctx.act)
        if dx is not None:
            dx = dx.view(B, n, -1)
            if ctx.squeeze:
                dx = dx[0]
        return (dx,) + (None,) * 6 + G.out()


class LayerNormFn(torch.autograd.Function):
    """Node-mode LayerNorm.  Given a GradLanding (the final LayerNorm of a GAT processor inside
    WeatherPrediction.forward) it takes part in the same two channels as GCNStackFn's fused LayerNorm: the output rows
    the decoder reads go straight into the decoder's input, and the backward reads its gradient through the
    decoder-input gather's row map instead of a zero-filled dense tensor."""

    @staticmethod
    def forward(ctx, x, owner, eps, land, gamma, beta):
        x2 = hip.rows2d(x.detach())
        if x.dim() != 3:
            land = None
        ctx.land, ctx.params, ctx.x2 = land, (gamma, beta), x2
        if land is not None:
            land.expect_mapped_reader()
            if land.ln_plan(x.shape[1], x.shape[2], False)[0]:
                ctx.stats = land.ln_write(x2, gamma.detach(), beta.detach(), eps, False)
                return _token(x2, x.shape)
        y, ctx.stats = hip.layernorm_fwd(x2, gamma.detach(), beta.detach(), eps)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        gamma, beta = ctx.params
        G = _Grads([gamma, beta], list(ctx.needs_input_grad[4:]))
        dg = G.dst[0] if G.dst[0] is not None else torch.zeros_like(gamma)
        db = G.dst[1] if G.dst[1] is not None else torch.zeros_like(beta)
        dy, dy_map = GradLanding.claim(ctx.land, dy)
        dx = hip.layernorm_bwd(None if dy_map is not None else hip.rows2d(dy), ctx.x2, gamma.detach(), ctx.stats, dg, db,
                               G.acc[0] and G.acc[1], dy_map=dy_map)
        return (dx.view(dy.shape), None, None, None) + G.out()


class GraphNormFn(torch.autograd.Function):
    """PyG LayerNorm(mode="graph"): statistics over all n*F elements of each sample."""

    @staticmethod
    def forward(ctx, x, owner, eps, gamma, beta):
        squeeze = x.dim() == 2
        x3 = _flat3(x.detach())
        y, stats = hip.graphnorm_fwd(x3, gamma.detach(), beta.detach(), eps)
        ctx.x3, ctx.stats, ctx.params, ctx.eps, ctx.squeeze = x3, stats, (gamma, beta), eps, squeeze
        return y[0] if squeeze else y

    @staticmethod
    def backward(ctx, dy):
        gamma, beta = ctx.params
        G = _Grads([gamma, beta], list(ctx.needs_input_grad[3:]))
        dg = G.dst[0] if G.dst[0] is not None else torch.zeros_like(gamma)
        db = G.dst[1] if G.dst[1] is not None else torch.zeros_like(beta)
        dx = hip.graphnorm_bwd(_flat3(dy), ctx.x3, gamma.detach(), ctx.stats, dg, db, G.acc[0] and G.acc[1], ctx.eps)
        return ((dx[0] if ctx.squeeze else dx), None, None) + G.out()


class MeanAggFn(torch.autograd.Function):
    """SimpleConv(aggr="mean") (src/models.py:414)."""

    @staticmethod
    def forward(ctx, x, graph):
        squeeze = x.dim() == 2
        x3 = _flat3(x.detach())
        ctx.graph, ctx.squeeze = graph, squeeze
        y = hip.aggregate(graph, x3, None)
        return y[0] if squeeze else y

    @staticmethod
    def backward(ctx, dy):
        dx = hip.aggregate(ctx.graph, _flat3(dy), None, transpose=True)
        return (dx[0] if ctx.squeeze else dx), None


class AssembleFn(torch.autograd.Function):
    """`_preprocess_input` (src/models.py:776-806)."""

    @staticmethod
    def forward(ctx, x, grid_static, mesh_static, tail3=None):
        squeeze = x.dim() == 2
        x3 = _flat3(x.detach())
        ctx.squeeze, ctx.G, ctx.Cdyn = squeeze, x3.shape[1], x3.shape[2]
        out = hip.assemble_input(x3, grid_static, mesh_static, tail3)
        return out[0] if squeeze else out

    @staticmethod
    def backward(ctx, dy):
        dy3 = dy if dy.dim() == 3 else dy.unsqueeze(0)
        dx = dy3[:, : ctx.G, : ctx.Cdyn].contiguous()
        return (dx[0] if ctx.squeeze else dx), None, None, None


class WeightedMSEFn(torch.autograd.Function):
    """Residual add + weighted MSE (src/train.py:203-213, 85-102); the gradient with respect to
    the model output is produced by the same kernel that computes the loss."""

    @staticmethod
    def forward(ctx, delta, x_last, y, node_w, chan_w, inv_wsum: float):
        loss, dd, _ = hip.wmse_fwd_bwd(delta.detach(), x_last, y, node_w, chan_w, inv_wsum, 1.0, want_grad=True)
        ctx.dd = dd
        return loss

    @staticmethod
    def backward(ctx, g):
        d = ctx.dd * g
        # pred = x_last + delta: in an autoregressive rollout x_last is the previous step's prediction and
        # carries the same gradient as delta (src/train.py:202-204)
        return d, (d if ctx.needs_input_grad[1] else None), None, None, None, None


class ARStepLossFn(torch.autograd.Function):
    """One autoregressive step of the training loop (src/train.py:203-228) as ONE differentiable unit:
    loss_out = loss_prev + weighted MSE(residual ? x_last + delta : delta, y_step) and, when `advance`, the window
    rolled forward (static channels carried, forcing channels from y).  Forward = gcl_wmse_fwd_bwd + gcl_ar_advance,
    backward = ONE gcl_ar_step_bwd pass producing d_delta and d_state (the upstream loss gradient is read on the
    device): no torch arithmetic, clone, per-channel writes or cat on the differentiated path."""

    @staticmethod
    def forward(ctx, state4, delta3, y3, loss_prev, node_w, chan_w, inv_wsum: float, kinds, residual: bool,
                advance: bool):
        st = state4.detach()
        if not st.is_contiguous():
            st = st.contiguous()
        B, G, obs, Cc = st.shape
        d3 = delta3.detach()
        if d3.stride(2) != 1:
            d3 = d3.contiguous()
        x_last = st[:, :, obs - 1, :] if residual else None
        # delta with rows padded to whole 16 bytes (the decoder's last conv stores 33 / 19 columns 36 / 20 wide): its
        # gradient is born in the same row layout, zero padding columns included, where the decoder's backward reads it
        ctx.inplace = _loss_grad_inplace()
        ldp = (Cc + 3) // 4 * 4
        ctx.ldo = ldp if (ctx.inplace and ldp != Cc and d3.stride(1) == ldp) else None
        loss, dd, _ = hip.wmse_fwd_bwd(d3, x_last, y3, node_w, chan_w, inv_wsum, 1.0, want_grad=True,
                                       loss_prev=loss_prev.detach() if loss_prev is not None else None, ldd_out=ctx.ldo)
        new_state = hip.ar_advance(st, d3, y3, kinds, None, 0, residual) if advance else st.new_empty(0)
        ctx.dd, ctx.kinds, ctx.residual, ctx.advance, ctx.obs, ctx.has_y = dd, kinds, residual, advance, obs, y3 is not None
        if not advance:
            ctx.mark_non_differentiable(new_state)
        return loss, new_state

    @staticmethod
    def backward(ctx, g_loss, g_new):
        g_new = g_new if (ctx.advance and g_new is not None and g_new.numel()) else None
        one = _ONE.get(g_loss.device)
        if (ctx.inplace and g_new is None and not ctx.needs_input_grad[0] and one is not None
                and g_loss.data_ptr() == one.data_ptr()):
            # the upstream gradient is the constant one: dd IS d_delta, no launch (a view, so that nothing adds into dd)
            return None, ctx.dd[..., :ctx.dd.shape[2]], None, (g_loss if ctx.needs_input_grad[3] else None), None, None, None, \
                None, None, None
        d_delta, d_state = hip.ar_step_bwd(ctx.dd, g_loss, g_new, ctx.kinds, ctx.has_y, ctx.residual, ctx.obs,
                                           want_state=ctx.needs_input_grad[0], ldd_out=ctx.ldo)
        return d_state, d_delta, None, (g_loss if ctx.needs_input_grad[3] else None), None, None, None, None, None, None


class Gather2Fn(torch.autograd.Function):
    """Row gather from two sources with precomputed index maps (see hip.gather2_rows).
    maps = (map_a, map_b, inv_a, inv_b): forward maps have length nd; inv_x[j] = destination row
    fed by row j of source x, or -1.  A source with leading dimension 1 is broadcast over the
    batch and receives the batch-summed gradient."""

    @staticmethod
    def forward(ctx, a, b, maps, nd: int, B: int, landing=None):
        map_a, map_b, inv_a, inv_b = maps
        a3 = a.detach()
        ctx.maps, ctx.B, ctx.landing = maps, B, landing
        ctx.sa, ctx.sb = a3.shape, (b.shape if b is not None else None)
        # (asked before a3 is made contiguous: with its head rows already in the buffer, a is a stride-0 token)
        buf = landing.take_decoder_input(a3) if landing is not None else None
        if buf is not None:  # the rows of source b are already in place (b itself is a stride-0 token)
            return buf
        if not a3.is_contiguous():
            a3 = a3.contiguous()
        b3 = b.detach() if b is not None else None
        if b3 is not None and not b3.is_contiguous():
            b3 = b3.contiguous()
        return hip.gather2_rows(a3, map_a, b3, map_b, nd, B)

    @staticmethod
    def backward(ctx, g):
        map_a, map_b, inv_a, inv_b = ctx.maps
        g = g.contiguous()
        da = db = None
        land = ctx.landing
        if ctx.needs_input_grad[0]:
            bc = ctx.sa[0] == 1 and ctx.B > 1
            if land is not None and not bc:
                da = land.head_grad(g, inv_a, ctx.sa, ctx.B)  # the shared buffer with its head rows filled, or None
            if da is None:
                da = hip.gather2_rows(g, inv_a, None, None, ctx.sa[1], ctx.B, sum_batch=bc)
        if ctx.sb is not None and ctx.needs_input_grad[1]:
            bc = ctx.sb[0] == 1 and ctx.B > 1
            if land is not None and not bc:
                db = land.offer(g, inv_b, ctx.sb)  # the token when the consumer reads (g, inv_b) itself, or None
            if db is None:
                db = hip.gather2_rows(g, inv_b, None, None, ctx.sb[1], ctx.B, sum_batch=bc)
        return da, db, None, None, None, None


class GradLanding:
    """The hand-offs of one WeatherPrediction.forward call between the Functions around its processor (`head` = the
    number of grid rows).  The model makes one per call and gives it to MeshLatFn (or the LatSource), to the processor's
    final LayerNorm (GCNStackFn / LayerNormFn) and to the decoder-input gather (Gather2Fn): only those use the encoder output.

    Encoder-output gradient.  The compact encoder output [B, ne, D] has two consumers: the decoder-input gather sends
    gradient only to the first `head` rows, the mesh side (MeshLatFn, or a first processor layer reading through a
    LatSource) only to the rest.  They share one buffer instead of autograd adding two zero-filled tensors:
      forward   mesh side: expect_tail()
      backward  Gather2Fn: head_grad() - fills the head rows and returns the WHOLE buffer to autograd (None when no tail
                writer was announced: the caller gathers densely)
                mesh side (always later: its gradient comes through the processor from the gather): tail() - the buffer,
                to be filled in place from row `head` (its backward then returns None), or (None, 0): write a fresh
                tensor from row 0.  The landing lets go of the buffer here; autograd already owns it.
    Where the producer of the encoder output is a GCN stack that can read a two-part gradient (GCNStackFn `split`: the
    model makes the landing before the encoder runs and hands it in), neither part is copied at all:
      forward   encoder stack: expect_split_reader()
      backward  Gather2Fn: head_grad() keeps the gather's incoming gradient g - its first `head` rows ARE the head rows
                (`head_identity`: inv_a[:head] is the identity) - and returns a stride-0 token
                mesh side: keep_tail(dxc) keeps its compact rows (its backward then returns None)
                encoder stack: claim_parts(dy) - the two parts when `dy` is the token; when something else also sent
                gradient to the encoder output (a hook, the grid latents forward_with_latents returns) autograd has
                summed it with the token into a real tensor, and the parts are copied into one buffer and added to it.

    Processor-output gradient.  The processor's output is consumed by the decoder-input gather alone, so its gradient is
    the gather's incoming gradient seen through a row map; the final LayerNorm's backward reads it that way
    (gcl_layernorm_bwd_map) instead of a zero-filled dense [B, M, D] tensor:
      forward   LayerNorm: expect_mapped_reader()
      backward  Gather2Fn: offer(g, inv_b) - keeps the pair and returns a stride-0 token for autograd to carry (None
                when no reader was announced: the caller gathers densely)
                LayerNorm: claim(dy) - the map, or, when something else also sent gradient to the processor's output (a
                hook, a second consumer: autograd has summed it with the token into a real tensor, so the shortcut
                would drop it), the dense gradient with the gather's share added.  Clears the offer.

    Decoder input (forward).  Nobody sees the processor's output, so its final LayerNorm writes the rows the decoder
    reads straight into the decoder's input [B, head + U, D] and the gather only copies the head rows:
      model      open_decoder_input(), before the processor runs: the buffer, the map mesh row -> row of the buffer (or
                 -1) and, optionally, the mesh rows with a reader as a list (lets the producer skip the others)
      LayerNorm  ln_plan() - does the output go through the map, and are the unread rows skipped? - then ln_write()
      Gather2Fn  take_decoder_input(): the filled buffer with the head rows copied in; a buffer nobody filled is dropped
                 (None: the caller gathers both sources).

    Encoder output (forward).  Inside forward() the encoder output has two readers: the decoder-input gather takes its
    first `head` rows in order (`head_identity`), the mesh side (a LatSource) the rest.  Where the producer is a GCN stack
    whose last conv can store to two destinations (gcl_gcn_layer_fwd_split), each part is written where its reader takes it
    from and the [B, ne, D] tensor never exists:
      model          open_decoder_input() BEFORE the encoder runs, then want_split_out() - once it knows that the mesh side
                     will be a LatSource and that the processor's LayerNorm will fill the decoder's input
      encoder stack  split_out(): the head rows of the decoder's input, or None; after a launch that stored there and
                     in a fresh compact [B, ne - head, D] tensor, keep_split_out(tail).  Its output is then a stride-0
                     token
      model          split_tail(): the compact rows for the LatSource (None: the stack wrote one tensor, today's path)
      Gather2Fn      take_decoder_input() skips its copy (a buffer whose other rows nobody filled is an error: the
                     model asks for the split only when the LayerNorm will fill them)."""

    def __init__(self, head: int, head_identity: bool = False):
        self.head, self.buf, self.mesh_pending = head, None, False
        self.head_identity, self.split_ready, self.part_head, self.part_tail = head_identity, False, None, None
        self.proc_ready, self.proc_src, self.proc_map = False, None, None
        self.dec_buf, self.dec_map, self.dec_rows, self.dec_filled = None, None, None, False
        self.out_wanted, self.out_tail, self.dec_head_placed = False, None, False

    # encoder-output gradient (the static methods take the landing as it reaches their caller: it may be None)
    @staticmethod
    def expect_tail(land):
        if land is not None:
            land.mesh_pending = True

    def expect_split_reader(self):
        self.split_ready = True

    def head_grad(self, g, inv_a, shape, B: int):
        if not self.mesh_pending:
            return None
        if (self.split_ready and self.head_identity and g.dim() == 3 and g.shape[1] >= self.head and g.shape[2] == shape[2]
                and g.shape[2] % 4 == 0 and g.stride(2) == 1 and g.stride(1) % 4 == 0 and g.stride(0) % 4 == 0
                and g.data_ptr() % 16 == 0):  # whole 16-byte rows, as gcl_aggregate_split / gcl_colsum_split need
            self.part_head = g[:, : self.head]
            return _token(g, shape)
        self.buf = torch.empty(shape, dtype=torch.float32, device=g.device)
        hip.gather2_rows(g, inv_a, None, None, self.head, B, out=self.buf[:, : self.head])
        return self.buf

    @staticmethod
    def tail(land):
        if land is None or land.buf is None:
            return None, 0
        buf, land.buf, land.mesh_pending = land.buf, None, False
        return buf, land.head

    @staticmethod
    def keep_tail(land, tail3) -> bool:
        """Mesh side, before tail(): with a two-part reader waiting, keep the compact tail rows [B, ne - head, F] (None: the
        mesh side sends no gradient, the rows are zero) and say so."""
        if land is None or land.part_head is None:
            return False
        land.part_tail, land.mesh_pending = tail3, False
        return True

    @staticmethod
    def claim_parts(land, dy):
        """-> (dy, parts): parts = (head rows, tail rows) when `dy` is the token, else None and `dy` dense (with the
        kept parts added, if any were kept)."""
        if land is None or land.part_head is None:
            return dy, None
        a3, b3 = land.part_head, land.part_tail
        land.part_head = land.part_tail = None
        land.split_ready = False
        if b3 is not None and all(st == 0 for st in dy.stride()):
            return dy, (a3, b3)
        # the old way: one dense buffer (head rows copied, tail rows copied or zero), plus what else arrived
        B, ne, F = dy.shape
        buf = torch.empty(B, ne, F, dtype=torch.float32, device=a3.device) if b3 is not None else \
            torch.zeros(B, ne, F, dtype=torch.float32, device=a3.device)
        hip.copy_rows(a3, buf[:, : land.head])
        if b3 is not None:
            hip.copy_rows(b3, buf[:, land.head:])
        if all(st == 0 for st in dy.stride()):
            return buf, None
        return _flat3(dy) + buf, None

    # processor-output gradient
    def expect_mapped_reader(self):
        self.proc_ready = True

    def offer(self, g, inv_b, shape):
        if not self.proc_ready:
            return None
        self.proc_src, self.proc_map = g, inv_b
        return _token(g, shape)

    @staticmethod
    def claim(land, dy):
        """-> (dy, dy_map): dy_map = (src3, pos) for hip.layernorm_bwd when `dy` is the token, else None and `dy` dense."""
        if land is None or land.proc_src is None:
            return dy, None
        src, pmap = land.proc_src, land.proc_map
        land.proc_src = land.proc_map = None
        land.proc_ready = False
        if all(st == 0 for st in dy.stride()):
            return dy, (src, pmap)
        return _flat3(dy) + hip.gather2_rows(src, pmap, None, None, dy.shape[-2], src.shape[0]), None

    # decoder input
    def open_decoder_input(self, B: int, rows: int, width: int, device, dec_map, dec_rows=None):
        self.dec_buf = torch.empty(B, rows, width, dtype=torch.float32, device=device)
        self.dec_map, self.dec_rows = dec_map, dec_rows

    def ln_plan(self, n: int, F: int, may_skip: bool):
        """For a LayerNorm over n rows per sample, F wide: (mapped?, the `present` table when unread rows are skipped)."""
        if self.dec_buf is None or self.dec_buf.shape[2] != F:
            return False, None
        skip = may_skip and self.dec_rows is not None and self.dec_rows.numel() < n
        return True, (self.dec_map if skip else None)

    def ln_write(self, x2, gamma, beta, eps: float, skip: bool):
        """The mapped LayerNorm of x2 [B * n, F] into the decoder input; returns the row statistics."""
        if skip:
            stats = hip.layernorm_fwd_map_skip(x2, gamma, beta, eps, self.dec_buf, self.dec_map, self.dec_rows)
        else:
            stats = hip.layernorm_fwd_map(x2, gamma, beta, eps, self.dec_buf, self.dec_map)
        self.dec_filled = True
        return stats

    def take_decoder_input(self, a3):
        buf, filled, placed = self.dec_buf, self.dec_filled, self.dec_head_placed
        self.dec_buf, self.dec_filled, self.dec_head_placed = None, False, False
        if placed:  # the encoder's last conv stored the head rows here (a3 is a token)
            if not filled:  # (the model asks for the split only when the LayerNorm will fill the rest)
                raise RuntimeError("the encoder output was stored in two parts, but nothing filled the decoder's mesh rows")
            return buf
        if not filled:
            return None
        hip.copy_rows(a3[:, : self.head, :], buf[:, : self.head, :])
        return buf

    # encoder output
    def want_split_out(self):
        self.out_wanted = True

    def split_out(self, B: int, n: int, F: int):
        """For the stack whose output [B, n, F] is the encoder output: the head rows of the decoder's input to store its
        first `head` rows into (the others go to a compact tensor the stack makes once the kernel has said yes), or None."""
        buf = self.dec_buf
        if not (self.out_wanted and self.head_identity and buf is not None and buf.shape[0] == B and buf.shape[2] == F
                and buf.shape[1] >= self.head and 0 < self.head < n and _split_out()):
            return None
        return buf[:, : self.head]

    def keep_split_out(self, tail):
        self.out_tail, self.dec_head_placed = tail, True

    def split_tail(self):
        tail, self.out_tail = self.out_tail, None
        return tail


class MeshLatFn(torch.autograd.Function):
    """Mesh latents [B, M, D] of the compact pipeline from ONE encoder output [B, n_e, D] whose rows per sample are
    [G grid | Md batch-dependent mesh | r folded batch-invariant mesh rows]: the Mi batch-invariant mesh rows are
    dealt r = ceil(Mi / B) to a sample as isolated nodes, so they ride through the encoder's launches instead of a
    second (B = 1) pass of small launches.  Mesh row i reads enc[b, map_a[i]] (dependent rows) or the flat row
    map_b[i] of enc viewed as [1, B * n_e, D] (folded rows, shared by all samples).
    Backward: rows < G + Md gather g[b, inv_a[j]] (grid rows: 0), folded row j of the flat list gets the batch sum
    of g[:, inv_fold[j]]."""

    @staticmethod
    def forward(ctx, enc, maps, M: int, gmd: int, r: int, landing=None):
        map_a, map_b, inv_a, inv_fold = maps
        e3 = enc.detach()
        if not e3.is_contiguous():
            e3 = e3.contiguous()
        B, ne, D = e3.shape
        ctx.maps, ctx.shape, ctx.gmd, ctx.r, ctx.landing = maps, (B, ne, D), gmd, r, landing
        GradLanding.expect_tail(landing)
        return hip.gather2_rows(e3, map_a, e3.view(1, B * ne, D), map_b, M, B)

    @staticmethod
    def backward(ctx, g):
        _, _, inv_a, inv_fold = ctx.maps
        B, ne, D = ctx.shape
        g = g.contiguous()
        land = ctx.landing
        if land is not None and land.part_head is not None:  # a two-part reader waits: write the tail rows compact
            h = land.head
            t3 = torch.empty(B, ne - h, D, dtype=torch.float32, device=g.device)
            hip.gather2_rows(g, inv_a[h:], None, None, ctx.gmd - h, B, out=t3[:, : ctx.gmd - h])
            _fold_sum(g, inv_fold, ctx.r, B, t3[:, ctx.gmd - h:])
            GradLanding.keep_tail(land, t3)
            return None, None, None, None, None, None
        buf, h = GradLanding.tail(ctx.landing)  # rows below h were written by the decoder-input gather's backward
        out = buf if buf is not None else torch.empty(B, ne, D, dtype=torch.float32, device=g.device)
        hip.gather2_rows(g, inv_a[h:], None, None, ctx.gmd - h, B, out=out[:, h: ctx.gmd])
        _fold_sum(g, inv_fold, ctx.r, B, out[:, ctx.gmd:])  # straight in the tail rows
        return (None if buf is not None else out), None, None, None, None, None


# ------------------------------------------------------------------------------------------------
# InteractionNet processor (src/models.py:166-285): edge encoder + N unshared message-passing steps.
# The first edge-MLP layer on cat([x_s, x_r, e]) is split by operand,
#     hidden = e We^T + (x Ws^T)[senders] + (x Wr^T)[receivers] + b,     [Ws | Wr | We] = edge_mlp[0].weight
# so the per-edge contraction is D wide instead of 3D and the node projections are done once per
# node; same for cat([x, agg]) of the node MLP.  Edges are kept receiver-sorted internally
# (EdgeLayout): the scatter-mean is then a contiguous segment mean and nothing needs atomics.
# params layout: [enc_W, enc_b, slope_enc] + per step [We1, be1, We2, be2, Wn1, bn1, Wn2, bn2, slope,
#                 gamma_e, beta_e, gamma_n, beta_n]   (slope* only for PReLU, gamma/beta only with LN; None otherwise)
# ------------------------------------------------------------------------------------------------
class EdgeLayout:
    """Receiver-sorted view of a reference-layout edge_index [2, E] (+ its sender-sorted transpose)."""

    def __init__(self, edge_index: torch.Tensor, n: int, device):
        ei = edge_index.detach().to("cpu", torch.int64)
        snd, rcv = ei[0], ei[1]
        if ei.numel() and (int(ei.min()) < 0 or int(ei.max()) >= n):
            raise ValueError("edge_index refers to nodes outside [0, n)")
        order = torch.sort(rcv, stable=True).indices            # sorted position -> reference edge id
        self.order = order.to(device)
        snd_s, rcv_s = snd[order], rcv[order]
        cnt = torch.bincount(rcv_s, minlength=n)
        rowptr = torch.zeros(n + 1, dtype=torch.int64)
        rowptr[1:] = torch.cumsum(cnt, 0)
        torder = torch.sort(snd_s, stable=True).indices        # sender-grouped list of sorted positions
        tcnt = torch.bincount(snd_s, minlength=n)
        trowptr = torch.zeros(n + 1, dtype=torch.int64)
        trowptr[1:] = torch.cumsum(tcnt, 0)
        i32 = lambda t: t.to(torch.int32).to(device)
        self.n, self.E = n, int(ei.shape[1])
        self.snd, self.rcv, self.rowptr = i32(snd_s), i32(rcv_s), i32(rowptr)
        self.tperm, self.trowptr = i32(torder), i32(trowptr)
        self.invdeg = (1.0 / cnt.clamp(min=1).to(torch.float32)).to(device)


class InteractionNetFn(torch.autograd.Function):
    PER_STEP = 13

    @staticmethod
    def forward(ctx, x, owner, lay: EdgeLayout, raw_edges, n_steps: int, act: int, use_ln: bool, eps: float, *params):
        squeeze = x.dim() == 2
        x3 = _flat3(x.detach())
        B, n, D = x3.shape
        E = lay.E
        P = [p.detach() if p is not None else None for p in params]
        # ReLU (src/models.py:154-163) runs as a PReLU with the owner's constant zero slope (no slope gradient)
        cs = getattr(owner, "const_slope", None)
        slope_enc = P[2] if P[2] is not None else cs
        e0pre = hip.dense_fwd(raw_edges, P[0], P[1])                       # [E, D]  batch-invariant
        e0 = hip.act_fwd(e0pre, act, slope_enc)
        e = e0.unsqueeze(0) if B == 1 else e0.unsqueeze(0).expand(B, E, D).contiguous()
        saved = []
        xc = x3
        for k in range(n_steps):
            We1, be1, We2, be2, Wn1, bn1, Wn2, bn2, slope, ge, bte, gn, btn = P[3 + 13 * k: 16 + 13 * k]
            slope = slope if slope is not None else cs
            last = k == n_steps - 1
            x2, e2 = xc.view(B * n, D), e.view(B * E, D)
            # edge update
            PS = torch.empty(B, n, 2 * D, dtype=torch.float32, device=x3.device)
            PS2 = PS.view(B * n, 2 * D)
            hip.dense_fwd(x2, We1[:, :D], None, out=PS2[:, :D])
            hip.dense_fwd(x2, We1[:, D:2 * D], None, out=PS2[:, D:])
            H = hip.dense_fwd(e2, We1[:, 2 * D:], be1).view(B, E, D)
            hip.edge_combine(H, None, PS[:, :, :D], lay.snd, None, PS[:, :, D:], lay.rcv, out3=H)
            U = hip.dense_fwd(H.view(B * E, D), We2, be2, act, slope).view(B, E, D)
            agg = hip.segment_reduce(U, None, lay.rowptr, True)
            epre = estats = None
            if not last:  # the edge state after the last step is never read (src/models.py:282-285)
                epre = hip.edge_combine(e, U, None, None, None, None, None, out3=U)  # e + U, in place of U
                if use_ln:
                    e_next, estats = hip.graphnorm_fwd(epre, ge, bte, eps)
                else:
                    e_next = epre
            # node update
            Hn = hip.dense_fwd(x2, Wn1[:, :D], bn1)
            hip.dense_fwd(agg.view(B * n, D), Wn1[:, D:], None, addend=Hn, out=Hn)
            xpre = hip.dense_fwd(Hn, Wn2, bn2, act, slope, addend=x2)
            xstats = None
            if use_ln:
                xn, xstats = hip.layernorm_fwd(xpre, gn, btn, eps)
            else:
                xn = xpre
            saved.append((xc, e, H, agg, epre, estats, Hn, xpre, xstats))
            xc = xn.view(B, n, D)
            if not last:
                e = e_next
        ctx.owner, ctx.lay, ctx.raw, ctx.n_steps, ctx.act, ctx.use_ln, ctx.eps = owner, lay, raw_edges, n_steps, act, use_ln, eps
        ctx.params, ctx.saved, ctx.e0pre, ctx.squeeze, ctx.dims, ctx.cs = params, saved, e0pre, squeeze, (B, n, D, E), cs
        return xc[0] if squeeze else xc

    @staticmethod
    def backward(ctx, dy):
        params, lay, act, use_ln, eps = ctx.params, ctx.lay, ctx.act, ctx.use_ln, ctx.eps
        B, n, D, E = ctx.dims
        needs = list(ctx.needs_input_grad[8:])
        G = _Grads(list(params), needs)
        P = [p.detach() if p is not None else None for p in params]

        def dst(i):  # gradient destination of parameter i (a scratch tensor when not wanted)
            return G.dst[i] if G.dst[i] is not None else (torch.zeros_like(P[i]) if P[i] is not None else None)

        dx = _flat3(dy).view(B * n, D)
        de = None  # gradient wrt the edge state flowing into the step above
        for k in range(ctx.n_steps - 1, -1, -1):
            o = 3 + 13 * k
            We1, be1, We2, be2, Wn1, bn1, Wn2, bn2, slope, ge, bte, gn, btn = P[o: o + 13]
            slope = slope if slope is not None else ctx.cs
            xc, e, H, agg, epre, estats, Hn, xpre, xstats = ctx.saved[k]
            ctx.saved[k] = None
            x2, e2, H2 = xc.view(B * n, D), e.view(B * E, D), H.view(B * E, D)
            dsl = dst(o + 8)
            # node side
            if use_ln:
                dxpre = hip.layernorm_bwd(dx, xpre, gn, xstats, dst(o + 11), dst(o + 12), G.acc[o + 11] and G.acc[o + 12])
            else:
                dxpre = dx
            dHn = hip.dense_bwd_dx(dxpre, Wn2, Hn, act, slope, dsl)
            hip.dense_bwd_dw(dxpre, Hn, dst(o + 6), dst(o + 7), G.acc[o + 6], act, slope)
            dxa = hip.dense_bwd_dx(dHn, Wn1[:, :D], addend=dxpre)
            dagg = hip.dense_bwd_dx(dHn, Wn1[:, D:])
            dWn1 = dst(o + 4)
            hip.dense_bwd_dw(dHn, x2, dWn1[:, :D], dst(o + 5), G.acc[o + 4])
            hip.dense_bwd_dw(dHn, agg.view(B * n, D), dWn1[:, D:], None, G.acc[o + 4])
            # edge side
            depre = None
            if de is not None:
                depre = hip.graphnorm_bwd(de, epre, ge, estats, dst(o + 9), dst(o + 10), G.acc[o + 9] and G.acc[o + 10],
                                          eps) if use_ln else de
            dU = hip.edge_combine(depre, None, dagg.view(B, n, D), lay.rcv, lay.invdeg, None, None)
            dU2 = dU.view(B * E, D)
            dH = hip.dense_bwd_dx(dU2, We2, H2, act, slope, dsl)
            hip.dense_bwd_dw(dU2, H2, dst(o + 2), dst(o + 3), G.acc[o + 2], act, slope)
            dWe1 = dst(o)
            de_in = hip.dense_bwd_dx(dH, We1[:, 2 * D:], addend=depre.view(B * E, D) if depre is not None else None)
            hip.dense_bwd_dw(dH, e2, dWe1[:, 2 * D:], dst(o + 1), G.acc[o])
            dPS = torch.empty(B, n, 2 * D, dtype=torch.float32, device=dH.device)
            dH3 = dH.view(B, E, D)
            hip.segment_reduce(dH3, lay.tperm, lay.trowptr, False, out3=dPS[:, :, :D])
            hip.segment_reduce(dH3, None, lay.rowptr, False, out3=dPS[:, :, D:])
            dPS2 = dPS.view(B * n, 2 * D)
            t = hip.dense_bwd_dx(dPS2[:, :D], We1[:, :D], addend=dxa)
            dx = hip.dense_bwd_dx(dPS2[:, D:], We1[:, D:2 * D], addend=t, out=t)
            hip.dense_bwd_dw(dPS2[:, :D], x2, dWe1[:, :D], None, G.acc[o])
            hip.dense_bwd_dw(dPS2[:, D:], x2, dWe1[:, D:2 * D], None, G.acc[o])
            de = de_in.view(B, E, D)
        # edge encoder (batch-invariant: its gradient is the sum over samples)
        de0 = de[0] if B == 1 else de.sum(dim=0)
        de0pre = hip.act_bwd(ctx.e0pre, de0.contiguous(), act, P[2] if P[2] is not None else ctx.cs, dst(2))
        hip.dense_bwd_dw(de0pre, ctx.raw, dst(0), dst(1), G.acc[0])
        gx = None
        if ctx.needs_input_grad[0]:
            gx = dx.view(B, n, D)
            gx = gx[0] if ctx.squeeze else gx
        return (gx, None, None, None, None, None, None, None) + G.out()
