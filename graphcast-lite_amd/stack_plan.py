"""What one call of a GCNConv stack (functional.GCNStackFn) does, decided before its first launch.

`plan_gcn_stack` answers every question the forward used to ask between its launches - which kernel runs each conv, where
the output goes, how the LayerNorm writes - and the backward reads the answers instead of working them out again.  It can
do so ahead of time because every tensor between two layers is a fresh allocation whose layout follows from the step
before it: a `Layout` stands in for it when a kernel's gate is asked."""
from dataclasses import dataclass
from typing import NamedTuple, Optional, Tuple

from . import hip


class Switches(NamedTuple):
    """The switches a stack's forward obeys, as functional.stack_switches read them for this call."""
    ln_colsum: bool
    rows_out: bool
    row_skip: bool
    split_grad: bool


class Layout(NamedTuple):
    """Shape, strides and 16-byte alignment of a tensor: all that the gates in hip.py look at."""
    shape: Tuple[int, ...]
    strides: Tuple[int, ...]
    aligned: bool

    @classmethod
    def of(cls, t):
        return cls(tuple(t.shape), tuple(t.stride()), t.data_ptr() % 16 == 0)

    @classmethod
    def dense(cls, B: int, n: int, F: int):
        """A fresh contiguous [B, n, F] allocation."""
        return cls((B, n, F), (n * F, F, 1), True)

    def stride(self, i: int) -> int:
        return self.strides[i]

    def data_ptr(self) -> int:
        return 0 if self.aligned else 4


@dataclass(frozen=True)
class ConvStep:
    kind: str  # tab | split | fused | two_kernel_padded | two_kernel, in this order of preference
    Fin: int
    Fout: int
    ldh: int  # Fout rounded up to whole 16-byte rows
    rows_out: Optional[int] = None  # fused: only the first rows_out rows are computed
    present: bool = False  # fused: only the rows with a reader are stored (the stack's `present` table)
    dense_after: bool = False  # an odd width that feeds another layer / the LayerNorm is copied to dense rows


@dataclass(frozen=True)
class StackPlan:
    convs: Tuple[ConvStep, ...]
    B: int
    n: int
    squeeze: bool
    out_rows: int  # > 0: only that many rows are returned
    ln: Optional[str]  # None | dense | mapped | mapped_skip
    landing: bool  # the LayerNorm's gradient may come through the GradLanding's row map
    split_reader: bool  # the gradient may come in two parts
    padded_last: Optional[Tuple[int, int, bool]]  # the last conv ran ldh wide: (ldh, Fout, with a padded weight copy?)
    enc_shape: Optional[Tuple[int, ...]]  # the first layer read the compact rows of an encoder output of this shape
    ln_colsum: bool  # the LayerNorm backward emits the last conv's bias gradient

    def __post_init__(self):
        # with parts the gradient of the last conv is a token: only gcl_aggregate_split may read "it", so no table of present
        # rows; and a padded last conv's gradient goes straight to it
        assert not (self.split_reader and self.ln is not None) and not (self.padded_last and self.ln is not None)

    @property
    def split_store(self) -> bool:
        return self.convs[-1].kind == "split"


def plan_gcn_stack(x: Layout, enc_shape, squeeze: bool, w_shapes, graph, has_ln: bool, out_rows, land, lat, split, sw: Switches):
    """-> (plan, out_head, present).  x: the layout of the stack's input [B, rows, F]; w_shapes: (Fout, Fin) per conv; the
    rest as GCNStackFn.forward takes them.  out_head (the head rows of the decoder's input, for a `split` last conv) and
    present (the row table of a `mapped_skip` LayerNorm) are the landings' tensors that the answers were read from.  Asks
    the landings, changes nothing."""
    B, n, L = x.shape[0], (lat.M if lat is not None else x.shape[1]), len(w_shapes)
    F_last = w_shapes[-1][0]
    out_rows = int(out_rows) if out_rows and out_rows < n else 0
    # what the two-part reader assumes: the gradient goes straight to the last conv (no LayerNorm, no row slice, no padded
    # width) in whole 16-byte rows; the same conditions let the last conv STORE its output in two parts
    two_part = split is not None and not has_ln and not out_rows and not squeeze and lat is None and F_last % 4 == 0
    out_head = split.split_out(B, n, F_last) if two_part else None
    # The landing serves a stack whose whole LayerNorm output goes to the decoder-input gather: dense, through the row map
    # into the decoder's input (`mapped`), or mapped with the rows that have no reader neither stored nor loaded
    # (`mapped_skip`: the last conv stores only present rows, the LayerNorm pair skips the rest, and the transposed
    # aggregation takes their zero gradient from the table).  Rows are skipped only when every reader of those tensors
    # honours the table: the LayerNorm backward emits the bias gradient's column sums itself and rows are whole 16-byte units.
    landing = land is not None and has_ln and not out_rows and not squeeze
    mapped, present = land.ln_plan(n, F_last, sw.ln_colsum and F_last % 4 == 0 and sw.row_skip) if landing else (False, None)
    ln = None if not has_ln else "mapped_skip" if present is not None else "mapped" if mapped else "dense"
    convs, padded_last, cur = [], None, x
    for k, (Fout, Fin) in enumerate(w_shapes):
        last, ldh = k == L - 1, (Fout + 3) // 4 * 4
        pad = last and ldh != Fout and not has_ln  # stored ldh wide with zero padding columns: 16-byte rows, there and back
        if k == 0 and lat is not None:
            st = ConvStep("tab", Fin, Fout, ldh, dense_after=ldh != Fout)
        elif last and out_head is not None and hip.gcn_layer_split_ok(graph, cur, Fout, out_head):
            st = ConvStep("split", Fin, Fout, ldh)
        elif hip.gcn_layer_fusable(graph, cur, Fin, Fout):
            # the last conv of a stack whose caller keeps only the first rows (decoder: grid rows) computes only those
            st = ConvStep("fused", Fin, Fout, ldh, rows_out=out_rows if last and out_rows and not has_ln and sw.rows_out else None,
                          present=last and present is not None, dense_after=ldh != Fout and not pad)
        else:
            st = ConvStep("two_kernel_padded" if pad else "two_kernel", Fin, Fout, ldh)
        if pad and st.kind in ("fused", "two_kernel_padded"):
            padded_last = (ldh, Fout, st.kind == "two_kernel_padded")
        convs.append(st)
        cur = Layout.dense(B, n, Fout)  # (what every step hands to a next one, once dense_after is applied)
    plan = StackPlan(tuple(convs), B, n, squeeze, out_rows, ln, landing, two_part and sw.split_grad, padded_last, enc_shape,
                     sw.ln_colsum)
    return plan, (out_head if plan.split_store else None), present
