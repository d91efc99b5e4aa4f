"""Row layouts for the kernel contract tests (test_norm_glue, test_dense_layouts, test_sparse_layouts, test_assim_kernels,
test_scoring_kernels, test_map_kernels, test_mos_kernels, test_region_glue_kernels): operands as
views inside buffers the test owns, whose other elements hold a known value - NaN around an input (a kernel that
reads its padding poisons the result), a sentinel around an output (a kernel that writes outside its view changes
it) - plus the element-wise bound check and the launched-kernel queries the tests share."""
import math

import torch

DEV = "cuda:0"
U = 2.0 ** -24  # fp32 unit roundoff
SENT = -7.25  # what an output buffer holds outside the part a kernel may write
NAN = float("nan")


def randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV)


def rand(*shape, seed):
    return torch.rand(*shape, generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV)


def within(got, ref, tol, what):
    """|got - ref| <= tol element-wise (a NaN anywhere fails)."""
    got, ref = got.double(), ref.double()
    tol = torch.as_tensor(tol, dtype=torch.float64, device=ref.device)
    err = (got - ref).abs()
    bad = ~(err <= tol)
    if bad.any():
        ratio = torch.where(bad, (err / tol).nan_to_num(nan=math.inf), torch.full_like(err, -1.0))
        k = int(ratio.flatten().argmax())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; worst at flat index "
                             f"{k}: got {got.flatten()[k].item()!r}, want {ref.flatten()[k].item()!r}, "
                             f"bound {tol.expand_as(err).flatten()[k].item():.3e}")


def same_bits(a, b):
    """Bit-equal, NaN payloads included (torch.equal calls NaN != NaN)."""
    bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
    ia, ib = a.contiguous().view(bits[a.element_size()]), b.contiguous().view(bits[b.element_size()])
    return a.shape == b.shape and ia.dtype == ib.dtype and bool((ia == ib).all())


COLBLOCK_LEAD = 8  # the column block starts at column 4 * 2 of its wider row


def geometry(F, layout, role="in", ld=None):
    """(row stride, offset of the base from the buffer's start, column offset inside the row) of a layout, in floats."""
    F4 = (F + 3) // 4 * 4
    off = lead = 0
    if layout == "contig":
        ld = F
    elif layout == "odd_ld":
        ld = F + 1 if F % 2 == 0 else F + 2
    else:
        if layout == "colblock":
            lead = COLBLOCK_LEAD
        ld = lead + (F4 if layout == "tight" else F4 + 4 if ld is None else ld)
        off = 1 if layout == "offset" or (layout == "mixed" and role == "out") else 0
    assert ld >= lead + F
    return ld, off, lead


class Geom:
    """What the launch code sees of a layout, without a buffer behind it."""

    def __init__(self, F, layout, role="in"):
        self.ld, self.off, _ = geometry(F, layout, role)

    def aligned(self):
        return self.ld % 4 == 0 and self.off == 0


class Rows:
    """A [rows, F] view (or, with B, a [B, rows, F] view) inside a flat buffer, laid out as `layout` says; the rest of
    the buffer holds `fill`.
      contig    row stride F
      pad_1e3   row stride roundup(F, 4) + 4 (16-byte rows), padding 1e3
      pad_nan   the same, padding NaN
      pad_zero  the same, padding zero
      tight     row stride roundup(F, 4): the tightest 16-byte rows (19 floats on rows of 20), padding NaN
      colblock  16-byte rows; the view sits at column offset 8 of rows that are roundup(F, 4) + 4 wider than that:
                `fill` on both sides
      odd_ld    an odd row stride, padding NaN
      offset    16-byte row stride, base one float past a 16-byte boundary (the scalar path), padding NaN
      mixed     inputs as pad_nan, outputs as offset (vector loads, scalar stores)
    `ld` overrides the row stride of the padded layouts.  With B the samples are bs = rows * ld + gap apart, gap > 0
    (8 where rows are 16-byte ones, else 5), and the gap holds `fill`.  `dtype` (float32 unless given) is the element
    type of the buffer; strides and offsets stay in elements."""

    def __init__(self, rows, F, layout, fill, role="in", ld=None, B=None, dtype=torch.float32):
        ld, off, lead = geometry(F, layout, role, ld)
        self.ld = ld
        nb = 1 if B is None else B
        self.bs = rows * ld + (0 if B is None else 8 if ld % 4 == 0 else 5)
        self.buf = torch.full((off + nb * self.bs + 3,), fill, dtype=dtype, device=DEV)
        self.ptr = self.buf.data_ptr() + self.buf.element_size() * (off + lead)  # (an empty view's data_ptr() is 0)
        self.inside = torch.zeros(self.buf.shape, dtype=torch.bool, device=DEV)
        if B is None:
            self.view = self.buf[off:off + rows * ld].view(rows, ld)[:, lead:lead + F]
            self.inside[off:off + rows * ld].view(rows, ld)[:, lead:lead + F] = True
        else:
            self.view = torch.as_strided(self.buf, (B, rows, F), (self.bs, ld, 1), off + lead)
            torch.as_strided(self.inside, (B, rows, F), (self.bs, ld, 1), off + lead).fill_(True)

    @classmethod
    def of(cls, src, layout, fill, role="in", ld=None, dtype=torch.float32):
        """The layout holding a copy of src ([rows, F] or [B, rows, F])."""
        B = src.shape[0] if src.dim() == 3 else None
        r = cls(src.shape[-2], src.shape[-1], layout, fill, role, ld, B, dtype)
        r.view.copy_(src)
        return r

    def untouched(self, fill):
        return bool((self.buf[~self.inside] == fill).all())

    def aligned(self):
        """16-byte rows: what the vector paths of the kernels ask for."""
        return self.ld % 4 == 0 and self.bs % 4 == 0 and self.ptr % 16 == 0


class Guarded:
    """A contiguous tensor of `shape` (for the operands a kernel takes without strides) with eight elements of `fill`
    on either side of it in the same buffer; `init` is copied into it."""

    def __init__(self, shape, dtype=torch.float32, fill=SENT, init=None):
        n = math.prod(shape)
        self.fill = fill
        self.buf = torch.full((n + 16,), fill, dtype=dtype, device=DEV)
        self.view = self.buf[8:8 + n].view(shape)
        if init is not None:
            self.view.copy_(init)

    def untouched(self):
        return bool((self.buf[:8] == self.fill).all()) and bool((self.buf[-8:] == self.fill).all())


class Field4:
    """A [B, G, steps, C] forecast view (unit channel stride) inside a flat buffer holding `fill`: with `pad` the steps
    are C + 2 apart, the rows steps * (C + 2) + 3 and the samples G * that + 5, otherwise the view is dense.  `strides`
    is (bs, gs, ss) in elements, `ptr` the address of element 0 (an empty view's data_ptr() is 0)."""

    def __init__(self, B, G, steps, C, dtype=torch.float32, pad=True, fill=NAN):
        ss = C + 2 if pad else C
        gs = steps * ss + (3 if pad else 0)
        bs = G * gs + (5 if pad else 0)
        lead = 7 if pad else 0
        self.strides, self.fill = (bs, gs, ss), fill
        self.buf = torch.full((lead + B * bs + 3,), fill, dtype=dtype, device=DEV)
        self.ptr = self.buf.data_ptr() + self.buf.element_size() * lead
        self.view = torch.as_strided(self.buf, (B, G, steps, C), (bs, gs, ss, 1), lead)
        self.inside = torch.zeros(self.buf.shape, dtype=torch.bool, device=DEV)
        torch.as_strided(self.inside, (B, G, steps, C), (bs, gs, ss, 1), lead).fill_(True)

    @classmethod
    def of(cls, src, pad=True, fill=NAN):
        r = cls(*src.shape, dtype=src.dtype, pad=pad, fill=fill)
        r.view.copy_(src)
        return r

    def untouched(self):
        rest = self.buf[~self.inside]
        return bool(rest.isnan().all()) if math.isnan(self.fill) else bool((rest == self.fill).all())


class Worst:
    """The worst error / bound ratio per group of checks, for the figures DESIGN.md quotes."""

    def __init__(self, title):
        self.title, self.worst = title, {}

    def within(self, group, got, ref, tol, what):
        """`within`, and remember the largest |got - ref| / tol of the group (0 / 0 counts as 0)."""
        within(got, ref, tol, what)
        got, ref = got.double(), ref.double()
        tol = torch.as_tensor(tol, dtype=torch.float64, device=ref.device)
        ratio = ((got - ref).abs() / tol).nan_to_num(nan=0.0)
        self.worst[group] = max(self.worst.get(group, 0.0), float(ratio.max()) if ratio.numel() else 0.0)

    def exact(self, group):
        self.worst.setdefault(group, 0.0)

    def report(self, *groups):
        for g in groups:
            print(f"[{self.title}] {g}: worst error / bound = {self.worst.get(g, 0.0):.3e}")


def input_fill(layout):
    return {"pad_1e3": 1e3, "pad_zero": 0.0}.get(layout, NAN)


def launched(fn):
    """(result of fn(), names of the GPU kernels it launched)."""
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    names = sorted({e.name for e in prof.events()})
    assert names, "the profiler recorded no kernel"
    return out, names


def has(names, kern):
    return any(kern in n for n in names)


def targs(names, kern):
    """Template argument lists of every launched instance of `kern` (demangled names: `kern<a, b, ..>(...)`)."""
    out = []
    for n in names:
        i = n.find(kern + "<")
        if i < 0:
            continue
        j = k = i + len(kern) + 1
        depth = 1
        while depth:
            depth += {"<": 1, ">": -1}.get(n[k], 0)
            k += 1
        out.append([a.strip() for a in n[j:k - 1].split(",")])
    return out
