"""Values for the value contract (tests/test_value_contract.py): one non-finite element in an operand and the check
that it comes out only where the arithmetic carries it, power-of-two scalings and the check that a linear kernel
follows them bit for bit, the float64-arbitrated comparison with an fp32 GEMM, and a CPU restatement of the
three-piece bf16 split of csrc/x3.h."""
import math

import torch

from layouts import same_bits

NAN, INF = float("nan"), float("inf")
SCALES = (-48, -24, 24, 48)  # exponents k of the scale covariance cases: operands times 2^k


def poison_rows(rows, per_sample=None):
    """Row 0, a row in the middle of a 64-row tile, the last row; with samples of per_sample rows also the first row of
    sample 1 (where per_sample % 64 != 0 a tile spans two samples there)."""
    out = [0, 64 * ((rows - 1) // 64 // 2) + 31 if rows > 64 else rows // 2, rows - 1]
    if per_sample is not None:
        out.append(per_sample)
    return sorted(set(out))


def poisoned(t, index, value=NAN):
    """A copy of t with `value` at `index`."""
    p = t.clone()
    p[index] = value
    return p


def contained(clean, dirty, ref, what, min_finite=0.5):
    """The three tensors (or lists of them) are the outputs of the clean run, of the poisoned run and of a float64
    restatement of the poisoned run.  The poisoned run is finite exactly where the reference is, and bit-equal to the
    clean run there; at least min_finite of all elements are finite in the reference (else this checks nothing)."""
    if isinstance(ref, torch.Tensor):
        clean, dirty, ref = [clean], [dirty], [ref]
    total = finite = 0
    for i, (c, d, r) in enumerate(zip(clean, dirty, ref)):
        c, d, fin = c.detach().cpu(), d.detach().cpu(), torch.isfinite(r.detach().cpu())
        assert c.shape == d.shape == fin.shape, f"{what}: output {i} has shapes {c.shape}, {d.shape}, {fin.shape}"
        assert bool(torch.isfinite(c).all()), f"{what}: output {i} of the clean run is not finite"
        got = torch.isfinite(d)
        if not torch.equal(got, fin):
            leak, lost = (~got & fin).nonzero(), (got & ~fin).nonzero()
            raise AssertionError(f"{what}: output {i}: {len(leak)} elements non-finite where float64 is finite (first "
                                 f"{leak[:4].tolist()}), {len(lost)} finite where float64 is not (first {lost[:4].tolist()})")
        if not same_bits(d[fin], c[fin]):
            diff = ((d != c) & fin).nonzero()
            raise AssertionError(f"{what}: output {i}: {len(diff)} finite elements differ from the clean run, first "
                                 f"{diff[:4].tolist()}")
        total += fin.numel()
        finite += int(fin.sum())
    assert finite >= min_finite * total, f"{what}: only {finite} of {total} reference elements are finite"
    return finite, total


def covariant(base, scaled, k, what):
    """scaled == base * 2^k bit for bit (tensors or lists of tensors; the product is exact while nothing leaves the
    normal range, which the caller's magnitudes guarantee and this checks)."""
    if isinstance(base, torch.Tensor):
        base, scaled = [base], [scaled]
    f = 2.0 ** k
    for i, (b, s) in enumerate(zip(base, scaled)):
        want = b.detach() * f
        tiny = torch.finfo(torch.float32).tiny
        nz = want != 0
        assert bool(torch.isfinite(want).all()) and bool((want[nz].abs() >= tiny).all()), f"{what}: left the normal range"
        if not same_bits(s.detach(), want):
            bad = (s != want).nonzero()
            j = tuple(bad[0].tolist())
            raise AssertionError(f"{what}: output {i}: {len(bad)} of {want.numel()} elements are not 2^{k} times the unscaled "
                                 f"result; first at {j}: {s[j].item()!r} against {want[j].item()!r}")


def arbitration(got, ref32, ref64):
    """(Frobenius error of got / that of the fp32 GEMM, max error of got / that of the fp32 GEMM) against float64."""
    got, ref32, ref64 = got.detach().cpu().double(), ref32.detach().cpu().double(), ref64.detach().cpu()
    e_hip, e_32 = float((got - ref64).norm()), float((ref32 - ref64).norm())
    m_hip, m_32 = float((got - ref64).abs().max()), float((ref32 - ref64).abs().max())
    return e_hip, e_32, m_hip, m_32


def as_accurate_as_fp32(got, ref32, ref64, what):
    """The rule of test_hip_ops.py::test_x3_linear_fwd_is_as_accurate_as_fp32: the distance to the exact result is at
    most 1.5 x (2 x for the largest element) that of a plain fp32 GEMM, plus rounding noise of 1e-7 of the result."""
    e_hip, e_32, m_hip, m_32 = arbitration(got, ref32, ref64)
    r64 = ref64.detach().cpu()
    print(f"{what}: fro err {e_hip:.3e} (fp32 GEMM {e_32:.3e}), max err {m_hip:.3e} (fp32 GEMM {m_32:.3e})")
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    assert e_hip <= 1.5 * e_32 + 1e-7 * float(r64.norm()), f"{what}: fro err {e_hip:.3e}, fp32 GEMM {e_32:.3e}"
    assert m_hip <= 2.0 * m_32 + 1e-7 * float(r64.abs().max()), f"{what}: max err {m_hip:.3e}, fp32 GEMM {m_32:.3e}"


# ------------------------------------------------------------------------------------------------------------------
# csrc/x3.h split2, restated with torch.bfloat16 (round to nearest even, subnormals kept)
# ------------------------------------------------------------------------------------------------------------------
def split3(x):
    """(hi, mid, lo) of fp32 x as csrc/x3.h forms them: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid), the
    subtractions in fp32."""
    assert x.dtype == torch.float32
    hi = x.to(torch.bfloat16).float()
    r = x - hi
    mid = r.to(torch.bfloat16).float()
    r = r - mid
    lo = r.to(torch.bfloat16).float()
    return hi, mid, lo


def split_is_exact(x):
    """Element-wise: do the three pieces sum to x exactly (in float64, where the sum of three bf16 values is exact)?"""
    hi, mid, lo = split3(x)
    return (hi.double() + mid.double() + lo.double()) == x.double()


def full_significands(e, count=4096, seed=0):
    """fp32 values in [2^e, 2^(e+1)) with random 24-bit significands whose lowest bit is set, both signs."""
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(0, 2 ** 22, (count,), generator=g, dtype=torch.int64) * 2 + 1 + 2 ** 23  # odd, in [2^23, 2^24)
    sign = torch.randint(0, 2, (count,), generator=g, dtype=torch.int64) * 2 - 1
    return (sign * m).double().mul(math.ldexp(1.0, e - 23)).float()
