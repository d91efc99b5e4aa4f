// Host-side dispatch plans of the dense kernels (linear.hip, linear_x3.hip, gemm_tile.h): which kernel takes a call, with
// which template constants, grid and LDS, and where its partial records lie in the workspace.  As in tile_plan.h a plan is
// a plain function of shapes, leading dimensions, alignment bits, requested outputs and switches - no data pointer, no HIP
// call - so the launchers, the *_ws_bytes functions and the _ok queries read the SAME rule, and
// tests/dense_plan_check.hip pins every comparison on a CPU.  Pointer alignment enters as a bool (aligned16(p)) because
// here it selects the kernel.  Offsets into a workspace are in floats unless a name says bytes.
#pragma once
#include <algorithm>

#include "common.h"

namespace gcl {
namespace plan {

// ---- switches ---------------------------------------------------------------------------------------------------
// One reader per translation unit fills `valu` and `gt_mi`, which stay cached for the process.  The others are read per
// call (the dispatch tests switch them), and only when a plan consults them: a slot holds -1 until then, so a call asks
// the environment for exactly the switches its path depends on, each at most once.  tests set the slots directly.
struct DenseSwitches {
  bool valu = false;  // GCL_LINEAR_IMPL=valu
  int gt_mi = 0;      // GCL_GT_MI: 1 / 2 force the tile kernel's row tile (experiments)
  mutable int impl_ = -1, x3_ = -1, x3_tile_ = -1, no_fused_ = -1, no_fused64_ = -1, chain_ = -1, lean_ = -1;
  int dense_impl() const {  // GCL_DENSE_IMPL: 0 by measurement, 1 tile, 2 panel
    if (impl_ < 0) impl_ = env_is("GCL_DENSE_IMPL", "tile") ? 1 : env_is("GCL_DENSE_IMPL", "panel") ? 2 : 0;
    return impl_;
  }
  bool x3() const { return on(x3_, "GCL_X3", 1); }
  bool x3_tile() const { return on(x3_tile_, "GCL_X3_TILE", 1); }
  bool no_fused() const { return on(no_fused_, "GCL_NO_FUSED_BWD", 0); }
  bool no_fused64() const { return on(no_fused64_, "GCL_NO_FUSED64", 0); }
  bool chain() const { return on(chain_, "GCL_MLP_CHAIN", 1); }
  bool lean() const { return on(lean_, "GCL_X3_BWD_LEAN", 1); }

 private:
  static bool on(int& slot, const char* name, int dflt) {
    if (slot < 0) slot = env_int(name, dflt) != 0;
    return slot != 0;
  }
};

inline bool below_2_31(int64_t v) { return v < (int64_t)1 << 31; }
inline int round4(int v) { return (v + 3) & ~3; }

// ---- resident-panel kernel (linear_mfma_kernel) -------------------------------------------------------------------
// waves per SIMD the register allocator must leave room for (LDS admits ~3 blocks of 4 waves at
// K,N <= 64; wide panels are LDS-limited to 1-2 blocks anyway)
constexpr int lin_min_waves(int NS, int KT) { return (NS <= 2 && KT <= 64) ? 3 : (NS <= 2 && KT <= 128) ? 2 : 1; }
constexpr int kValuGridCap = 4096;  // grid cap of linear_valu_kernel
constexpr int kPanelPerCu = 3;      // most blocks per CU of the panel kernel: lin_min_waves <= 3 at 4 waves
static_assert(kNumCU * kPanelPerCu <= kValuGridCap, "slope_parts_cap: the VALU cap also has to cover the panel grid");

struct PanelPlan {
  bool range_ok, vec_ok;  // K, N in 1..256; K > 128 needs 16-byte rows
  int NS, KT, waves;      // <NS, EPI, KT, VEC>: NS in {1, 2, 4, 8}, KT in {64, 128, 256}; block = waves * 64
  bool vec;
  size_t lds;
  int grid;
  bool valid() const { return range_ok && vec_ok && lds <= (size_t)kLdsBytes; }
};
inline PanelPlan plan_panel(int64_t rows, int K, int N, bool vec_x) {
  PanelPlan p;
  p.range_ok = K >= 1 && K <= 256 && N >= 1 && N <= 256; p.vec_ok = vec_x || K <= 128; p.vec = vec_x;
  p.NS = (N + 31) / 32;
  if (p.NS == 3) p.NS = 4;
  if (p.NS > 4) p.NS = 8;  // instantiated: 1,2,4,8
  p.KT = K <= 64 ? 64 : K <= 128 ? 128 : 256;
  const int KP = round4(K) + 2;
  auto lds = [&](int tile_rows) { return ((size_t)p.NS * 32 + tile_rows) * KP * sizeof(float) + 64; };
  p.waves = 4;
  p.lds = lds(128);
  if (p.lds > (size_t)kLdsBytes) {  // wide panels: 64-row tiles (2 waves) keep the weight panel resident
    p.waves = 2;
    p.lds = lds(64);
  }
  // persistent grid = what is resident at once (LDS- and register-limited), so no partial last wave
  int bpc = (int)((size_t)kLdsBytes / p.lds);
  bpc = std::max(1, std::min(bpc, lin_min_waves(p.NS, p.KT) * 4 / p.waves));
  p.grid = (int)std::min<int64_t>(cdiv(rows, 32 * p.waves), (int64_t)kNumCU * bpc);
  return p;
}

// ---- 128-column tile kernels (gemm_tile_kernel, gemm_tile_x3_kernel) -----------------------------------------------
constexpr int kGtTN = 128, kGtKC = 32, kGtKP = kGtKC + 2;
// MI = 32-row MFMA tiles per wave: the block tile is (64*MI) x 128.  MI = 1 (64-row tiles) is used when
// 128-row tiles would leave the persistent grid a short, badly balanced queue (a few hundred tiles).
constexpr size_t gt_lds(int MI) { return (size_t)2 * (64 * MI + kGtTN) * kGtKP * sizeof(float); }
constexpr int kX3KC = 16, kX3RowB = 48;
constexpr size_t gtx3_lds() { return (size_t)2 * 3 * 256 * kX3RowB; }

struct TilePlan { int mi, nt; int64_t total; int per_xcd; unsigned grid; };
inline TilePlan plan_tile(int64_t rows, int N, const DenseSwitches& sw) {
  TilePlan g;
  g.nt = (N + kGtTN - 1) / kGtTN;
  // 128-row tiles unless they would give the 512 persistent blocks fewer than ~3 tiles each
  g.mi = (cdiv(rows, 128) * g.nt < 3 * 2 * kNumCU) ? 1 : 2;
  if (sw.gt_mi == 1 || sw.gt_mi == 2) g.mi = sw.gt_mi;
  const int TM = 64 * g.mi;
  g.total = cdiv(rows, TM) * g.nt;
  // whole row tiles per XCD so that the column tiles of a row tile share an L2
  g.per_xcd = (int)(cdiv(cdiv(rows, TM), kNumXCD) * g.nt);
  // persistent: the resident blocks per CU (LDS-limited: 2 at 128-row tiles, 3 at 64-row tiles)
  const int cap = (g.mi == 1 ? 3 : 2) * kNumCU / kNumXCD;
  g.grid = (unsigned)(std::min(g.per_xcd, cap) * kNumXCD);
  return g;
}

// Slope partials of a dx call: one double per block of whichever kernel runs.  The tile kernels launch
// plan_tile(rows, Fin).grid blocks, the VALU kernel at most kValuGridCap, the panel kernel at most
// kNumCU * kPanelPerCu (below the VALU cap: the static_assert above).
inline size_t slope_parts_cap(int64_t rows, int Fin, const DenseSwitches& sw) {
  return (size_t)std::max<int64_t>(plan_tile(rows, Fin, sw).grid, kValuGridCap);
}

// ---- split-operand forward (linear_x3_fwd_kernel) and the chained MLP forward ----------------------------------------
constexpr size_t kX3FwdLds = 4 * 3 * 32 * 144;                // four 32-row tiles of three 144-byte-row piece images
constexpr size_t kX3BwdLds = 6 * 64 * 128 + 64 * 64 * 4;      // six 64-row piece images + the dX staging tile
inline bool x3_tile_offsets_ok(int64_t ld) { return below_2_31(ld * 4 * 35); }  // 32-bit offsets inside a tile

struct X3FwdPlan {  // <NS, SILU, NKS>: NKS k-steps of 16 (2 for K <= 32, else 4)
  bool ok = false, SILU = false;
  int NS = 0, NKS = 0, grid = 0;
  size_t lds = kX3FwdLds;
};
inline X3FwdPlan plan_x3_fwd(int64_t rows, int64_t ldx, int64_t ldy, bool x_al, bool y_al, int K, int N, int akind,
                             const DenseSwitches& sw) {
  X3FwdPlan p;
  if (!sw.x3()) return p;
  if (K < 1 || K > 64 || N < 4 || N > 64 || (N & 3) || (ldx & 3) || (ldy & 3) || !x_al || !y_al) return p;
  if (!x3_tile_offsets_ok(ldx) || !x3_tile_offsets_ok(ldy)) return p;
  if (akind != kActNone && akind != kActPrelu && akind != kActSilu) return p;
  p.ok = true; p.NS = N > 32 ? 2 : 1; p.NKS = K <= 32 ? 2 : 4; p.SILU = akind == kActSilu;
  p.grid = (int)std::min<int64_t>(cdiv(rows, 128), 2 * kNumCU);
  return p;
}

struct ChainCall {  // gcl_mlp_fwd_chain(_ok) without its pointers: present / aligned bits instead
  int64_t ldx, rows;
  int K, act0, L;
  bool has_x, x_al;
  bool has_z[3], z_al[3];
  int64_t ldz[3];
  int N[3];
  bool gamma, has_y, y_al, has_stats, stats_al8;  // the LayerNorm epilogue (gamma false: none)
  int64_t ldy;
};
struct ChainPlan {  // <L, LN>: (2, false), (2, true), (3, false)
  bool ok = false, LN = false;
  int L = 0, grid = 0;
  size_t lds = kX3FwdLds;
};
inline ChainPlan plan_mlp_chain(const ChainCall& c, const DenseSwitches& sw) {
  ChainPlan p;
  if (!sw.chain()) return p;
  if (sw.valu || c.L < 2 || c.L > 3 || c.rows < 0 || !c.has_x) return p;  // (valu: gcl_dense_fwd takes no matrix-pipe kernel)
  if (c.act0 != kActNone && c.act0 != kActPrelu) return p;
  bool in_al = c.x_al; int64_t ldin = c.ldx; int K = c.K;
  for (int k = 0; k < c.L; ++k) {
    // the layer as gcl_dense_fwd would launch it, and on linear_x3_fwd_kernel<2, false, 4> (widths 33..64)
    if (!c.has_z[k]) return p;
    const X3FwdPlan l = plan_x3_fwd(c.rows, ldin, c.ldz[k], in_al, c.z_al[k], K, c.N[k], k ? kActPrelu : c.act0, sw);
    if (!l.ok || l.NS != 2 || l.NKS != 4 || l.SILU || ldin < K || c.ldz[k] < c.N[k]) return p;
    if (k + 1 < c.L && c.ldz[k] != c.N[k]) return p;  // handed over: contiguous
    in_al = c.z_al[k]; ldin = c.ldz[k]; K = c.N[k];
  }
  if (c.gamma) {  // the epilogue: two-layer runs (with three the kernel would not fit the register file), 16-byte rows
    if (c.L != 2 || !c.has_y || !c.has_stats || (c.ldy & 3) || c.ldy < K || !c.y_al || !c.stats_al8) return p;
    if (!x3_tile_offsets_ok(c.ldy)) return p;
  }
  p.ok = true; p.L = c.L; p.LN = c.gamma;
  p.grid = (int)std::min<int64_t>(cdiv(c.rows, 128), kNumCU);  // one block a CU: the register file holds one wave a SIMD
  return p;
}

// ---- y = act(x) W^T (+ b) (+ addend) and dx = (dy W) act'(z) (+ addend) ----------------------------------------------
enum class DenseForm { kX3, kValu, kPanel, kTile, kTileX3 };
struct DenseCall {
  int64_t rows;
  int K, N;     // contraction length, output width (dx: K = Fout, N = Fin)
  bool plain;   // no addend and the weight is a whole matrix (ldw == Fin): the panel and split-operand kernels' contract
  bool vec_x;   // K % 4 == 0, the operand's ld % 4 == 0 and its base 16-byte aligned
  bool w_ok;    // ldw % 4 == 0 and W 16-byte aligned
};
struct DensePlan {
  DenseForm form;
  X3FwdPlan x3;      // kX3
  PanelPlan panel;   // kPanel
  TilePlan tile;     // kTile, kTileX3
  bool trans = false;  // kTile: <EPI, TRANS, MI>, the weight rows are strided
  size_t tile_lds = 0;
  // dx only
  bool transpose_first = false;  // W^T is written to the workspace, then read k-contiguously (trans = false)
  size_t wt_off_bytes = 0;       // ... at this offset, behind the slope partials
  size_t slope_cap = 0;          // slope partials the workspace must hold (doubles, at offset 0)
};
// does the resident-panel kernel take this shape?  Measured on MI355X (tools/gemm_bench.py): the 128x128
// tile kernel wins once the contraction is long or the output fills its 128 columns.
inline bool panel_fits(const DenseCall& c, bool trans, const PanelPlan& panel, const DenseSwitches& sw) {
  const int impl = sw.dense_impl();
  const bool tile_ok = c.vec_x && c.w_ok && c.K % 4 == 0 && c.N % 4 == 0;
  if (impl == 1 && tile_ok) return false;
  if (impl == 0 && tile_ok && (c.K > 128 || (c.N >= 128 && (c.K >= 128 || trans)))) return false;
  return panel.valid();
}
inline void set_tile(DensePlan& p, int64_t rows, int N, bool trans, const DenseSwitches& sw) {
  p.tile = plan_tile(rows, N, sw);
  p.trans = trans;
  // split-operand bf16 variant (gemm_tile_x3_kernel): non-transposed weights, 128-row tiles
  const bool x3 = sw.x3() && sw.x3_tile() && !trans && p.tile.mi == 2;
  p.form = x3 ? DenseForm::kTileX3 : DenseForm::kTile;
  p.tile_lds = x3 ? gtx3_lds() : gt_lds(p.tile.mi);
}
// x_al / y_al, ldx / ldy, act: what only the split-operand kernel asks about
inline DensePlan plan_dense_fwd(const DenseCall& c, int64_t ldx, int64_t ldy, bool x_al, bool y_al, int act, const DenseSwitches& sw) {
  DensePlan p;
  p.panel = plan_panel(c.rows, c.K, c.N, c.vec_x);
  if (c.plain && !sw.valu && (p.x3 = plan_x3_fwd(c.rows, ldx, ldy, x_al, y_al, c.K, c.N, act, sw)).ok) p.form = DenseForm::kX3;
  else if (c.plain && sw.valu) p.form = DenseForm::kValu;
  else if (c.plain && panel_fits(c, false, p.panel, sw)) p.form = DenseForm::kPanel;
  else set_tile(p, c.rows, c.N, false, sw);
  return p;
}
// ws_bytes: 0 without a workspace; ws_al: it is 16-byte aligned
inline DensePlan plan_dense_bwd_dx(const DenseCall& c, size_t ws_bytes, bool ws_al, const DenseSwitches& sw) {
  DensePlan p;
  const int Fin = c.N, Fout = c.K;
  p.slope_cap = slope_parts_cap(c.rows, Fin, sw);
  p.panel = plan_panel(c.rows, c.K, c.N, c.vec_x);
  // contraction over Fout: "weights" are W^T, i.e. Wl[j=c][k=o] = W[o*ldw + c]
  if (c.plain && sw.valu) p.form = DenseForm::kValu;
  else if (c.plain && panel_fits(c, true, p.panel, sw)) p.form = DenseForm::kPanel;
  else {
    // the tile kernel stages k-contiguous weight rows twice as cheaply as strided ones: transpose W
    // (a few hundred KB) into the workspace first when there is room
    p.wt_off_bytes = (p.slope_cap * sizeof(double) + 255) & ~(size_t)255;
    p.transpose_first = ws_bytes >= p.wt_off_bytes + (size_t)Fin * Fout * sizeof(float) && ws_al && Fout % 4 == 0 && c.rows >= 4096;
    set_tile(p, c.rows, c.N, !p.transpose_first, sw);
  }
  return p;
}

// ---- dW partials (dw_mfma_kernel) ------------------------------------------------------------------------------------
constexpr int kDwRT = 64;  // rows per step
constexpr int kDwBlocks = 512;
struct DwPlan {
  int nct, NC, NO;  // input chunks of 128 columns (grid.y); <NO, NC, VEC>: NO in {1, 2, 4, 8}, NC in 1..4
  bool vec;
  int FinP, FoutP;
  size_t lds;
  int64_t nblk, rpb, tile_stride;  // blocks (grid.x), rows per block, floats between two chunks' records
  int64_t rec;                     // floats per block record of `part`: FoutP * FinP
  size_t part_off = 0, dbpart_off; // `part` [nct][nblk][FoutP][FinP], `dbpart` [nblk][FoutP]
  size_t bytes;                    // both buffers at their capacity of kDwBlocks records
  bool may_defer;                  // one reducer launch for dW, 16-byte granular, 32-bit offsets (the launcher adds the pointers)
};
// One launch: Fout <= 256 (wider layers are walked 256 outputs at a time over the same workspace).
inline DwPlan plan_dw(int64_t rows, int Fin, int Fout, bool vec) {
  DwPlan p;
  p.vec = vec;
  p.nct = (Fin + 127) / 128;
  p.NC = p.nct > 1 ? 4 : (Fin + 31) / 32;  // slabs of the (widest) chunk
  p.NO = (Fout + 31) / 32;
  p.NO = p.NO <= 2 ? p.NO : p.NO <= 4 ? 4 : 8;  // instantiated: 1, 2, 4, 8 (extra slabs are zero)
  p.FinP = p.NC * 32; p.FoutP = p.NO * 32;
  p.lds = (size_t)kDwRT * (p.FoutP + p.FinP) * sizeof(float);
  // one partial tile per block: no more blocks than are resident at once (wide tiles fill the LDS
  // with one block per CU, and their partials are what the reduction then has to read back), and
  // at least four 64-row steps per block so the load pipeline has something to hide under
  const int64_t cap = (p.lds > 80 * 1024 ? kNumCU : kDwBlocks) / p.nct;
  p.nblk = std::max<int64_t>(1, std::min(cdiv(rows, (p.nct > 1 ? 4 : 2) * kDwRT), cap));
  p.rpb = cdiv(cdiv(rows, p.nblk), kDwRT) * kDwRT;
  p.nblk = rows > 0 ? cdiv(rows, p.rpb) : 1;
  p.rec = (int64_t)p.FoutP * p.FinP;
  p.tile_stride = p.nblk * p.rec;
  p.dbpart_off = (size_t)kDwBlocks * p.rec;
  p.bytes = (p.dbpart_off + (size_t)kDwBlocks * p.FoutP) * sizeof(float);
  p.may_defer = p.nct <= 3 && p.nblk >= 64 && p.tile_stride % 4 == 0 && below_2_31(2 * p.tile_stride);
  return p;
}
// gcl_linear_bwd_ws_bytes: the dW buffers of the widest launch plus the slope partials of a dx call
inline size_t dense_bwd_ws_bytes(int64_t rows, int Fin, int Fout, const DenseSwitches& sw) {
  return plan_dw(rows, Fin, std::min(Fout, 256), false).bytes + slope_parts_cap(rows, Fin, sw) * sizeof(double);
}

// ---- whole backward of one layer (gcl_linear_bwd_all) ----------------------------------------------------------------
enum class BwdAllForm { kSeparate, kFused128, kFused64, kX3Full, kX3Lean };
struct BwdAllCall {
  int64_t rows, lddy, ldx, lddx;
  int Fin, Fout;
  bool dy_al, x_al, dx_al, has_dx;
  bool act, want_db, want_cs;  // in_slope given; db / colsum_dx asked for
};
constexpr int kFusedRecords = 3 * kNumCU;  // most blocks of any fused form
struct BwdAllPlan {
  BwdAllForm form = BwdAllForm::kSeparate;
  int NO = 0, NC = 0, FoP = 0, FiP = 0;  // kFused128 <NO, NC>, kFused64 <NO>
  bool ACT = false, DB = false, CS = false, YMASK = false;  // kX3Lean <NO, ACT, DB, CS, YMASK>
  int nblk = 0;
  size_t lds = 0;
  // per-block record [dW tile FoP*FiP | db FoP | colsum FiP]; the slope partials (doubles) follow kFusedRecords records
  int64_t rec = 0;
  int db_off = 0, cs_off = 0;
  size_t slope_off_bytes = 0;
  size_t bytes = 0;
};
// the record layout alone: what gcl_linear_bwd_all_ws_bytes knows of a call
inline BwdAllPlan fused_layout(int Fin, int Fout) {
  BwdAllPlan p;
  p.NO = (Fout + 31) / 32; p.NC = (Fin + 31) / 32;
  p.FoP = p.NO * 32; p.FiP = p.NC * 32;
  p.db_off = p.FoP * p.FiP; p.cs_off = p.db_off + p.FoP;
  p.rec = (int64_t)p.cs_off + p.FiP;
  p.slope_off_bytes = (size_t)kFusedRecords * p.rec * sizeof(float);  // a multiple of 16: rec is one of 32
  p.bytes = p.slope_off_bytes + (size_t)kFusedRecords * sizeof(double) + 64;  // + room to align an odd base
  return p;
}
inline BwdAllPlan plan_bwd_all(const BwdAllCall& c, const DenseSwitches& sw) {
  BwdAllPlan p = fused_layout(c.Fin, c.Fout);
  // Fout need not be a multiple of 4 when the rows of dy are padded to one (lddy >= roundup(Fout, 4)): the 16-byte
  // loads then also fetch the padding columns, which meet zero weight rows (they must hold finite values)
  const bool rows16 = c.lddy >= round4(c.Fout) && c.Fin % 4 == 0 && c.lddy % 4 == 0 && c.ldx % 4 == 0 && c.lddx >= c.Fin &&
                      c.dy_al && c.x_al;
  if (sw.no_fused() || sw.valu || !(c.Fout <= 64 && c.Fin <= 96 && rows16 && c.has_dx) || c.rows == 0) return p;
  const bool use64 = p.NC == 2 && !sw.no_fused64();  // 64-row tiles, 3 blocks per CU
  // split-operand bf16 kernel (x3.h): same partial records, two blocks per CU.  Beyond the fused form's terms it wants
  // Fout >= 1, 16-byte rows of dx and 32-bit store offsets inside a tile
  const bool x3 = use64 && sw.x3() && c.Fout >= 1 && c.lddx % 4 == 0 && c.dx_al && below_2_31(c.lddx * 4 * 70);
  const int TM = use64 ? 64 : 128;
  p.nblk = (int)std::min<int64_t>(cdiv(c.rows, TM), (x3 ? 2 : use64 ? 3 : 1) * kNumCU);
  p.lds = x3 ? kX3BwdLds : ((size_t)p.FiP * (p.FoP + 2) + (size_t)TM * (p.FoP + 2) + (size_t)TM * p.FiP) * sizeof(float);
  p.form = !use64 ? BwdAllForm::kFused128 : !x3 ? BwdAllForm::kFused64 : BwdAllForm::kX3Lean;
  if (x3) {
    // what the caller asked for (the slope gradient comes with the activation).  A call that wants both column sums, db
    // and those of dX, keeps the full kernel whether or not it has an activation: no layer of the models makes such a call
    // (an MLP layer wants db, a GCNConv the column sums of dX), and linear_x3_bwd_kernel stays the kernel of the complete
    // contract.  GCL_X3_BWD_LEAN=0: every call
    if ((c.want_db && c.want_cs) || !sw.lean()) p.form = BwdAllForm::kX3Full;
    p.ACT = c.act; p.DB = c.want_db; p.CS = c.want_cs; p.YMASK = (c.Fout & 3) != 0;
  }
  return p;
}

}  // namespace plan
}  // namespace gcl
