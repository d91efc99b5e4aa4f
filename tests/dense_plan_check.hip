// Stand-alone check of csrc/dense_plan.h: every comparison of the dense dispatch plans, one case on each side of its edge.
// No data pointer is read and no HIP call is made, so this runs on a CPU (tests/test_dispatch_plan.py builds it with the
// host sanitizers).  The expected values are literals computed with the rules the launchers and the size functions had
// before the plans existed (lin_geom, panel_fits, gt_geom, dw_block, fused_ok, the split-operand applicability tests,
// x3_chain_ok and the three *_ws_bytes functions).  Every dW and fused-backward case also checks its workspace layout:
// sub-buffers inside the byte total, not overlapping, and 16-byte aligned where the 16-byte reducer reads them.
#include <cstdio>
#include <cstring>

#include "../graphcast-lite_amd/csrc/dense_plan.h"

using namespace gcl::plan;

static int g_fail = 0, g_run = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    ++g_run;                                                          \
    if (!(cond)) {                                                    \
      printf("FAIL line %d: %s\n", __LINE__, #cond);                  \
      ++g_fail;                                                       \
    }                                                                 \
  } while (0)

// every switch at its default (nothing is read from the environment), then the named one set to v
static DenseSwitches sw(const char* name, int v) {
  DenseSwitches s;
  s.impl_ = 0; s.x3_ = 1; s.x3_tile_ = 1; s.no_fused_ = 0; s.no_fused64_ = 0; s.chain_ = 1; s.lean_ = 1;
  if (!strcmp(name, "impl")) s.impl_ = v;
  else if (!strcmp(name, "x3")) s.x3_ = v;
  else if (!strcmp(name, "x3_tile")) s.x3_tile_ = v;
  else if (!strcmp(name, "no_fused")) s.no_fused_ = v;
  else if (!strcmp(name, "no_fused64")) s.no_fused64_ = v;
  else if (!strcmp(name, "chain")) s.chain_ = v;
  else if (!strcmp(name, "lean")) s.lean_ = v;
  else if (!strcmp(name, "valu")) s.valu = v != 0;
  else if (!strcmp(name, "gt_mi")) s.gt_mi = v;
  else ++g_fail;
  return s;
}

static bool panel_is(const PanelPlan& p, int NS, int KT, int waves, size_t lds, int grid) {
  return p.valid() && p.NS == NS && p.KT == KT && p.waves == waves && p.lds == lds && p.grid == grid;
}
static bool tile_is(const TilePlan& t, int mi, int nt, int64_t total, int per_xcd, unsigned grid) {
  return t.mi == mi && t.nt == nt && t.total == total && t.per_xcd == per_xcd && t.grid == grid;
}
static bool dx_is(const DensePlan& p, DenseForm form, bool trans, bool first, size_t wt_off, size_t slope_cap) {
  if (p.form != form || p.slope_cap != slope_cap) return false;
  if (form != DenseForm::kTile && form != DenseForm::kTileX3) return true;
  // the transposed copy starts behind the slope partials, 256-byte aligned
  return p.trans == trans && p.transpose_first == first && p.wt_off_bytes == wt_off && wt_off >= slope_cap * 8 && wt_off % 256 == 0 &&
         p.tile_lds == (form == DenseForm::kTileX3 ? 73728u : p.tile.mi == 1 ? 52224u : 69632u);
}
static bool dw_is(const DwPlan& p, int nct, int NC, int NO, size_t lds, int64_t nblk, int64_t rpb, int64_t tile_stride, size_t dbpart_off,
                  size_t bytes, bool may_defer) {
  // layout: `part` holds nct chunks of nblk records, `dbpart` nblk vectors; both inside the total, in this order
  const size_t part_end = p.part_off + (size_t)p.nct * p.tile_stride, db_end = p.dbpart_off + (size_t)p.nblk * p.FoutP;
  const bool layout = part_end <= p.dbpart_off && db_end * 4 <= p.bytes && p.part_off % 4 == 0 && p.dbpart_off % 4 == 0 && p.rec % 4 == 0 &&
                      p.FoutP % 4 == 0 && (!p.may_defer || p.tile_stride % 4 == 0) && p.rec == (int64_t)p.FoutP * p.FinP;
  return layout && p.nct == nct && p.NC == NC && p.NO == NO && p.FinP == NC * 32 && p.FoutP == NO * 32 && p.lds == lds && p.nblk == nblk &&
         p.rpb == rpb && p.tile_stride == tile_stride && p.dbpart_off == dbpart_off && p.bytes == bytes && p.may_defer == may_defer;
}
// lean: ACT * 8 + DB * 4 + CS * 2 + YMASK of a kX3Lean plan, else 0
static bool all_is(const BwdAllPlan& p, BwdAllForm form, int NO, int NC, int nblk, size_t lds, int64_t rec, int db_off, int cs_off,
                   size_t slope_off, int lean) {
  if (p.form != form) return false;
  if (form == BwdAllForm::kSeparate) return true;
  // layout: nblk <= kFusedRecords records [dW | db | colsum], then the slope partials, one double a block
  const bool layout = p.nblk <= kFusedRecords && p.db_off == p.FoP * p.FiP && p.cs_off == p.db_off + p.FoP && p.rec == p.cs_off + p.FiP &&
                      (size_t)kFusedRecords * p.rec * 4 <= p.slope_off_bytes && p.slope_off_bytes + 15 + (size_t)p.nblk * 8 <= p.bytes &&
                      p.rec % 4 == 0 && p.db_off % 4 == 0 && p.cs_off % 4 == 0 && p.slope_off_bytes % 16 == 0;
  const int got = form == BwdAllForm::kX3Lean ? p.ACT * 8 + p.DB * 4 + p.CS * 2 + p.YMASK : 0;
  return layout && p.NO == NO && p.NC == NC && p.FoP == NO * 32 && p.FiP == NC * 32 && p.nblk == nblk && p.lds == lds && p.rec == rec &&
         p.db_off == db_off && p.cs_off == cs_off && p.slope_off_bytes == slope_off && got == lean;
}

static void check_table() {
  // NS 2 / 3 -> 4 / 5 -> 8; KT 64 / 128 / 256
  EXPECT(panel_is(plan_panel(100000, 64, 64, true), 2, 64, 4, 50752, 768));
  EXPECT(panel_is(plan_panel(100000, 64, 96, true), 4, 64, 4, 67648, 256));
  EXPECT(panel_is(plan_panel(100000, 64, 128, true), 4, 64, 4, 67648, 256));
  EXPECT(panel_is(plan_panel(100000, 64, 160, true), 8, 64, 4, 101440, 256));
  EXPECT(panel_is(plan_panel(100000, 65, 64, true), 2, 128, 4, 53824, 512));
  EXPECT(panel_is(plan_panel(100000, 132, 64, true), 2, 256, 4, 102976, 256));
  // the 160 KiB limit: 128-row tiles become 64-row tiles, then nothing fits
  EXPECT(panel_is(plan_panel(100000, 104, 256, true), 8, 128, 4, 162880, 256));
  EXPECT(panel_is(plan_panel(100000, 108, 256, true), 8, 128, 2, 140864, 256));
  EXPECT(!plan_panel(100000, 256, 256, true).valid());  // refused (3)
  EXPECT(panel_is(plan_panel(100, 104, 256, true), 8, 128, 4, 162880, 1));
  // rows without 16-byte alignment: K <= 128
  EXPECT(panel_is(plan_panel(5000, 128, 64, false), 2, 128, 4, 99904, 40));
  EXPECT(!plan_panel(5000, 129, 64, false).valid());  // refused (2)
  EXPECT(!plan_panel(5000, 257, 64, true).valid());  // refused (1)
  EXPECT(!plan_panel(5000, 64, 257, true).valid());  // refused (1)
  EXPECT(panel_is(plan_panel(0, 64, 64, true), 2, 64, 4, 50752, 0));
  // the tile kernel's row tile flips at cdiv(rows, 128) * nt = 6 * kNumCU
  EXPECT(tile_is(plan_tile(196480, 128, sw("gt_mi", 0)), 1, 1, 3070, 384, 768));
  EXPECT(tile_is(plan_tile(196481, 128, sw("gt_mi", 0)), 2, 1, 1536, 192, 512));
  EXPECT(tile_is(plan_tile(98176, 256, sw("gt_mi", 0)), 1, 2, 3068, 384, 768));
  EXPECT(tile_is(plan_tile(98177, 256, sw("gt_mi", 0)), 2, 2, 1536, 192, 512));
  EXPECT(tile_is(plan_tile(196481, 128, sw("gt_mi", 1)), 1, 1, 3071, 384, 768));
  EXPECT(tile_is(plan_tile(1000, 128, sw("gt_mi", 2)), 2, 1, 8, 1, 8));
  EXPECT(tile_is(plan_tile(1000, 132, sw("gt_mi", 0)), 1, 2, 32, 4, 32));
  EXPECT(tile_is(plan_tile(0, 128, sw("gt_mi", 0)), 1, 1, 0, 0, 0));
  // panel or tile: K 128 / 132 at N 128, N 124 / 128 at K 128, GCL_DENSE_IMPL
  EXPECT(plan_dense_fwd({5000, 128, 128, true, true, true}, 128, 128, true, true, 0, sw("impl", 0)).form == DenseForm::kTile);
  EXPECT(plan_dense_fwd({5000, 132, 128, true, true, true}, 132, 128, true, true, 0, sw("impl", 0)).form == DenseForm::kTile);
  EXPECT(plan_dense_fwd({5000, 128, 124, true, true, true}, 128, 124, true, true, 0, sw("impl", 0)).form == DenseForm::kPanel);
  EXPECT(plan_dense_fwd({5000, 124, 128, true, true, true}, 124, 128, true, true, 0, sw("impl", 0)).form == DenseForm::kPanel);
  EXPECT(plan_dense_fwd({5000, 132, 128, true, true, false}, 132, 128, true, true, 0, sw("impl", 0)).form == DenseForm::kPanel);
  EXPECT(dx_is(plan_dense_bwd_dx({5000, 124, 128, true, true, true}, 0, true, sw("impl", 0)), DenseForm::kTile, true, false, 32768, 4096));
  EXPECT(dx_is(plan_dense_bwd_dx({5000, 124, 124, true, true, true}, 0, true, sw("impl", 0)), DenseForm::kPanel, false, false, 0, 4096));
  EXPECT(dx_is(plan_dense_bwd_dx({5000, 132, 128, true, true, true}, 0, true, sw("impl", 0)), DenseForm::kTile, true, false, 32768, 4096));
  EXPECT(plan_dense_fwd({5000, 128, 128, true, true, true}, 128, 128, true, true, 0, sw("impl", 1)).form == DenseForm::kTile);
  EXPECT(plan_dense_fwd({5000, 132, 128, true, true, true}, 132, 128, true, true, 0, sw("impl", 1)).form == DenseForm::kTile);
  EXPECT(plan_dense_fwd({5000, 128, 124, true, true, true}, 128, 124, true, true, 0, sw("impl", 1)).form == DenseForm::kTile);
  EXPECT(plan_dense_fwd({5000, 124, 128, true, true, true}, 124, 128, true, true, 0, sw("impl", 1)).form == DenseForm::kTile);
  EXPECT(plan_dense_fwd({5000, 132, 128, true, true, false}, 132, 128, true, true, 0, sw("impl", 1)).form == DenseForm::kPanel);
  EXPECT(dx_is(plan_dense_bwd_dx({5000, 124, 128, true, true, true}, 0, true, sw("impl", 1)), DenseForm::kTile, true, false, 32768, 4096));
  EXPECT(dx_is(plan_dense_bwd_dx({5000, 124, 124, true, true, true}, 0, true, sw("impl", 1)), DenseForm::kTile, true, false, 32768, 4096));
  EXPECT(dx_is(plan_dense_bwd_dx({5000, 132, 128, true, true, true}, 0, true, sw("impl", 1)), DenseForm::kTile, true, false, 32768, 4096));
  EXPECT(plan_dense_fwd({5000, 128, 128, true, true, true}, 128, 128, true, true, 0, sw("impl", 2)).form == DenseForm::kPanel);
  EXPECT(plan_dense_fwd({5000, 132, 128, true, true, true}, 132, 128, true, true, 0, sw("impl", 2)).form == DenseForm::kPanel);
  EXPECT(plan_dense_fwd({5000, 128, 124, true, true, true}, 128, 124, true, true, 0, sw("impl", 2)).form == DenseForm::kPanel);
  EXPECT(plan_dense_fwd({5000, 124, 128, true, true, true}, 124, 128, true, true, 0, sw("impl", 2)).form == DenseForm::kPanel);
  EXPECT(plan_dense_fwd({5000, 132, 128, true, true, false}, 132, 128, true, true, 0, sw("impl", 2)).form == DenseForm::kPanel);
  EXPECT(dx_is(plan_dense_bwd_dx({5000, 124, 128, true, true, true}, 0, true, sw("impl", 2)), DenseForm::kPanel, false, false, 0, 4096));
  EXPECT(dx_is(plan_dense_bwd_dx({5000, 124, 124, true, true, true}, 0, true, sw("impl", 2)), DenseForm::kPanel, false, false, 0, 4096));
  EXPECT(dx_is(plan_dense_bwd_dx({5000, 132, 128, true, true, true}, 0, true, sw("impl", 2)), DenseForm::kPanel, false, false, 0, 4096));
  // addend / column block of W: tile kernels only; VALU
  EXPECT(plan_dense_fwd({5000, 64, 64, false, true, true}, 64, 64, true, true, 0, sw("impl", 0)).form == DenseForm::kTile);
  EXPECT(plan_dense_fwd({5000, 64, 64, true, true, true}, 64, 64, true, true, 0, sw("valu", 1)).form == DenseForm::kValu);
  EXPECT(plan_dense_fwd({5000, 64, 64, false, true, true}, 64, 64, true, true, 0, sw("valu", 1)).form == DenseForm::kTile);
  EXPECT(dx_is(plan_dense_bwd_dx({5000, 64, 64, true, true, true}, 0, true, sw("valu", 1)), DenseForm::kValu, false, false, 0, 4096));
  // split-operand forward: K, N <= 64, N % 4, 16-byte rows, ld * 4 * 35 < 2^31, GCL_X3
  EXPECT(plan_dense_fwd({5000, 64, 64, true, true, true}, 64, 64, true, true, 1, sw("x3", 1)).form == DenseForm::kX3);
  EXPECT(plan_dense_fwd({5000, 65, 64, true, false, true}, 68, 64, true, true, 1, sw("x3", 1)).form == DenseForm::kPanel);
  EXPECT(plan_dense_fwd({5000, 64, 68, true, true, true}, 64, 68, true, true, 1, sw("x3", 1)).form == DenseForm::kPanel);
  EXPECT(plan_dense_fwd({5000, 64, 62, true, true, true}, 64, 64, true, true, 1, sw("x3", 1)).form == DenseForm::kPanel);
  EXPECT(plan_dense_fwd({5000, 64, 64, true, true, true}, 64, 64, false, true, 1, sw("x3", 1)).form == DenseForm::kPanel);
  EXPECT(plan_dense_fwd({5000, 64, 64, true, true, true}, 64, 64, true, false, 1, sw("x3", 1)).form == DenseForm::kPanel);
  EXPECT(plan_dense_fwd({5000, 64, 64, true, true, true}, 15339168, 64, true, true, 1, sw("x3", 1)).form == DenseForm::kX3);
  EXPECT(plan_dense_fwd({5000, 64, 64, true, true, true}, 15339172, 64, true, true, 1, sw("x3", 1)).form == DenseForm::kPanel);
  EXPECT(plan_dense_fwd({5000, 64, 64, true, true, true}, 64, 15339168, true, true, 2, sw("x3", 1)).form == DenseForm::kX3);
  EXPECT(plan_dense_fwd({5000, 64, 64, true, true, true}, 64, 15339172, true, true, 2, sw("x3", 1)).form == DenseForm::kPanel);
  EXPECT(plan_dense_fwd({5000, 33, 64, true, false, true}, 36, 64, true, true, 0, sw("x3", 1)).form == DenseForm::kX3);
  EXPECT(plan_dense_fwd({5000, 64, 64, true, true, true}, 64, 64, true, true, 1, sw("x3", 0)).form == DenseForm::kPanel);
  // the tile kernels: split-operand form at 128-row tiles, non-transposed weights; GCL_X3, GCL_X3_TILE
  EXPECT(plan_dense_fwd({200000, 256, 256, true, true, true}, 256, 256, true, true, 0, sw("x3", 1)).form == DenseForm::kTileX3);
  EXPECT(plan_dense_fwd({5000, 256, 256, true, true, true}, 256, 256, true, true, 0, sw("x3", 1)).form == DenseForm::kTile);
  EXPECT(plan_dense_fwd({200000, 256, 256, true, true, true}, 256, 256, true, true, 0, sw("x3", 0)).form == DenseForm::kTile);
  EXPECT(plan_dense_fwd({200000, 256, 256, true, true, true}, 256, 256, true, true, 0, sw("x3_tile", 0)).form == DenseForm::kTile);
  // dx: W^T goes to the workspace first from 4096 rows on, when it fits behind the slope partials
  EXPECT(dx_is(plan_dense_bwd_dx({200000, 256, 256, true, true, true}, 294912, true, sw("x3", 1)), DenseForm::kTileX3, false, true, 32768, 4096));
  EXPECT(dx_is(plan_dense_bwd_dx({200000, 256, 256, true, true, true}, 294911, true, sw("x3", 1)), DenseForm::kTile, true, false, 32768, 4096));
  EXPECT(dx_is(plan_dense_bwd_dx({200000, 256, 256, true, true, true}, 294912, false, sw("x3", 1)), DenseForm::kTile, true, false, 32768, 4096));
  EXPECT(dx_is(plan_dense_bwd_dx({200000, 256, 256, true, true, true}, 0, true, sw("x3", 1)), DenseForm::kTile, true, false, 32768, 4096));
  EXPECT(dx_is(plan_dense_bwd_dx({4096, 256, 256, true, true, true}, 294912, true, sw("x3", 1)), DenseForm::kTile, false, true, 32768, 4096));
  EXPECT(dx_is(plan_dense_bwd_dx({4095, 256, 256, true, true, true}, 294912, true, sw("x3", 1)), DenseForm::kTile, true, false, 32768, 4096));
  EXPECT(dx_is(plan_dense_bwd_dx({4096, 258, 256, true, false, true}, 294912, true, sw("x3", 1)), DenseForm::kTile, true, false, 32768, 4096));
  EXPECT(dx_is(plan_dense_bwd_dx({200000, 256, 256, true, true, true}, 294912, true, sw("x3", 0)), DenseForm::kTile, false, true, 32768, 4096));
  // dW: nct 1 / 2 (Fin 128 / 129), the block cap above 80 KiB of LDS, nblk 63 / 64 and nct 3 / 4 for 'may be deferred'
  EXPECT(dw_is(plan_dw(100000, 128, 64, true), 1, 4, 2, 49152, 391, 256, 3203072, 4194304, 16908288, true));
  EXPECT(dw_is(plan_dw(100000, 129, 64, true), 2, 4, 2, 49152, 224, 448, 1835008, 4194304, 16908288, true));
  EXPECT(dw_is(plan_dw(8064, 64, 64, true), 1, 2, 2, 32768, 63, 128, 258048, 2097152, 8519680, false));
  EXPECT(dw_is(plan_dw(8065, 64, 64, true), 1, 2, 2, 32768, 64, 128, 262144, 2097152, 8519680, true));
  EXPECT(dw_is(plan_dw(100000, 384, 64, true), 3, 4, 2, 49152, 157, 640, 1286144, 4194304, 16908288, true));
  EXPECT(dw_is(plan_dw(100000, 385, 64, true), 4, 4, 2, 49152, 121, 832, 991232, 4194304, 16908288, false));
  EXPECT(dw_is(plan_dw(1000000, 96, 256, true), 1, 3, 8, 90112, 253, 3968, 6217728, 12582912, 50855936, true));
  EXPECT(dw_is(plan_dw(1000000, 64, 256, true), 1, 2, 8, 81920, 505, 1984, 8273920, 8388608, 34078720, true));
  EXPECT(dw_is(plan_dw(1000000, 96, 128, true), 1, 3, 4, 57344, 505, 1984, 6205440, 6291456, 25427968, true));
  EXPECT(dw_is(plan_dw(0, 64, 64, true), 1, 2, 2, 32768, 1, 0, 4096, 2097152, 8519680, false));
  EXPECT(dw_is(plan_dw(1, 3, 1, true), 1, 1, 1, 16384, 1, 64, 1024, 524288, 2162688, false));
  EXPECT(dw_is(plan_dw(100000, 33, 65, true), 1, 2, 4, 49152, 391, 256, 3203072, 4194304, 17039360, true));
  EXPECT(dw_is(plan_dw(100000, 97, 129, true), 1, 4, 8, 98304, 224, 448, 7340032, 16777216, 67633152, true));
  EXPECT(dw_is(plan_dw(2000000, 384, 256, true), 3, 4, 8, 98304, 85, 23552, 2785280, 16777216, 67633152, true));
  // sizes: Fout 256 / 257 (wider layers reuse the buffers of a 256-wide launch)
  EXPECT(dense_bwd_ws_bytes(100000, 128, 64, sw("x3", 1)) == 16941056);
  EXPECT(dense_bwd_ws_bytes(100000, 128, 256, sw("x3", 1)) == 67665920);
  EXPECT(dense_bwd_ws_bytes(100000, 128, 257, sw("x3", 1)) == 67665920);
  EXPECT(dense_bwd_ws_bytes(100000, 128, 512, sw("x3", 1)) == 67665920);
  EXPECT(dense_bwd_ws_bytes(2000000, 256, 64, sw("x3", 1)) == 16941056);  // more tile blocks than the VALU cap
  EXPECT(slope_parts_cap(2000000, 256, sw("x3", 1)) == 4096 && slope_parts_cap(1000, 256, sw("x3", 1)) == 4096);
  // whole backward: Fout 64 / 65, Fin 96 / 100, NC == 2, Fin 32 / 36, lddx * 4 * 70 at 2^31, requests, switches
  EXPECT(all_is(plan_bwd_all({100000, 64, 96, 96, 96, 64, true, true, true, true, true, true, false}, sw("x3", 1)), BwdAllForm::kFused128, 2, 3, 256, 108288, 6304, 6144, 6208, 19365888, 0));
  EXPECT(all_is(plan_bwd_all({100000, 68, 96, 96, 96, 65, true, true, true, true, true, true, false}, sw("x3", 1)), BwdAllForm::kSeparate, 0, 0, 0, 0, 0, 0, 0, 0, 0));
  EXPECT(all_is(plan_bwd_all({100000, 64, 100, 100, 100, 64, true, true, true, true, true, true, false}, sw("x3", 1)), BwdAllForm::kSeparate, 0, 0, 0, 0, 0, 0, 0, 0, 0));
  EXPECT(all_is(plan_bwd_all({100000, 64, 32, 32, 32, 64, true, true, true, true, true, true, false}, sw("x3", 1)), BwdAllForm::kFused128, 2, 1, 256, 58624, 2144, 2048, 2112, 6586368, 0));
  EXPECT(all_is(plan_bwd_all({100000, 64, 36, 36, 36, 64, true, true, true, true, true, true, false}, sw("x3", 1)), BwdAllForm::kX3Lean, 2, 2, 512, 65536, 4224, 4096, 4160, 12976128, 12));
  EXPECT(all_is(plan_bwd_all({100000, 32, 64, 64, 64, 32, true, true, true, true, false, false, true}, sw("x3", 1)), BwdAllForm::kX3Lean, 1, 2, 512, 65536, 2144, 2048, 2080, 6586368, 2));
  EXPECT(all_is(plan_bwd_all({100000, 36, 64, 64, 64, 33, true, true, true, true, false, false, false}, sw("x3", 1)), BwdAllForm::kX3Lean, 2, 2, 512, 65536, 4224, 4096, 4160, 12976128, 1));
  EXPECT(all_is(plan_bwd_all({100000, 64, 64, 64, 64, 64, true, true, true, true, true, true, true}, sw("x3", 1)), BwdAllForm::kX3Full, 2, 2, 512, 65536, 4224, 4096, 4160, 12976128, 0));
  EXPECT(all_is(plan_bwd_all({100000, 64, 64, 7669584, 64, 64, true, true, true, true, true, true, false}, sw("x3", 1)), BwdAllForm::kX3Lean, 2, 2, 512, 65536, 4224, 4096, 4160, 12976128, 12));
  EXPECT(all_is(plan_bwd_all({100000, 64, 64, 7669588, 64, 64, true, true, true, true, true, true, false}, sw("x3", 1)), BwdAllForm::kFused64, 2, 2, 768, 50176, 4224, 4096, 4160, 12976128, 0));
  EXPECT(all_is(plan_bwd_all({100000, 64, 64, 64, 64, 64, true, true, false, true, true, true, false}, sw("x3", 1)), BwdAllForm::kFused64, 2, 2, 768, 50176, 4224, 4096, 4160, 12976128, 0));
  EXPECT(all_is(plan_bwd_all({100000, 64, 64, 66, 64, 64, true, true, true, true, true, true, false}, sw("x3", 1)), BwdAllForm::kFused64, 2, 2, 768, 50176, 4224, 4096, 4160, 12976128, 0));
  EXPECT(all_is(plan_bwd_all({100000, 64, 64, 64, 64, 64, false, true, true, true, true, true, false}, sw("x3", 1)), BwdAllForm::kSeparate, 0, 0, 0, 0, 0, 0, 0, 0, 0));
  EXPECT(all_is(plan_bwd_all({100000, 64, 64, 64, 64, 64, true, false, true, true, true, true, false}, sw("x3", 1)), BwdAllForm::kSeparate, 0, 0, 0, 0, 0, 0, 0, 0, 0));
  EXPECT(all_is(plan_bwd_all({100000, 64, 64, 64, 64, 64, true, true, true, false, true, true, false}, sw("x3", 1)), BwdAllForm::kSeparate, 0, 0, 0, 0, 0, 0, 0, 0, 0));
  EXPECT(all_is(plan_bwd_all({100000, 33, 64, 64, 64, 33, true, true, true, true, true, true, false}, sw("x3", 1)), BwdAllForm::kSeparate, 0, 0, 0, 0, 0, 0, 0, 0, 0));
  EXPECT(all_is(plan_bwd_all({100000, 64, 62, 64, 62, 64, true, true, true, true, true, true, false}, sw("x3", 1)), BwdAllForm::kSeparate, 0, 0, 0, 0, 0, 0, 0, 0, 0));
  EXPECT(all_is(plan_bwd_all({0, 64, 64, 64, 64, 64, true, true, true, true, true, true, false}, sw("x3", 1)), BwdAllForm::kSeparate, 0, 0, 0, 0, 0, 0, 0, 0, 0));
  EXPECT(all_is(plan_bwd_all({100, 64, 64, 64, 64, 64, true, true, true, true, true, true, false}, sw("x3", 1)), BwdAllForm::kX3Lean, 2, 2, 2, 65536, 4224, 4096, 4160, 12976128, 12));
  EXPECT(all_is(plan_bwd_all({100000, 64, 96, 96, 96, 32, true, true, true, true, true, true, false}, sw("x3", 1)), BwdAllForm::kFused128, 1, 3, 256, 79616, 3200, 3072, 3104, 9830400, 0));
  EXPECT(all_is(plan_bwd_all({100, 64, 96, 96, 96, 64, true, true, true, true, true, true, false}, sw("x3", 1)), BwdAllForm::kFused128, 2, 3, 1, 108288, 6304, 6144, 6208, 19365888, 0));
  EXPECT(all_is(plan_bwd_all({100000, 64, 64, 64, 64, 64, true, true, true, true, true, true, false}, sw("x3", 0)), BwdAllForm::kFused64, 2, 2, 768, 50176, 4224, 4096, 4160, 12976128, 0));
  EXPECT(all_is(plan_bwd_all({100, 64, 64, 64, 64, 32, true, true, true, true, true, true, false}, sw("x3", 0)), BwdAllForm::kFused64, 1, 2, 2, 33792, 2144, 2048, 2080, 6586368, 0));
  EXPECT(all_is(plan_bwd_all({100000, 64, 64, 64, 64, 64, true, true, true, true, true, true, false}, sw("no_fused", 1)), BwdAllForm::kSeparate, 0, 0, 0, 0, 0, 0, 0, 0, 0));
  EXPECT(all_is(plan_bwd_all({100000, 64, 64, 64, 64, 64, true, true, true, true, true, true, false}, sw("no_fused64", 1)), BwdAllForm::kFused128, 2, 2, 256, 83456, 4224, 4096, 4160, 12976128, 0));
  EXPECT(all_is(plan_bwd_all({100000, 64, 64, 64, 64, 64, true, true, true, true, true, true, false}, sw("lean", 0)), BwdAllForm::kX3Full, 2, 2, 512, 65536, 4224, 4096, 4160, 12976128, 0));
  EXPECT(all_is(plan_bwd_all({100000, 64, 64, 64, 64, 64, true, true, true, true, true, true, false}, sw("valu", 1)), BwdAllForm::kSeparate, 0, 0, 0, 0, 0, 0, 0, 0, 0));
  EXPECT(fused_layout(32, 1).bytes == 3348544);
  EXPECT(fused_layout(32, 33).bytes == 6592576);
  EXPECT(fused_layout(32, 64).bytes == 6592576);
  EXPECT(fused_layout(64, 1).bytes == 6592576);
  EXPECT(fused_layout(64, 33).bytes == 12982336);
  EXPECT(fused_layout(64, 64).bytes == 12982336);
  EXPECT(fused_layout(96, 1).bytes == 9836608);
  EXPECT(fused_layout(96, 33).bytes == 19372096);
  EXPECT(fused_layout(96, 64).bytes == 19372096);
}

static void check_x3_fwd() {
  // <NS, SILU, NKS> and the grid of two blocks a CU
  X3FwdPlan p = plan_x3_fwd(100000, 64, 64, true, true, 64, 64, 1, sw("x3", 1));
  EXPECT(p.ok && p.NS == 2 && p.NKS == 4 && !p.SILU && p.grid == 512 && p.lds == 55296);
  p = plan_x3_fwd(1000, 32, 32, true, true, 32, 32, 2, sw("x3", 1));
  EXPECT(p.ok && p.NS == 1 && p.NKS == 2 && p.SILU && p.grid == 8);
  p = plan_x3_fwd(1000, 36, 36, true, true, 33, 36, 0, sw("x3", 1));
  EXPECT(p.ok && p.NS == 2 && p.NKS == 4);
  EXPECT(!plan_x3_fwd(1000, 64, 64, true, true, 64, 64, 3, sw("x3", 1)).ok);  // unknown activation
  EXPECT(!plan_x3_fwd(1000, 64, 64, true, true, 0, 64, 0, sw("x3", 1)).ok && !plan_x3_fwd(1000, 64, 64, true, true, 64, 0, 0, sw("x3", 1)).ok);
  EXPECT(!plan_x3_fwd(1000, 66, 64, true, true, 64, 64, 0, sw("x3", 1)).ok && !plan_x3_fwd(1000, 64, 66, true, true, 64, 64, 0, sw("x3", 1)).ok);
}

// a run of L 64-wide layers on contiguous rows, PReLU in front, everything present and aligned
static ChainCall chain(int L) {
  ChainCall c{};
  c.ldx = 64; c.rows = 100000; c.K = 64; c.act0 = 1; c.L = L; c.has_x = c.x_al = true;
  for (int k = 0; k < 3; ++k) { c.has_z[k] = c.z_al[k] = true; c.ldz[k] = c.N[k] = 64; }
  c.ldy = 64;
  return c;
}
static ChainCall with_ln(ChainCall c) {
  c.gamma = c.has_y = c.y_al = c.has_stats = c.stats_al8 = true;
  return c;
}
static void check_chain() {
  const DenseSwitches on = sw("chain", 1);
  // chain lengths 1..4; <L, LN>; one block a CU
  EXPECT(!plan_mlp_chain(chain(1), on).ok && !plan_mlp_chain(chain(4), on).ok);
  ChainPlan p = plan_mlp_chain(chain(2), on);
  EXPECT(p.ok && p.L == 2 && !p.LN && p.grid == 256 && p.lds == 55296);
  p = plan_mlp_chain(chain(3), on);
  EXPECT(p.ok && p.L == 3 && !p.LN);
  ChainCall c = chain(2);
  c.rows = 1000;
  EXPECT(plan_mlp_chain(c, on).grid == 8);
  c.rows = -1;
  EXPECT(!plan_mlp_chain(c, on).ok);
  // every layer on <2, false, 4>: widths 33..64
  c = chain(2); c.N[0] = c.ldz[0] = 32; EXPECT(!plan_mlp_chain(c, on).ok);
  c = chain(2); c.K = c.ldx = 32; EXPECT(!plan_mlp_chain(c, on).ok);
  c = chain(2); c.N[0] = c.ldz[0] = 36; c.K = 33; c.ldx = 36; EXPECT(plan_mlp_chain(c, on).ok);
  c = chain(2); c.N[1] = c.ldz[1] = 68; EXPECT(!plan_mlp_chain(c, on).ok);
  c = chain(3); c.N[2] = 62; EXPECT(!plan_mlp_chain(c, on).ok);
  c = chain(2); c.act0 = 2; EXPECT(!plan_mlp_chain(c, on).ok);
  c = chain(2); c.act0 = 0; EXPECT(plan_mlp_chain(c, on).ok);
  // the hand-over is contiguous; the last layer's rows may be padded
  c = chain(2); c.ldz[0] = 68; EXPECT(!plan_mlp_chain(c, on).ok);
  c = chain(2); c.ldz[1] = 68; EXPECT(plan_mlp_chain(c, on).ok);
  c = chain(3); c.ldz[1] = 68; EXPECT(!plan_mlp_chain(c, on).ok);
  c = chain(2); c.ldx = 60; EXPECT(!plan_mlp_chain(c, on).ok);
  // presence and alignment (the layers of a two-layer run only)
  c = chain(2); c.has_x = false; EXPECT(!plan_mlp_chain(c, on).ok);
  c = chain(2); c.x_al = false; EXPECT(!plan_mlp_chain(c, on).ok);
  c = chain(2); c.has_z[1] = false; EXPECT(!plan_mlp_chain(c, on).ok);
  c = chain(2); c.z_al[0] = false; EXPECT(!plan_mlp_chain(c, on).ok);
  c = chain(2); c.has_z[2] = c.z_al[2] = false; EXPECT(plan_mlp_chain(c, on).ok);
  // the LayerNorm epilogue: L = 2 only, 16-byte rows of y, 8-byte stats, 32-bit offsets inside a tile
  p = plan_mlp_chain(with_ln(chain(2)), on);
  EXPECT(p.ok && p.LN);
  EXPECT(!plan_mlp_chain(with_ln(chain(3)), on).ok);
  c = with_ln(chain(2)); c.ldy = 66; EXPECT(!plan_mlp_chain(c, on).ok);
  c = with_ln(chain(2)); c.ldy = 60; EXPECT(!plan_mlp_chain(c, on).ok);
  c = with_ln(chain(2)); c.y_al = false; EXPECT(!plan_mlp_chain(c, on).ok);
  c = with_ln(chain(2)); c.stats_al8 = false; EXPECT(!plan_mlp_chain(c, on).ok);
  c = with_ln(chain(2)); c.has_y = false; EXPECT(!plan_mlp_chain(c, on).ok);
  c = with_ln(chain(2)); c.has_stats = false; EXPECT(!plan_mlp_chain(c, on).ok);
  c = with_ln(chain(2)); c.ldy = 15339168; EXPECT(plan_mlp_chain(c, on).ok);
  c = with_ln(chain(2)); c.ldy = 15339172; EXPECT(!plan_mlp_chain(c, on).ok);
  // switches
  EXPECT(!plan_mlp_chain(chain(2), sw("chain", 0)).ok && !plan_mlp_chain(chain(2), sw("valu", 1)).ok && !plan_mlp_chain(chain(2), sw("x3", 0)).ok);
}

int main() {
  check_table();
  check_x3_fwd();
  check_chain();
  printf("%d checks, %d failed\n", g_run, g_fail);
  return g_fail ? 1 : 0;
}
