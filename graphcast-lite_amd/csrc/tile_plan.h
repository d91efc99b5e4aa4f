// Host-side dispatch plans of the graph kernels (aggregate.hip, gcn_layer.hip, gat.hip): which kernel takes a call, with
// which grid and how much LDS.  A plan is a plain function of graph scalars, shapes, strides and switches - no data
// pointer, no HIP call - so the `_ok` queries and the launchers read the SAME rule, and tests/dispatch_plan_check.hip
// pins every comparison on a CPU.  What depends on a pointer (16-byte alignment) is checked where the launch is made.
#pragma once
#include <algorithm>

#include "common.h"

namespace gcl {
namespace plan {

// One sample's rows are addressed as base + 32-bit byte offset, the row index travels in 24 bits of a record.
inline bool bytes31_ok(int64_t rows, int64_t ld) { return rows * ld * 4 < (int64_t)1 << 31; }
inline bool offsets32_ok(int64_t rows, int64_t ld) { return bytes31_ok(rows, ld) && ld * 4 < (int64_t)1 << 24 && rows < 1 << 24; }
// Through a row table the offsets are unsigned and span the whole of x: x_rows flat rows, B samples of bsx floats.
inline bool table_offsets_ok(int64_t x_rows, int64_t ld, int64_t B, int64_t bs, int64_t n) {
  return x_rows * ld * 4 < (int64_t)1 << 32 && B * bs * 4 < (int64_t)1 << 32 && x_rows < 1 << 24 && n < 1 << 24 && ld * 4 < (int64_t)1 << 24;
}

// Largest LDS image of a source-tile block: half a CU's LDS, so that at least two blocks share a CU (one stages its
// next tile while the other sums).
constexpr int64_t kImageCap = 80 * 1024;

// Launch geometry of a source-tile kernel: persistent blocks, as many per CU as LDS allows (at most 8), 32 CUs per XCD.
struct TileGeo {
  int64_t lds = 0;    // dynamic LDS bytes: the image of smax + 1 rows (lpr lanes x 16 B each) + extra
  int pieces = 0;     // halo pieces (LDS-DMA instructions) per wave of the fullest tile
  int per_cu = 0;
  unsigned grid = 0;
  bool fits() const { return lds <= kImageCap; }
  int bucket() const { return pieces <= 4 ? 4 : pieces <= 8 ? 8 : pieces <= 16 ? 16 : 32; }  // the kernels' MAXPW constant
};
inline TileGeo tile_geo(const gcl_halo& hl, int lpr, int64_t extra, int bpc = 0) {  // bpc > 0: tuning override of per_cu
  TileGeo t;
  t.lds = (int64_t)(hl.smax + 1) * lpr * 16 + extra;
  t.pieces = (int)cdiv((hl.smax - hl.T) / (64 / lpr), 4);
  t.per_cu = (int)std::min<int64_t>(8, kLdsBytes / t.lds);
  t.grid = (unsigned)(kNumXCD * 32 * (bpc > 0 ? bpc : t.per_cu));
  return t;
}

// ---- aggregation ------------------------------------------------------------------------------------------------
enum class AggForm { kTile, kPerEdge, kRefused };
struct AggCall {
  int32_t transpose;  // bit 0
  int64_t ldh, bsh, ldy, bsy;
  int32_t F;
  bool two_part, store_map;  // gcl_aggregate_split / _head; gcl_aggregate_compact
};
struct AggSwitches { bool halo; int force_t, bpc; };  // GCL_AGG_HALO (per call); GCL_AGG_HALO_T, GCL_AGG_HALO_BPC (tuning)
struct AggPlan {
  AggForm form = AggForm::kPerEdge;
  int lpr = 4;                   // lanes per row
  bool vl = false, vs = false;   // strides allow 16-byte loads / stores (the launcher adds the base pointers)
  const gcl_halo* hl = nullptr;  // kTile: the layout staged (T = 64 first)
  TileGeo geo;
};
inline AggPlan plan_aggregate(const gcl_graph& g, const AggCall& c, const AggSwitches& sw) {
  AggPlan p;
  const int d = c.transpose & 1, lanes = (c.F + 3) / 4;
  const int n_heavy = d ? g.n_theavy : g.n_heavy;
  p.lpr = lanes <= 4 ? 4 : lanes <= 8 ? 8 : lanes <= 16 ? 16 : lanes <= 32 ? 32 : 64;
  // vector loads need 16-B aligned rows and a padded tail (ldh >= roundup(F,4))
  p.vl = c.ldh % 4 == 0 && c.bsh % 4 == 0 && c.ldh >= (c.F + 3) / 4 * 4;
  p.vs = c.ldy % 4 == 0 && c.bsy % 4 == 0 && c.F % 4 == 0;
  // the source tiles stage ONE tensor's rows; the arithmetic is that of agg_kernel<.., EW = 8>; the one-block-per-row
  // kernel of the heavy rows has no store map
  if (p.lpr >= 16 && !c.two_part && p.vl && p.vs && sw.halo && (d ? g.tell_width : g.ell_width) == 8 &&
      offsets32_ok(g.n, c.ldh) && !(c.store_map && n_heavy > 0))
    for (int t = 0; t < 2 && !p.hl; ++t) {
      const gcl_halo& h = g.halo[d][t];
      if (h.T == 0 || (sw.force_t && h.T != sw.force_t)) continue;
      p.geo = tile_geo(h, p.lpr, 0, sw.bpc);
      if (p.geo.fits() && p.geo.pieces <= 32) p.hl = &h;
    }
  p.form = p.hl ? AggForm::kTile : c.store_map ? AggForm::kRefused : AggForm::kPerEdge;  // the store map lives in the source-tile kernel only
  return p;
}

// ---- one-kernel GCNConv layer -----------------------------------------------------------------------------------
enum class GcnForm {
  kTileFirst,        // source tiles, DMA issue up front, staged 16-byte stores (GCL_GCN_HALO_FORM=0)
  kTileInterleaved,  // <= 4 pieces: stores straight from the accumulator, next item's DMA between the k-steps
  kTileTab,          // interleaved, input rows through a row table
  kTilePred,         // interleaved, output-row predicate
  kTileEight,        // 5 .. 8 pieces
  kEdgeX3,           // per-edge kernel, split-operand dense part (8 waves)
  kEdgeFp32,         // per-edge kernel, fp32 operands (12 waves)
  kEdgeMean,         // per-edge kernel of a GCL_GRAPH_MEAN graph
  kRefused
};
inline bool is_tile(GcnForm f) { return f <= GcnForm::kTileEight; }
struct GcnCall {
  int64_t ldx, bsx, ldy;
  int32_t B, Fin, rows_out;
  int64_t x_rows = 0;    // tab: rows of x as one flat list
  bool tab = false;      // gcl_gcn_layer_fwd_tab
  bool present = false;  // gcl_gcn_layer_fwd_present
  bool two_part = false; // gcl_gcn_layer_fwd_split (ldy: the first part's)
};
struct GcnSwitches {
  bool halo, x3, form;    // GCL_GCN_HALO, GCL_X3 && GCL_X3_GCN, GCL_GCN_HALO_FORM (per call)
  int bpc;                // GCL_GCN_HALO_BPC
  bool edge_pipe = true;  // GCL_GCN_EDGE_PIPE (per call): kEdgeX3's waves with few items start without the stagger; no form depends on it
};
struct GcnPlan {
  GcnForm form = GcnForm::kRefused;
  const char* why = "";  // kRefused
  TileGeo geo;
};
inline GcnPlan plan_gcn_layer(const gcl_graph& g, const GcnCall& c, const GcnSwitches& sw) {
  GcnPlan p;
  const int32_t n = g.n;
  const gcl_halo& hl = g.halo[0][0];
  const int64_t stage = (int64_t)2 * std::max(32 * (c.Fin + 2), 2048) * 4;  // the two operand tiles of the dense part
  // Source tiles only where the gather is the bulk of the layer (>= 6 edges per row: the mesh graph has 7.4): on the
  // decoder graph of the 512x256 configs (3.3 edges per row) the per-edge kernel's twelve wave-independent pipelines
  // run 1.6x faster.  Heavy rows (> kHeavy in-edges) have no records in the tile layout (build_halo_host).  The table
  // and the row predicate exist for the interleaved form only.
  auto tile = [&](bool pred) {
    p.geo = tile_geo(hl, 16, stage + (pred ? 512 : 0), sw.bpc);
    return sw.halo && sw.x3 && g.kind == GCL_GRAPH_GCN && g.n_heavy == 0 && hl.T == 64 && p.geo.pieces <= 8 &&
           c.Fin % 16 == 0 && c.Fin > 32 && c.rows_out == n && g.e >= 6 * (int64_t)n && p.geo.fits() &&
           (c.tab ? table_offsets_ok(c.x_rows, c.ldx, c.B, c.bsx, n) : offsets32_ok(n, c.ldx)) && bytes31_ok(n, c.ldy) &&
           !(c.tab && p.geo.pieces > 4) && !(pred && (c.tab || p.geo.pieces > 4 || !sw.form));
  };
  if (c.present && tile(true)) {
    p.form = GcnForm::kTilePred;
  } else if (tile(false)) {
    p.form = c.tab ? GcnForm::kTileTab : p.geo.pieces > 4 ? GcnForm::kTileEight : sw.form ? GcnForm::kTileInterleaved : GcnForm::kTileFirst;
    if (c.two_part) p = {GcnForm::kRefused, "gcn_layer_fwd_split: the source-tile form takes this layer and keeps its one-tensor destination", {}};
  } else if (c.tab) {
    p.why = g.n_heavy ? "gcn_layer_fwd_tab: the graph has heavy rows (more than 64 in-edges), which the source-tile form does not compute"
                      : "gcn_layer_fwd_tab: this graph / shape has no source-tile form";
  } else if (const bool x3 = sw.x3 && c.Fin % 16 == 0; c.two_part && !(x3 && g.kind == GCL_GRAPH_GCN)) {
    // the 8-wave split-operand instantiations carry the variant; the 12-wave fp32-operand ones sit at their register limit
    p.why = "gcn_layer_fwd_split: only the split-operand kernel of a GCN graph stores in two parts";
  } else if (!offsets32_ok(n, c.ldx)) {
    p.why = "gcn_layer_fwd: one sample of x must stay below 2 GiB (n, row bytes < 2^24)";
  } else {
    p.form = g.kind == GCL_GRAPH_MEAN ? GcnForm::kEdgeMean : x3 ? GcnForm::kEdgeX3 : GcnForm::kEdgeFp32;
  }
  return p;
}

// ---- one-head GAT -----------------------------------------------------------------------------------------------
enum class GatForm { kTile, kPerEdge };
struct GatPlan {
  GatForm form = GatForm::kPerEdge;
  TileGeo geo;      // forward kernel / backward dst-side kernel (forward layout)
  TileGeo geo_src;  // backward src-side kernel (transposed layout)
};
// One head of 64 or 128 channels on a graph with a tile layout: everything of the layer from one LDS image per tile.
inline bool gat_tile_shape(const gcl_graph& g, int64_t ldh, int32_t H, int32_t C, bool halo_on) {
  return halo_on && g.kind == GCL_GRAPH_GAT && H == 1 && (C == 64 || C == 128) && g.halo[0][0].T == 64 && g.n_heavy == 0 &&
         offsets32_ok(g.n, ldh);
}
inline GatPlan plan_gat_fwd(const gcl_graph& g, int64_t ldh, int32_t H, int32_t C, bool halo_on /*GCL_GAT_HALO, per call*/) {
  GatPlan p;
  if (!gat_tile_shape(g, ldh, H, C, halo_on)) return p;
  const gcl_halo& hf = g.halo[0][0];
  p.geo = tile_geo(hf, C / 4, (int64_t)(hf.smax + 1 + 64) * 4);  // image + one score per image row and own row
  if (p.geo.fits() && p.geo.pieces <= 16) p.form = GatForm::kTile;
  return p;
}
// Both edge passes from LDS images: tile layouts in both directions, dy in 16-byte rows.
inline GatPlan plan_gat_bwd(const gcl_graph& g, int64_t ldh, int64_t lddy, int64_t bsdy, int32_t H, int32_t C, bool halo_on) {
  GatPlan p;
  const gcl_halo &hf = g.halo[0][0], &ht = g.halo[1][0];
  if (!gat_tile_shape(g, ldh, H, C, halo_on) || ht.T != 64 || g.n_theavy != 0 || lddy % 4 != 0 || bsdy % 4 != 0 ||
      !offsets32_ok(g.n, lddy))
    return p;
  p.geo = tile_geo(hf, C / 4, (int64_t)(64 + 128 + 8) * 4);  // image + a_s of up to 64 + 128 staged rows
  p.geo_src = tile_geo(ht, C / 4, 0);
  if (hf.smax - 64 <= 128 && p.geo.fits() && p.geo_src.fits() && p.geo.pieces <= 16 && p.geo_src.pieces <= 16) p.form = GatForm::kTile;
  return p;
}

}  // namespace plan
}  // namespace gcl
