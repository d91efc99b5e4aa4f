// Stand-alone check of csrc/tile_plan.h: every comparison of the dispatch plans, one case on each side of its edge.
// Graphs are fabricated from scalar fields only; no data pointer is read and no HIP call is made, so this runs on a
// CPU (tests/test_dispatch_plan.py builds it with the host sanitizers).  The expected forms are written out from the
// conditions the launchers had before the plans existed.  Edges that the 80 KiB image cap makes unreachable through a
// plan (more than 16 / 32 pieces per wave) are pinned on tile_geo itself.
#include <cstdio>
#include <cstring>

#include "../graphcast-lite_amd/csrc/tile_plan.h"

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

// n rows, 7 edges per row, T = 64 layouts of `smax` image rows in both directions
static gcl_graph tile_graph(int32_t n, int32_t kind, int32_t smax) {
  gcl_graph g;
  g.n = n;
  g.e = 7 * (int64_t)n;
  g.kind = kind;
  for (int d = 0; d < 2; ++d) {
    g.halo[d][0].T = 64;
    g.halo[d][0].smax = smax;
    g.halo[d][0].ntiles = (n + 63) / 64;
  }
  return g;
}
static int32_t smax_of(int T, int quads) { return T + 4 * quads; }  // lpr = 16: `quads` = (smax - T) / 4, pieces = cdiv(quads, 4)

constexpr int64_t k2_22 = (int64_t)1 << 22, k2_23 = (int64_t)1 << 23, k2_24 = (int64_t)1 << 24, k2_29 = (int64_t)1 << 29;

static void check_helpers() {
  EXPECT(bytes31_ok(k2_23 - 1, 64) && !bytes31_ok(k2_23, 64));
  EXPECT(offsets32_ok(k2_23 - 1, 64) && !offsets32_ok(k2_23, 64));           // rows * ld * 4 < 2^31
  EXPECT(offsets32_ok(100, k2_22 - 4) && !offsets32_ok(100, k2_22));         // ld * 4 < 2^24
  EXPECT(offsets32_ok(k2_24 - 1, 4) && !offsets32_ok(k2_24, 4));             // rows < 2^24
  EXPECT(table_offsets_ok(k2_23 - 1, 128, 1, 4, 100) && !table_offsets_ok(k2_23, 128, 1, 4, 100));   // x_rows * ld * 4 < 2^32
  EXPECT(table_offsets_ok(100, 64, 2, k2_29 - 4, 100) && !table_offsets_ok(100, 64, 2, k2_29, 100)); // B * bs * 4 < 2^32
  EXPECT(table_offsets_ok(k2_24 - 1, 48, 1, 4, 100) && !table_offsets_ok(k2_24, 48, 1, 4, 100));     // x_rows < 2^24
  EXPECT(table_offsets_ok(100, 64, 1, 4, k2_24 - 1) && !table_offsets_ok(100, 64, 1, 4, k2_24));     // n < 2^24
  EXPECT(table_offsets_ok(100, k2_22 - 4, 1, 4, 100) && !table_offsets_ok(100, k2_22, 1, 4, 100));   // ld * 4 < 2^24
  // pieces per wave and the kernels' MAXPW constant at 4/5, 8/9, 16/17, 32/33
  const int quads[8] = {16, 17, 32, 33, 64, 65, 128, 129}, pieces[8] = {4, 5, 8, 9, 16, 17, 32, 33}, bucket[8] = {4, 8, 8, 16, 16, 32, 32, 32};
  for (int i = 0; i < 8; ++i) {
    gcl_halo h;
    h.T = 64;
    h.smax = smax_of(64, quads[i]);
    const TileGeo t = tile_geo(h, 16, 0);
    EXPECT(t.pieces == pieces[i] && t.bucket() == bucket[i]);
    h.smax = 64 + 2 * quads[i];  // lpr = 32: two rows per wave pass
    EXPECT(tile_geo(h, 32, 0).pieces == pieces[i]);
  }
  gcl_halo h;
  h.T = 64;
  h.smax = 128;
  TileGeo t = tile_geo(h, 16, 0);  // 129 rows x 256 B
  EXPECT(t.lds == 33024 && t.per_cu == 4 && t.grid == 1024 && t.fits());
  EXPECT(tile_geo(h, 16, 0, 2).grid == 512);  // blocks-per-CU override
  h.smax = 64;
  EXPECT(tile_geo(h, 16, 0).per_cu == 8 && tile_geo(h, 16, 0).pieces == 0);  // 9 fit, 8 are used
  h.smax = 319;
  EXPECT(tile_geo(h, 16, 0).lds == kImageCap && tile_geo(h, 16, 0).fits() && !tile_geo(h, 16, 4).fits());
}

static void check_gcn() {
  const GcnSwitches on{true, true, true, 0};
  const int32_t n = 1000;
  auto form = [&](const gcl_graph& g, GcnCall c, GcnSwitches sw = {true, true, true, 0}) { return plan_gcn_layer(g, c, sw).form; };
  auto call = [&](const gcl_graph& g, int32_t Fin = 64) { return GcnCall{Fin, (int64_t)g.n * Fin, 64, 2, Fin, g.n}; };
  auto tab = [&](const gcl_graph& g, int32_t Fin = 64) {
    GcnCall c = call(g, Fin);
    c.x_rows = 2 * (int64_t)g.n;
    c.tab = true;
    return c;
  };
  auto pres = [&](const gcl_graph& g) {
    GcnCall c = call(g);
    c.present = true;
    return c;
  };
  auto two = [&](const gcl_graph& g, int32_t Fin = 64) {
    GcnCall c = call(g, Fin);
    c.two_part = true;
    return c;
  };
  const gcl_graph g4 = tile_graph(n, GCL_GRAPH_GCN, smax_of(64, 16)), g5 = tile_graph(n, GCL_GRAPH_GCN, smax_of(64, 17));
  const gcl_graph g8 = tile_graph(n, GCL_GRAPH_GCN, smax_of(64, 32)), g9 = tile_graph(n, GCL_GRAPH_GCN, smax_of(64, 33));
  // pieces per wave and GCL_GCN_HALO_FORM
  EXPECT(form(g4, call(g4)) == GcnForm::kTileInterleaved);
  EXPECT(form(g4, call(g4), {true, true, false, 0}) == GcnForm::kTileFirst);
  EXPECT(form(g5, call(g5)) == GcnForm::kTileEight && form(g5, call(g5), {true, true, false, 0}) == GcnForm::kTileEight);
  EXPECT(form(g8, call(g8)) == GcnForm::kTileEight);
  EXPECT(form(g9, call(g9)) == GcnForm::kEdgeX3);
  // the row table: interleaved form only
  EXPECT(form(g4, tab(g4)) == GcnForm::kTileTab && form(g4, tab(g4), {true, true, false, 0}) == GcnForm::kTileTab);
  GcnPlan p = plan_gcn_layer(g5, tab(g5), on);
  EXPECT(p.form == GcnForm::kRefused && strstr(p.why, "no source-tile form"));
  // the row predicate: interleaved form only, else a form that stores every row
  EXPECT(form(g4, pres(g4)) == GcnForm::kTilePred);
  EXPECT(form(g4, pres(g4), {true, true, false, 0}) == GcnForm::kTileFirst);
  EXPECT(form(g5, pres(g5)) == GcnForm::kTileEight);
  EXPECT(form(g9, pres(g9)) == GcnForm::kEdgeX3);
  // geometry: two operand tiles of 32 x (Fin + 2) floats (at least 2048), the image, 512 B of predicate table
  p = plan_gcn_layer(g4, call(g4), on);
  EXPECT(p.geo.lds == 16896 + 129 * 256 && p.geo.per_cu == 3 && p.geo.grid == 768 && p.geo.pieces == 4);
  EXPECT(plan_gcn_layer(g4, pres(g4), on).geo.lds == 16896 + 129 * 256 + 512);
  EXPECT(plan_gcn_layer(g4, call(g4, 48), on).geo.lds == 16384 + 129 * 256);
  EXPECT(plan_gcn_layer(g4, call(g4), {true, true, true, 2}).geo.grid == 512);
  // e >= 6 n
  gcl_graph g = g4;
  g.e = 6 * (int64_t)n;
  EXPECT(form(g, call(g)) == GcnForm::kTileInterleaved);
  g.e = 6 * (int64_t)n - 1;
  EXPECT(form(g, call(g)) == GcnForm::kEdgeX3 && form(g, tab(g)) == GcnForm::kRefused);
  // Fin: source tiles above 32 in steps of 16, split operands in steps of 16
  EXPECT(form(g4, call(g4, 32)) == GcnForm::kEdgeX3 && form(g4, call(g4, 40)) == GcnForm::kEdgeFp32);
  EXPECT(form(g4, call(g4, 48)) == GcnForm::kTileInterleaved && form(g4, call(g4, 64)) == GcnForm::kTileInterleaved);
  EXPECT(form(g4, tab(g4, 32)) == GcnForm::kRefused && form(g4, tab(g4, 48)) == GcnForm::kTileTab);
  // heavy rows have no records in the tile layout
  g = g4;
  g.n_heavy = 1;
  EXPECT(form(g, call(g)) == GcnForm::kEdgeX3);
  p = plan_gcn_layer(g, tab(g), on);
  EXPECT(p.form == GcnForm::kRefused && strstr(p.why, "heavy rows"));
  // switches, graph kind, layout, rows_out
  EXPECT(form(g4, call(g4), {false, true, true, 0}) == GcnForm::kEdgeX3 && form(g4, tab(g4), {false, true, true, 0}) == GcnForm::kRefused);
  EXPECT(form(g4, call(g4), {true, false, true, 0}) == GcnForm::kEdgeFp32 && form(g4, tab(g4), {true, false, true, 0}) == GcnForm::kRefused);
  g = g4;
  g.kind = GCL_GRAPH_MEAN;
  EXPECT(form(g, call(g)) == GcnForm::kEdgeMean && form(g, call(g), {true, false, true, 0}) == GcnForm::kEdgeMean);
  g = g4;
  g.halo[0][0].T = 0;
  EXPECT(form(g, call(g)) == GcnForm::kEdgeX3);
  GcnCall c = call(g4);
  c.rows_out = n - 1;
  EXPECT(form(g4, c) == GcnForm::kEdgeX3);
  // two-part destination: the per-edge split-operand kernel of a GCN graph only
  EXPECT(form(g4, two(g4)) == GcnForm::kRefused && form(g9, two(g9)) == GcnForm::kEdgeX3);
  EXPECT(form(g4, two(g4), {false, true, true, 0}) == GcnForm::kEdgeX3 && form(g4, two(g4), {false, false, true, 0}) == GcnForm::kRefused);
  EXPECT(form(g9, two(g9, 40)) == GcnForm::kRefused && form(g9, two(g9, 48)) == GcnForm::kEdgeX3);
  g = g9;
  g.kind = GCL_GRAPH_MEAN;
  EXPECT(form(g, two(g)) == GcnForm::kRefused);
  // 32-bit offsets of x without a table: n * ldx * 4 < 2^31 (the per-edge kernels too), ldx * 4 < 2^24
  gcl_graph big = tile_graph((int32_t)k2_23 - 1, GCL_GRAPH_GCN, 128), big1 = tile_graph((int32_t)k2_23, GCL_GRAPH_GCN, 128);
  c = call(big);
  c.ldy = 4;
  EXPECT(form(big, c) == GcnForm::kTileInterleaved);
  c = call(big1);
  c.ldy = 4;
  p = plan_gcn_layer(big1, c, on);
  EXPECT(p.form == GcnForm::kRefused && strstr(p.why, "2 GiB"));
  g = tile_graph(100, GCL_GRAPH_GCN, 128);
  c = call(g);
  c.ldx = k2_22 - 4;
  EXPECT(form(g, c) == GcnForm::kTileInterleaved);
  c.ldx = k2_22;
  EXPECT(form(g, c) == GcnForm::kRefused);
  // n * ldy * 4 < 2^31: the output of the source-tile forms, with or without a table
  c = call(big, 48);
  EXPECT(form(big, c) == GcnForm::kTileInterleaved && form(big1, call(big1, 48)) == GcnForm::kEdgeX3);
  EXPECT(form(big, tab(big, 48)) == GcnForm::kTileTab && form(big1, tab(big1, 48)) == GcnForm::kRefused);
  // the 2^32 limits of the row table and its 24-bit row numbers
  c = tab(g4);
  c.ldx = 128;
  c.x_rows = k2_23 - 1;
  EXPECT(form(g4, c) == GcnForm::kTileTab);
  c.x_rows = k2_23;
  EXPECT(form(g4, c) == GcnForm::kRefused);
  c = tab(g4, 48);
  c.x_rows = k2_24 - 1;
  EXPECT(form(g4, c) == GcnForm::kTileTab);
  c.x_rows = k2_24;
  EXPECT(form(g4, c) == GcnForm::kRefused);
  c = tab(g4);
  c.bsx = k2_29 - 4;
  EXPECT(form(g4, c) == GcnForm::kTileTab);
  c.bsx = k2_29;
  EXPECT(form(g4, c) == GcnForm::kRefused);
  c = tab(g4);
  c.ldx = k2_22 - 4;
  c.x_rows = 100;
  EXPECT(form(g4, c) == GcnForm::kTileTab);
  c.ldx = k2_22;
  EXPECT(form(g4, c) == GcnForm::kRefused);
  big = tile_graph((int32_t)k2_24 - 1, GCL_GRAPH_GCN, 128);
  big1 = tile_graph((int32_t)k2_24, GCL_GRAPH_GCN, 128);
  c = tab(g4);
  c.ldy = 4;
  c.rows_out = big.n;
  EXPECT(form(big, c) == GcnForm::kTileTab);
  c.rows_out = big1.n;
  EXPECT(form(big1, c) == GcnForm::kRefused);
}

static void check_aggregate() {
  const AggSwitches on{true, 0, 0};
  const int32_t n = 1000;
  auto call = [&](const gcl_graph& g, int32_t F = 64, int64_t ld = 64) { return AggCall{0, ld, (int64_t)g.n * ld, ld, (int64_t)g.n * ld, F, false, false}; };
  auto form = [&](const gcl_graph& g, AggCall c, bool store_map = false, AggSwitches sw = {true, 0, 0}) {
    c.store_map = store_map;
    return plan_aggregate(g, c, sw).form;
  };
  const gcl_graph g4 = tile_graph(n, GCL_GRAPH_GCN, 128);
  AggPlan p = plan_aggregate(g4, call(g4), on);
  EXPECT(p.form == AggForm::kTile && p.lpr == 16 && p.vl && p.vs && p.hl == &g4.halo[0][0]);
  EXPECT(p.geo.lds == 33024 && p.geo.grid == 1024 && p.geo.bucket() == 4);
  EXPECT(plan_aggregate(g4, call(g4), {true, 0, 3}).geo.grid == 768);
  EXPECT(form(g4, call(g4), true) == AggForm::kTile);
  // F: 16 lanes per row and more (F > 32); lanes per row at 16/17, 32/33, 64/65, 128/129 columns
  EXPECT(form(g4, call(g4, 32)) == AggForm::kPerEdge && form(g4, call(g4, 32), true) == AggForm::kRefused);
  EXPECT(form(g4, call(g4, 36)) == AggForm::kTile && form(g4, call(g4, 36), true) == AggForm::kTile);
  const int Fs[9] = {16, 17, 32, 33, 64, 65, 128, 129, 256}, lpr[9] = {4, 8, 8, 16, 16, 32, 32, 64, 64};
  for (int i = 0; i < 9; ++i) EXPECT(plan_aggregate(g4, call(g4, Fs[i], 256), on).lpr == lpr[i]);
  // 16-byte rows: strides and F
  EXPECT(form(g4, call(g4, 62)) == AggForm::kPerEdge && !plan_aggregate(g4, call(g4, 62), on).vs && plan_aggregate(g4, call(g4, 62), on).vl);
  EXPECT(form(g4, call(g4, 64, 66)) == AggForm::kPerEdge && !plan_aggregate(g4, call(g4, 64, 66), on).vl);
  AggCall c = call(g4, 62, 62);  // no padded tail for the last 16-byte load
  c.ldy = 64;
  EXPECT(!plan_aggregate(g4, c, on).vl);
  c = call(g4);
  c.bsh += 2;
  EXPECT(form(g4, c) == AggForm::kPerEdge);
  c = call(g4);
  c.bsy += 2;
  EXPECT(form(g4, c) == AggForm::kPerEdge && form(g4, c, true) == AggForm::kRefused);
  // two-part sources, GCL_AGG_HALO, the prefix width
  c = call(g4);
  c.two_part = true;
  EXPECT(form(g4, c) == AggForm::kPerEdge);
  EXPECT(form(g4, call(g4), false, {false, 0, 0}) == AggForm::kPerEdge && form(g4, call(g4), true, {false, 0, 0}) == AggForm::kRefused);
  gcl_graph g = g4;
  g.ell_width = 4;
  EXPECT(form(g, call(g)) == AggForm::kPerEdge);
  // heavy rows: a launch of their own behind the tiles, which has no store map; per direction
  g = g4;
  g.n_heavy = 1;
  EXPECT(form(g, call(g)) == AggForm::kTile && form(g, call(g), true) == AggForm::kRefused);
  c = call(g);
  c.transpose = 1;
  EXPECT(form(g, c, true) == AggForm::kTile && plan_aggregate(g, c, on).hl == &g.halo[1][0]);
  g.n_theavy = 1;
  g.n_heavy = 0;
  EXPECT(form(g, c, true) == AggForm::kRefused && form(g, call(g), true) == AggForm::kTile);
  g = g4;
  g.tell_width = 4;
  EXPECT(form(g, c) == AggForm::kPerEdge && form(g, call(g)) == AggForm::kTile);
  // the image cap: T = 64 first, then T = 32; GCL_AGG_HALO_T
  g = tile_graph(n, GCL_GRAPH_GCN, 319);
  EXPECT(form(g, call(g)) == AggForm::kTile);
  g.halo[0][0].smax = 320;
  EXPECT(form(g, call(g)) == AggForm::kPerEdge);
  g.halo[0][1].T = 32;
  g.halo[0][1].smax = smax_of(32, 64);
  p = plan_aggregate(g, call(g), on);
  EXPECT(p.form == AggForm::kTile && p.hl == &g.halo[0][1] && p.geo.pieces == 16 && p.geo.bucket() == 16);
  g.halo[0][1].smax = smax_of(32, 65);
  EXPECT(plan_aggregate(g, call(g), on).geo.pieces == 17 && plan_aggregate(g, call(g), on).geo.bucket() == 32);
  g.halo[0][0].smax = 128;
  EXPECT(plan_aggregate(g, call(g), on).hl == &g.halo[0][0] && plan_aggregate(g, call(g), {true, 32, 0}).hl == &g.halo[0][1]);
  EXPECT(form(g4, call(g4), false, {true, 32, 0}) == AggForm::kPerEdge && form(g4, call(g4), false, {true, 64, 0}) == AggForm::kTile);
  g.halo[0][1].smax = smax_of(32, 129);  // 33 pieces: over the cap as well
  EXPECT(form(g, call(g), false, {true, 32, 0}) == AggForm::kPerEdge);
  // pieces per wave at 4/5 and 8/9
  const int quads[4] = {16, 17, 32, 33}, bucket[4] = {4, 8, 8, 16};
  for (int i = 0; i < 4; ++i) {
    g = tile_graph(n, GCL_GRAPH_GCN, smax_of(64, quads[i]));
    EXPECT(plan_aggregate(g, call(g), on).form == AggForm::kTile && plan_aggregate(g, call(g), on).geo.bucket() == bucket[i]);
  }
  // 32-bit offsets of h
  gcl_graph big = tile_graph((int32_t)k2_23 - 1, GCL_GRAPH_GCN, 128), big1 = tile_graph((int32_t)k2_23, GCL_GRAPH_GCN, 128);
  EXPECT(form(big, call(big)) == AggForm::kTile && form(big1, call(big1)) == AggForm::kPerEdge);
  g = tile_graph(100, GCL_GRAPH_GCN, 128);
  EXPECT(form(g, call(g, 64, k2_22 - 4)) == AggForm::kTile && form(g, call(g, 64, k2_22)) == AggForm::kPerEdge);
}

static void check_gat() {
  const int32_t n = 1000;
  auto fwd = [&](const gcl_graph& g, int32_t H = 1, int32_t C = 64, bool on = true) { return plan_gat_fwd(g, (int64_t)H * C, H, C, on).form; };
  auto bwd = [&](const gcl_graph& g, int32_t H = 1, int32_t C = 64, bool on = true) {
    return plan_gat_bwd(g, (int64_t)H * C, C, (int64_t)g.n * C, H, C, on).form;
  };
  const GatForm T = GatForm::kTile, E = GatForm::kPerEdge;
  const gcl_graph g4 = tile_graph(n, GCL_GRAPH_GAT, 128);
  EXPECT(fwd(g4) == T && bwd(g4) == T);
  GatPlan p = plan_gat_fwd(g4, 64, 1, 64, true);
  EXPECT(p.geo.lds == 129 * 256 + 193 * 4 && p.geo.per_cu == 4 && p.geo.grid == 1024 && p.geo.bucket() == 4);
  p = plan_gat_bwd(g4, 64, 64, (int64_t)n * 64, 1, 64, true);
  EXPECT(p.geo.lds == 129 * 256 + 800 && p.geo_src.lds == 129 * 256 && p.geo_src.grid == 1024);
  // H, C, the switch, the graph kind
  EXPECT(fwd(g4, 2) == E && bwd(g4, 2) == E);
  EXPECT(fwd(g4, 1, 96) == E && bwd(g4, 1, 96) == E && fwd(g4, 1, 128) == T && bwd(g4, 1, 128) == T);
  EXPECT(fwd(g4, 1, 64, false) == E && bwd(g4, 1, 64, false) == E);
  gcl_graph g = g4;
  g.kind = GCL_GRAPH_GCN;
  EXPECT(fwd(g) == E && bwd(g) == E);
  // heavy rows and layouts, per direction
  g = g4;
  g.n_heavy = 1;
  EXPECT(fwd(g) == E && bwd(g) == E);
  g = g4;
  g.n_theavy = 1;
  EXPECT(fwd(g) == T && bwd(g) == E);
  g = g4;
  g.halo[1][0].T = 0;
  EXPECT(fwd(g) == T && bwd(g) == E);
  g = g4;
  g.halo[0][0].T = 0;
  EXPECT(fwd(g) == E && bwd(g) == E);
  // the image cap, C = 128: image rows of 512 B + the kernel's own arrays
  g = tile_graph(n, GCL_GRAPH_GAT, 157);
  EXPECT(fwd(g, 1, 128) == T && bwd(g, 1, 128) == T);
  g.halo[0][0].smax = 158;
  EXPECT(fwd(g, 1, 128) == E && bwd(g, 1, 128) == E);
  g = g4;
  g.halo[1][0].smax = 159;
  EXPECT(bwd(g, 1, 128) == T);
  g.halo[1][0].smax = 160;
  EXPECT(bwd(g, 1, 128) == E && fwd(g, 1, 128) == T);
  // the dst-side backward kernel stages a_s of at most 128 halo rows
  g = tile_graph(n, GCL_GRAPH_GAT, 64 + 128);
  EXPECT(fwd(g) == T && bwd(g) == T);
  g.halo[0][0].smax = 64 + 129;
  EXPECT(fwd(g) == T && bwd(g) == E);
  // 16 pieces per wave at most (beyond the image cap at both widths: pinned on the geometry)
  gcl_halo h;
  h.T = 64;
  h.smax = smax_of(64, 64);
  EXPECT(tile_geo(h, 16, 0).pieces == 16 && !tile_geo(h, 16, 0).fits());
  g = tile_graph(n, GCL_GRAPH_GAT, smax_of(64, 65));
  EXPECT(fwd(g) == E && bwd(g) == E);
  // dy in 16-byte rows, 32-bit offsets of h and dy
  EXPECT(plan_gat_bwd(g4, 64, 66, (int64_t)n * 66, 1, 64, true).form == E && plan_gat_bwd(g4, 64, 64, (int64_t)n * 64 + 2, 1, 64, true).form == E);
  gcl_graph big = tile_graph((int32_t)k2_23 - 1, GCL_GRAPH_GAT, 128), big1 = tile_graph((int32_t)k2_23, GCL_GRAPH_GAT, 128);
  EXPECT(fwd(big) == T && bwd(big) == T && fwd(big1) == E && bwd(big1) == E);
  big = tile_graph((int32_t)k2_22 - 1, GCL_GRAPH_GAT, 128);
  big1 = tile_graph((int32_t)k2_22, GCL_GRAPH_GAT, 128);
  EXPECT(plan_gat_bwd(big, 64, 128, 0, 1, 64, true).form == T && plan_gat_bwd(big1, 64, 128, 0, 1, 64, true).form == E && fwd(big1) == T);
  g = tile_graph(100, GCL_GRAPH_GAT, 128);
  EXPECT(plan_gat_fwd(g, k2_22 - 4, 1, 64, true).form == T && plan_gat_fwd(g, k2_22, 1, 64, true).form == E);
  EXPECT(plan_gat_bwd(g, 64, k2_22 - 4, 0, 1, 64, true).form == T && plan_gat_bwd(g, 64, k2_22, 0, 1, 64, true).form == E);
}

int main() {
  check_helpers();
  check_gcn();
  check_aggregate();
  check_gat();
  printf("%d checks, %d failed\n", g_run, g_fail);
  return g_fail ? 1 : 0;
}
