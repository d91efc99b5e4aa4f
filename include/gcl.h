/*
 * gcl.h - C ABI of libgcl_hip.so: graphcast-lite's encode-process-decode GNN hot path as
 * hand-written gfx950 (MI355X / CDNA4) HIP kernels.
 *
 * The reference (ArturKKK/graphcast-lite) has no native boundary: its hot path is Python calling
 * torch / torch_geometric ops from src/models.py.  Each entry point below names the reference
 * call site whose stock-op expansion it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch types.  Every function returns 0 on success
 *     or a negative GCL_E* code; gcl_last_error() returns a thread-local message.
 *   - Compute entry points never allocate, never synchronise and never create streams: the caller
 *     passes device pointers it owns (contiguous fp32 / int32), explicit leading dimensions, a
 *     workspace where one is needed (size from the matching *_ws_bytes query) and the hipStream_t
 *     to enqueue on (as void*).  They are re-entrant; the only state is the immutable graph handle.
 *   - Node features are row-major `[B, n, F]`: `ld*` = floats between consecutive rows,
 *     `bs*` = floats between consecutive samples.  B independent samples share one graph.
 *   - Activation chaining: buffers passed between layers hold PRE-activation values.  An entry
 *     point that takes `in_slope` (device pointer to one float, may be NULL) applies
 *     PReLU(x) = max(0,x) + slope*min(0,x) to its input while loading it, and its backward returns
 *     the gradient with respect to the PRE-activation input (and adds the slope gradient into
 *     `d_in_slope`).  This is how the reference's `conv -> shared PReLU -> conv` stacks
 *     (src/models.py:321-330,416-421) and `Linear -> PReLU -> Linear` chains (src/models.py:61-109)
 *     run without a separate activation pass.
 */
#ifndef GCL_H
#define GCL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GCL_VERSION 100 /* 0.1.0 */

#define GCL_OK 0
#define GCL_EINVAL (-1)   /* bad argument (shape, alignment, null pointer) */
#define GCL_EHIP (-2)     /* HIP runtime error (message has the hipError string) */
#define GCL_ENOMEM (-3)   /* workspace too small / allocation failed in graph_create */
#define GCL_EUNSUPPORTED (-4)

typedef struct gcl_graph gcl_graph_t; /* opaque; owns device CSR arrays */
typedef void* gcl_stream_t;           /* hipStream_t */

int gcl_version(void);
const char* gcl_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Graph handle: reference-layout edge list -> receiver-sorted CSR (+ sender-sorted transpose).
 * Replaces, once per graph instead of once per forward: add_remaining_self_loops + degree
 * scatter_add + pow(-1/2) + two gathers of PyG gcn_norm (GCNConv, src/models.py:419), the
 * remove_self_loops + add_self_loops of GATConv (src/models.py:425,135) and the in-degree count of
 * SimpleConv(aggr="mean") (src/models.py:414).
 * ------------------------------------------------------------------------------------------- */
#define GCL_GRAPH_GCN 0  /* drop self-loops, append one per node, w_e = deg_in[s]^-1/2 * deg_in[r]^-1/2 */
#define GCL_GRAPH_GAT 1  /* drop self-loops, append one per node, no weights */
#define GCL_GRAPH_MEAN 2 /* edges as given, w_e = 1 / max(1, deg_in[r]) */

/* Sizes of the processed edge set for (edge_index, E, n, kind): E' written to *e_out. */
int gcl_graph_count_edges(const int64_t* edge_index, int64_t E, int32_t n, int32_t kind, int64_t* e_out);

/* Host-only CSR construction into caller arrays (no GPU needed; used by gcl_graph_create and by
 * the CPU tests).  edge_index is int64 [2,E] row 0 = sender, row 1 = receiver (src/models.py:12).
 * Outputs (E' = gcl_graph_count_edges):
 *   rowptr[n+1], col[E'] (sender of each slot), w[E'], eperm[E'] (slot -> position in the PyG edge
 *   order "kept edges in input order, then loops 0..n-1"), and the transpose trowptr[n+1],
 *   tcol[E'] (receiver), tw[E'], tslot[E'] (transpose slot -> forward slot).
 * Within a row, slots keep PyG edge order (stable sort), so sums run in the reference's order. */
int gcl_graph_build_host(const int64_t* edge_index, int64_t E, int32_t n, int32_t kind,
                         int32_t* rowptr, int32_t* col, float* w, int32_t* eperm,
                         int32_t* trowptr, int32_t* tcol, float* tw, int32_t* tslot);

int gcl_graph_create(const int64_t* edge_index, int64_t E, int32_t n, int32_t kind, gcl_graph_t** out);
void gcl_graph_destroy(gcl_graph_t* g);
int32_t gcl_graph_num_nodes(const gcl_graph_t* g);
int64_t gcl_graph_num_edges(const gcl_graph_t* g); /* E' */
int32_t gcl_graph_max_in_degree(const gcl_graph_t* g);
/* PyG-order edge list with loops, host int64 [2,E'] (what GATConv returns: src/models.py:135). */
int gcl_graph_export_edges(const gcl_graph_t* g, int64_t* edge_index_out);
/* Device pointer to eperm (int32 [E']), for callers that re-order per-slot data themselves. */
const int32_t* gcl_graph_eperm_device(const gcl_graph_t* g);
/* Source-tile ("halo") layout of one direction (transpose != 0: sender-sorted) for tile height T (64 or 32):
 * out4 = {T (0 when that layout was not built), tiles, largest staged source count per tile (rounded up to 8),
 * 1 when the per-edge kernels of this direction run their 16-row groups in a processing order (GCL_AGG_ORDER, n >= 32768
 * and no source-tile layout; independent of T) else 0}.  gcl_graph_create builds it when a tile's edges share their sources well enough (>= 1.6 reads per staged
 * row) - e.g. mesh nodes numbered tile by tile; gcl_aggregate then stages every source row of a tile once in
 * LDS instead of gathering it once per edge (the propagate of src/models.py:419). */
int gcl_graph_halo_info(const gcl_graph_t* g, int32_t transpose, int32_t T, int32_t* out4);

/* ---------------------------------------------------------------------------------------------
 * Dense per-node transform  y = act(x) W^T (+ bias)      [rows, Fin] x [Fout, Fin]^T
 * Replaces nn.Linear (+ the preceding nn.PReLU) inside MLP.forward (src/models.py:106-109) and the
 * `lin` GEMM inside every GCNConv/GATConv (src/models.py:419,425).  fp32 in, fp32 accumulate
 * (v_mfma_f32_32x32x2_f32: exact fp32 FMA chain in k order).
 * Padding and strides: every row argument of the dense entry points below (x, z, dy, addend, y, dx; W and dW with their
 * ldw / lddw) may have a row stride larger than its width, sit at a column offset inside wider rows, and start at any
 * float-aligned address.  The columns of an INPUT past its width and everything between its rows are ignored, whatever
 * they hold (NaN and Inf included): the result is bit-equal to the result with zeros there.  The columns of an OUTPUT
 * past its width (Fout of y, Fin of dx and of dW's rows) and everything between its rows are never written.  One
 * exception: gcl_linear_bwd_all with Fout % 4 != 0 needs FINITE padding in dy up to roundup(Fout, 4) (see there).  The
 * layout only selects the kernel: rows with ld % 4 == 0 on a 16-byte aligned base are read 16 bytes at a time, all
 * others element by element.
 * Refused with GCL_EINVAL (nothing is written): a leading dimension smaller than its width; and every call that falls
 * to the 128x128 tile kernel (ldw != Fin, an addend, a contraction or an output wider than 256, a weight panel beyond
 * the LDS, or a contraction longer than 128 on rows that are not 16-byte ones) whose contraction length is no multiple
 * of 4 or whose input rows or weight rows are not 16-byte ones; gcl_dense_bwd_dx on that kernel also needs Fin % 4 == 0
 * unless it can transpose W into the workspace first (Fout % 4 == 0 and rows >= 4096).
 * Values (tests/test_value_contract.py).  A NaN or Inf in one element reaches only the outputs the arithmetic carries it
 * to (a row of y or dx, a row / column of dW, an element of db); every other output keeps, bit for bit, what it has
 * without it.  PReLU takes its slope branch for NaN in the forward AND in the backward (x > 0 ? 1 : slope, as torch does),
 * so a NaN in x reaches the slope gradient.  The kernels are linear in each operand: while nothing leaves fp32's normal
 * range, scaling an operand (and the additive terms) by 2^k scales the result by exactly 2^k.
 * The band of the split-operand kernels.  gcl_dense_fwd (Fin <= 64, Fout <= 64 on 16-byte rows; the tile
 * kernel once it has 1536 tiles), gcl_linear_bwd_all (Fin 33..64), gcl_mlp_fwd_chain and the staged gcl_gcn_layer_fwd run on the bf16 matrix
 * pipe with every fp32 operand split into three bf16 pieces (csrc/x3.h; GCL_X3=0: the fp32-operand kernels).  Their
 * result is as close to the exact one as an fp32 GEMM's when
 *   - every element v of both operands is 0 or 2^-110 <= |v| < 2^127, and
 *   - for every output the sum of |products| is below 2^127.
 * Below 2^-110 an element loses the bits under 2^-133 (accuracy halves per binade; nothing becomes non-finite); from
 * 2^128 (1 - 2^-9) on - the largest finite fp32 included - a FINITE element gives NaN, because its first piece rounds
 * to inf.  Measured table and derivation: csrc/x3.h, DESIGN.md 3.1.
 * ------------------------------------------------------------------------------------------- */
int gcl_linear_fwd(const float* x, int64_t ldx, const float* in_slope, const float* W /*[Fout,Fin]*/,
                   const float* bias /*[Fout] or NULL*/, float* y, int64_t ldy, int64_t rows,
                   int32_t Fin, int32_t Fout, gcl_stream_t stream);

/* dx = (dy W) * PReLU'(x)   [rows, Fin]; adds sum(dy W * min(0,x)) into *d_in_slope when in_slope
 * is given.  ws: gcl_linear_bwd_ws_bytes(rows, Fin, Fout). */
int gcl_linear_bwd_dx(const float* dy, int64_t lddy, const float* W, const float* x, int64_t ldx,
                      const float* in_slope, float* d_in_slope, float* dx, int64_t lddx,
                      int64_t rows, int32_t Fin, int32_t Fout, void* ws, size_t ws_bytes,
                      gcl_stream_t stream);
/* dW (+)= dy^T act(x), db (+)= colsum(dy) (db may be NULL).  accumulate != 0 adds into dW/db. */
int gcl_linear_bwd_dw(const float* dy, int64_t lddy, const float* x, int64_t ldx,
                      const float* in_slope, float* dW, float* db, int64_t rows, int32_t Fin,
                      int32_t Fout, int32_t accumulate, void* ws, size_t ws_bytes,
                      gcl_stream_t stream);
size_t gcl_linear_bwd_ws_bytes(int64_t rows, int32_t Fin, int32_t Fout);
/* Whole backward of one dense transform in one call: dx (pre-activation gradient), dW, db (NULL: no
 * bias), the slope gradient, and optionally colsum_dx[c] (+)= sum_r dx[r,c] (the bias gradient of
 * the conv layer that produced x).  Uses ONE fused kernel (dY and x read once) when
 * Fout <= 64, Fin <= 96 and rows are 16-B aligned, else the three separate kernels.  Fout itself need not be a
 * multiple of 4 when lddy >= roundup(Fout, 4) and the padding columns of dy hold finite values (zeros): this is how
 * the 33- / 19-wide last decoder conv runs on 16-byte rows without padded copies of its weight.
 * `accumulate` is a bit mask with ONE BIT PER DESTINATION (they belong to different parameters,
 * whose gradients may be in different states): a set bit adds into that destination, a clear bit
 * overwrites it.  *d_in_slope is always added to. */
#define GCL_ACC_DW 1     /* dW */
#define GCL_ACC_DB 2     /* db */
#define GCL_ACC_COLSUM 4 /* colsum_dx */
int gcl_linear_bwd_all(const float* dy, int64_t lddy, const float* W, const float* x, int64_t ldx,
                       const float* in_slope, float* d_in_slope, float* dx, int64_t lddx, float* dW,
                       float* db, float* colsum_dx, int64_t rows, int32_t Fin, int32_t Fout,
                       int32_t accumulate, void* ws, size_t ws_bytes, gcl_stream_t stream);
size_t gcl_linear_bwd_all_ws_bytes(int64_t rows, int32_t Fin, int32_t Fout);

/* Deferred final pass.  A training step calls gcl_linear_bwd_all once per layer, and each call ends in a small launch
 * that sums its per-block partial records into dW / db / colsum_dx / the slope gradient.  The _deferred form runs the
 * main kernel only and DESCRIBES that pass in *job; gcl_reduce_jobs later runs the passes of many calls in one launch
 * per 24 jobs (the gradients of one optimiser step, src/train.py:232-233, are only read after the whole backward).
 * Rules: every deferred call needs its OWN workspace, alive until gcl_reduce_jobs has run; two pending jobs must not
 * write the same dW / db / colsum_dx (flush first; a shared slope gradient is fine: slopes are summed job after job);
 * job->nparts == 0 means the call took the non-fused path and has already reduced on the spot. */
/* One output of a final pass: `count` consecutive floats of every partial record from offset `poff`; element e goes to
 * out[(e / pld) * ldo + e % pld] when e % pld < cols, added to what is there (acc 1) or replacing it (acc 0). */
typedef struct gcl_reduce_seg {
  float* out; /* NULL: unused segment */
  int32_t poff, count, pld, cols, ldo, acc;
} gcl_reduce_seg;
typedef struct gcl_reduce_job {
  const float* part; /* per-block partial records */
  int64_t pstride;   /* floats between records */
  gcl_reduce_seg seg[3]; /* dW | db | colsum_dx */
  const double* spart; /* slope partials (one per block) or NULL */
  float* sout;
  int32_t nparts, ns;
} gcl_reduce_job;
int gcl_linear_bwd_all_deferred(const float* dy, int64_t lddy, const float* W, const float* x, int64_t ldx,
                                const float* in_slope, float* d_in_slope, float* dx, int64_t lddx, float* dW,
                                float* db, float* colsum_dx, int64_t rows, int32_t Fin, int32_t Fout,
                                int32_t accumulate, void* ws, size_t ws_bytes, gcl_stream_t stream,
                                gcl_reduce_job* job);
int gcl_reduce_jobs(const gcl_reduce_job* jobs, int32_t n, gcl_stream_t stream);
/* Deferred forms of the other calls that end in such a pass, under the same rules (declared here because they share
 * gcl_reduce_job; the calls themselves are described further down).  Each behaves as its immediate form up to the final
 * pass and fills *job; a call whose immediate pass would not take the 16-byte reducer (fewer than 64 partial records)
 * reduces on the spot and leaves nparts == 0.  The dW forms fill job[0] (dW) and job[1] (db; nparts == 0 without db):
 * `job` must have room for two.
 * gcl_layernorm_bwd_deferred covers gcl_layernorm_bwd / _cs (pos NULL), _map (skip 0) and _map_skip (skip 1). */
int gcl_layernorm_bwd_deferred(const float* dy, int64_t lddy, int64_t bsdy, const int32_t* pos, int32_t n_per,
                               int32_t skip, const float* x, int64_t ldx, const float* gamma, const float* stats,
                               float* dx, int64_t lddx, float* dgamma, float* dbeta, float* colsum_dx,
                               int32_t accumulate, int64_t rows, int32_t F, void* ws, size_t ws_bytes,
                               gcl_stream_t stream, gcl_reduce_job* job);
int gcl_colsum_deferred(const float* x, int64_t ldx, int64_t rows, int32_t F, float* out, int32_t accumulate, void* ws,
                        size_t ws_bytes, gcl_stream_t stream, gcl_reduce_job* job);
int gcl_colsum_split_deferred(const float* a, int64_t lda, int64_t bsa, const float* b, int64_t ldb, int64_t bsb,
                              int32_t head, int32_t n, int32_t B, int32_t F, float* out, int32_t accumulate, void* ws,
                              size_t ws_bytes, gcl_stream_t stream, gcl_reduce_job* job);
int gcl_linear_bwd_dw_deferred(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* in_slope,
                               float* dW, float* db, int64_t rows, int32_t Fin, int32_t Fout, int32_t accumulate,
                               void* ws, size_t ws_bytes, gcl_stream_t stream, gcl_reduce_job* job /* [2] */);
int gcl_dense_bwd_dw_deferred(const float* dy, int64_t lddy, const float* x, int64_t ldx, int32_t act,
                              const float* slope, float* dW, int64_t lddw, float* db, int64_t rows, int32_t Fin,
                              int32_t Fout, int32_t accumulate, void* ws, size_t ws_bytes, gcl_stream_t stream,
                              gcl_reduce_job* job /* [2] */);

/* General form of the three calls above, for wide layers and fused operands (the InteractionNet
 * processor, src/models.py:185-233, and the 256-wide MLPs): any Fin / Fout, the weight may be a
 * column block of a wider matrix (row stride ldw >= Fin, e.g. one third of edge_mlp[0].weight
 * [256, 768]), the activation on the input is selectable, and an addend [rows, Fout] can be summed
 * in the epilogue (residuals; the second half of a split contraction).
 * Shapes that fit the resident-weight-panel kernel run there; wider ones (K or N > 256, or a panel
 * beyond 160 KiB of LDS) run a 128x128-tile contraction that needs Fin % 4 == 0 and 16-B aligned
 * rows.  All use the exact-fp32 matrix instruction. */
#define GCL_ACT_NONE 0
#define GCL_ACT_PRELU 1 /* one learnable slope (nn.PReLU()); needs the slope pointer */
#define GCL_ACT_SILU 2  /* x * sigmoid(x)  (nn.SiLU, "swish": src/models.py:154-163) */
/* y = act(x) W^T + bias + addend */
int gcl_dense_fwd(const float* x, int64_t ldx, int32_t act, const float* slope, const float* W,
                  int64_t ldw, const float* bias, const float* addend, int64_t ldadd, float* y,
                  int64_t ldy, int64_t rows, int32_t Fin, int32_t Fout, gcl_stream_t stream);
/* dx = (dy W) * act'(z) + addend, z = the pre-activation the forward call read as x; PReLU adds
 * its slope gradient into *d_slope (may be NULL).  ws: gcl_linear_bwd_ws_bytes(rows, Fin, Fout). */
int gcl_dense_bwd_dx(const float* dy, int64_t lddy, const float* W, int64_t ldw, const float* z,
                     int64_t ldz, int32_t act, const float* slope, float* d_slope,
                     const float* addend, int64_t ldadd, float* dx, int64_t lddx, int64_t rows,
                     int32_t Fin, int32_t Fout, void* ws, size_t ws_bytes, gcl_stream_t stream);
/* dW[o, c] (+)= sum_r dy[r, o] act(x[r, c]) (row stride lddw), db (+)= colsum(dy) (may be NULL) */
int gcl_dense_bwd_dw(const float* dy, int64_t lddy, const float* x, int64_t ldx, int32_t act,
                     const float* slope, float* dW, int64_t lddw, float* db, int64_t rows,
                     int32_t Fin, int32_t Fout, int32_t accumulate, void* ws, size_t ws_bytes,
                     gcl_stream_t stream);

/* A run of nlayers = 2 or 3 consecutive Linear layers of an MLP in ONE launch (src/models.py:106-109):
 *   z0 = act0(x) W0^T + b0,   z1 = prelu(z0; slope1) W1^T + b1,   z2 = prelu(z1; slope2) W2^T + b2
 * with every z_k [rows, N_k] stored (row stride ldz_k) as the per-layer calls store it, bit for bit: a layer runs the same
 * code as in gcl_dense_fwd, its input rows are handed over inside the kernel instead of being read back.  act0 is
 * GCL_ACT_NONE or GCL_ACT_PRELU (slope0); a null slope1 / slope2 means no activation in front of that layer; the
 * arguments of layer 2 are ignored when nlayers == 2.  gamma != NULL: the node LayerNorm that follows the last layer is
 * applied in the same launch (the arithmetic of gcl_layernorm_fwd on 16-byte rows, bit for bit): y [rows, N_last] (row
 * stride ldy) and stats [rows][2] = (mean, rstd) are stored besides the pre-norm z.
 * gcl_mlp_fwd_chain_ok answers 1 when the run can be chained: GCL_MLP_CHAIN is not 0 (read per call), every layer is
 * one that gcl_dense_fwd runs on the 3-way-split bf16 kernel for 33..64 wide layers (33 <= K, N_k <= 64, N_k % 4 == 0,
 * GCL_X3 on, 16-byte rows), z_k of every layer but the last is contiguous (ldz_k == N_k) and, with gamma, nlayers == 2,
 * y has 16-byte rows and stats is 8-byte aligned (a run refused with gamma may pass without: the LayerNorm is then a
 * launch of its own).  gcl_mlp_fwd_chain refuses other runs with GCL_EINVAL: the caller launches them per layer. */
int gcl_mlp_fwd_chain_ok(const float* x, int64_t ldx, int64_t rows, int32_t K, int32_t act0, int32_t nlayers,
                         const float* z0, int64_t ldz0, int32_t N0, const float* z1, int64_t ldz1, int32_t N1,
                         const float* z2, int64_t ldz2, int32_t N2, const float* gamma, const float* y, int64_t ldy,
                         const float* stats);
int gcl_mlp_fwd_chain(const float* x, int64_t ldx, int64_t rows, int32_t K, int32_t act0, const float* slope0,
                      int32_t nlayers, const float* W0, const float* b0, float* z0, int64_t ldz0, int32_t N0,
                      const float* W1, const float* b1, const float* slope1, float* z1, int64_t ldz1, int32_t N1,
                      const float* W2, const float* b2, const float* slope2, float* z2, int64_t ldz2, int32_t N2,
                      const float* gamma, const float* beta, float eps, float* y, int64_t ldy, float* stats,
                      gcl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Sparse aggregation over the CSR  y[b,i,:] = sum_{e in row i} w_e * h[b, col_e, :] (+ bias)
 * Replaces the index_select -> multiply -> scatter_add_ of PyG propagate for GCNConv
 * (src/models.py:419) and SimpleConv mean (src/models.py:414).  transpose != 0 walks the
 * sender-sorted CSR instead (the backward: dh = A_hat^T dy).
 * Padding and strides: h and y of gcl_aggregate / gcl_aggregate_present may have any row stride >= F, any batch stride
 * and any float-aligned base; 16-byte rows (ld % 4 == 0, bs % 4 == 0, aligned base; for h: ldh >= roundup(F, 4), which
 * such rows always have) are read and, when F % 4 == 0 too, written 16 bytes at a time.  The columns of h past F, the
 * space between its rows and between its samples are ignored, whatever they hold (NaN and Inf included; the vector loads
 * do fetch columns F .. roundup(F, 4) and drop them); the columns of y past F, rows past n and the space between samples
 * are never written.  The same holds for the graph layers further down, which only take 16-byte rows and refuse others
 * with GCL_EINVAL: gcl_gcn_layer_fwd* (x: columns past Fin ignored; y: columns [Fout, Fout_store) written as zeros,
 * columns past Fout_store and rows past rows_out never written), gcl_gat_fwd / gcl_gat_bwd (h, dy: columns past H * C / C
 * ignored; y, dh: columns past C / H * C never written; dy must be row-contiguous across the batch), gcl_segment_reduce
 * and gcl_edge_combine (strided src / A / C; strided out of the former).
 * Refused with GCL_EINVAL (nothing is written): a leading dimension smaller than F, h == y, a GCL_GRAPH_GAT graph.
 * ------------------------------------------------------------------------------------------- */
int gcl_aggregate(const gcl_graph_t* g, int32_t transpose, const float* h, int64_t ldh, int64_t bsh,
                  const float* bias, float* y, int64_t ldy, int64_t bsy, int32_t B, int32_t F,
                  gcl_stream_t stream);
/* Rows with more than 64 edges (in the direction of the call) are summed by one block each, in a launch of their own
 * behind the main one.  `transpose` of gcl_aggregate, gcl_aggregate_present and gcl_aggregate_split is a flag word: bit 0
 * the direction, GCL_AGG_HEAVY_INSIDE asks for those blocks as the FIRST blocks of the main launch instead, where the
 * per-edge kernel runs it with 16-byte rows (elsewhere, and with GCL_AGG_HEAVY_SEPARATE=1, read per call, the flag is
 * ignored) - the same bits either way.  gcl_aggregate_heavy_launches: how many separate launches this process has made
 * (a counter for tests). */
#define GCL_AGG_HEAVY_INSIDE 2
int64_t gcl_aggregate_heavy_launches(void);
/* The same with ABSENT source rows: present [n] has one entry per node, >= 0 = the row of h exists, < 0 = it counts as a
 * row of zeros and is never read, whatever the memory behind it holds (a stage boundary that drops rows: the producer of
 * h need not store them).  Bit-equal to gcl_aggregate on a copy of h whose absent rows are zero. */
int gcl_aggregate_present(const gcl_graph_t* g, int32_t transpose, const float* h, int64_t ldh, int64_t bsh,
                          const int32_t* present /*[n]*/, const float* bias, float* y, int64_t ldy, int64_t bsy,
                          int32_t B, int32_t F, gcl_stream_t stream);
/* The same with the source rows in TWO tensors: row j of sample b is h + b * bsh + j * ldh for j < head and
 * h2 + b * bsh2 + (j - head) * ldh2 otherwise (a gradient whose head and tail rows were left in two places by their
 * producers).  Both parts and y need 16-byte rows (F % 4 == 0, strides % 4 == 0, aligned bases), else GCL_EINVAL; a part
 * with no rows (head == 0 / head == n) may be NULL.  Bit-equal to gcl_aggregate on the two parts copied into one tensor. */
int gcl_aggregate_split(const gcl_graph_t* g, int32_t transpose, const float* h, int64_t ldh, int64_t bsh,
                        const float* h2, int64_t ldh2, int64_t bsh2, int32_t head, const float* bias, float* y,
                        int64_t ldy, int64_t bsy, int32_t B, int32_t F, gcl_stream_t stream);
/* The two-part form whose second part is all zeros: rows j < head of every sample are h + b * bsh + j * ldh, rows
 * j >= head count as rows of zeros that the library supplies itself (the gradient of a layer that returned only its
 * first `head` rows, read where its producer left it instead of from a zero-filled copy).  Same conditions on h and y as
 * gcl_aggregate_split; 0 < head <= n.  Bit-equal to gcl_aggregate on h widened with zero rows. */
int gcl_aggregate_head(const gcl_graph_t* g, int32_t transpose, const float* h, int64_t ldh, int64_t bsh, int32_t head,
                       const float* bias, float* y, int64_t ldy, int64_t bsy, int32_t B, int32_t F, gcl_stream_t stream);
/* gcl_aggregate with a STORE map: smap [n] has one entry per row, >= 0 = that row of every sample is stored to row
 * smap[i] of the compact destination yc [B, *, F] INSTEAD of y, < 0 = stored to y as always.  Each row is written once,
 * to one place, with gcl_aggregate's bits; the rows of y with an entry >= 0 are not touched.  Only the source-tile kernel
 * has the map: gcl_aggregate_compact_ok says (1 / 0) whether a call with these strides is taken, otherwise
 * gcl_aggregate_compact returns GCL_EINVAL and writes nothing.  The query reads the plan the launcher reads
 * (csrc/tile_plan.h, plan_aggregate): it is 1 exactly when the call runs, given 16-byte aligned h, y and yc. */
int gcl_aggregate_compact_ok(const gcl_graph_t* g, int32_t transpose, int64_t ldh, int64_t bsh, int64_t ldy, int64_t bsy,
                             int32_t B, int32_t F);
int gcl_aggregate_compact(const gcl_graph_t* g, int32_t transpose, const float* h, int64_t ldh, int64_t bsh,
                          const int32_t* smap /*[n]*/, float* y, int64_t ldy, int64_t bsy, float* yc, int64_t ldc,
                          int64_t bsc, int32_t B, int32_t F, gcl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * GATConv(heads=H, concat=False) attention + aggregation  (src/models.py:425; SparseGATConv :135)
 *   a_s = <h, att_src>, a_d = <h, att_dst> per head; e = LeakyReLU_0.2(a_s[j] + a_d[i]);
 *   softmax over the in-edges of i (max subtracted, +1e-16 in the denominator);
 *   y[i] = mean_heads sum_e alpha_e h[j_e] + bias.
 * h is the output of gcl_linear_fwd with Fout = H*C, laid out [B, n, H*C].
 * alpha (may be NULL in inference) is written per CSR slot: [B, E', H].
 * ------------------------------------------------------------------------------------------- */
int gcl_gat_fwd(const gcl_graph_t* g, const float* h, int64_t ldh, int64_t bsh,
                const float* att_src /*[H*C]*/, const float* att_dst /*[H*C]*/, const float* bias /*[C]*/,
                float* a_src /*[B,n,H]*/, float* a_dst /*[B,n,H]*/, float* alpha /*[B,E',H]*/,
                float* y, int64_t ldy, int64_t bsy, int32_t B, int32_t H, int32_t C,
                gcl_stream_t stream);
/* Gradients of gcl_gat_fwd: dh [B,n,H*C] (grad of the linear output, attention paths included),
 * d_att_src/d_att_dst [H*C] and d_bias [C] (added when accumulate != 0, else overwritten).
 * ws: gcl_gat_bwd_ws_bytes(E', n, B, H, C). */
int gcl_gat_bwd(const gcl_graph_t* g, const float* dy, int64_t lddy, int64_t bsdy,
                const float* h, int64_t ldh, int64_t bsh, const float* att_src, const float* att_dst,
                const float* a_src, const float* a_dst, const float* alpha,
                float* dh, int64_t lddh, int64_t bsdh, float* d_att_src, float* d_att_dst,
                float* d_bias, int32_t accumulate, int32_t B, int32_t H, int32_t C,
                void* ws, size_t ws_bytes, gcl_stream_t stream);
size_t gcl_gat_bwd_ws_bytes(int64_t e_prime, int32_t n, int32_t B, int32_t H, int32_t C);
/* The same two calls with the rows of h read THROUGH a row table (the stage split of src/models.py:837-838 folded
 * into the first processor layer: only the compact rows are transformed, functional.LatSource): row i of sample b is
 * row tab[i] of sample b of h when tab[i] >= 0, the batch-invariant flat row ~tab[i] of h otherwise; a_src / a_dst /
 * alpha / y / dh stay dense [B, n, ..].  One head on a source-tile graph (gcl_gat_tab_ok returns 1), else
 * GCL_EUNSUPPORTED.  gcl_gat_bwd_tab's dh is the gradient of the table-read rows; the caller folds it back.
 * gcl_gat_tab_ok is 1 when the plans of BOTH launchers (csrc/tile_plan.h, plan_gat_fwd and plan_gat_bwd) choose the
 * source-tile kernels for this ldh, taking dy as a contiguous [B, n, C] tensor.  It sees neither pointers nor B and bsh:
 * 16-byte aligned att_src / att_dst / bias / dy and B * bsh * 4 < 2^32 are the caller's to keep. */
int gcl_gat_fwd_tab(const gcl_graph_t* g, const float* h, int64_t ldh, int64_t bsh, const int32_t* tab /*[n]*/,
                    const float* att_src, const float* att_dst, const float* bias, float* a_src, float* a_dst,
                    float* alpha, float* y, int64_t ldy, int64_t bsy, int32_t B, int32_t H, int32_t C,
                    gcl_stream_t stream);
int gcl_gat_bwd_tab(const gcl_graph_t* g, const float* dy, int64_t lddy, int64_t bsdy, const float* h, int64_t ldh,
                    int64_t bsh, const int32_t* tab /*[n]*/, const float* att_src, const float* att_dst,
                    const float* a_src, const float* a_dst, const float* alpha, float* dh, int64_t lddh, int64_t bsdh,
                    float* d_att_src, float* d_att_dst, float* d_bias, int32_t accumulate, int32_t B, int32_t H,
                    int32_t C, void* ws, size_t ws_bytes, gcl_stream_t stream);
int gcl_gat_tab_ok(const gcl_graph_t* g, int64_t ldh, int32_t H, int32_t C);
/* Re-order per-slot attention of ONE sample into PyG edge order: out[eperm[s]*H + k] = alpha[s*H + k]
 * (what SparseGATConv thresholds: src/models.py:136-149). */
int gcl_gat_alpha_to_edge_order(const gcl_graph_t* g, const float* alpha_slots, float* alpha_edges,
                                int32_t H, gcl_stream_t stream);
/* SparseGATConv prune (src/models.py:138-149): keep PyG-order edges with alpha >= threshold.
 * alpha_edges is a DEVICE array [E'] (H = 1).  Writes the surviving edge list, host int64
 * [2, *kept] (capacity E'), synchronising `stream` once.  Wave-ballot + prefix compaction. */
int gcl_gat_prune(const gcl_graph_t* g, const float* alpha_edges, float threshold,
                  int64_t* edge_index_out, int64_t* kept, void* ws, size_t ws_bytes,
                  gcl_stream_t stream);
size_t gcl_gat_prune_ws_bytes(int64_t e_prime);

/* ---------------------------------------------------------------------------------------------
 * PyG LayerNorm(mode="node")  (src/models.py:102-104,368-374): per row, eps inside the sqrt.
 * stats [rows,2] receives (mean, rstd) for the backward.  x may carry an activation (in_slope).
 * Padding: every row argument (x, dy, y, dx) may have a row stride ld > F and any float-aligned base.  The columns past F
 * of x and dy are ignored, whatever their value (NaN and Inf included), and the columns past F of y and dx are not
 * written.  This holds for all the LayerNorm entry points below, mapped forms included.
 * ------------------------------------------------------------------------------------------- */
int gcl_layernorm_fwd(const float* x, int64_t ldx, const float* gamma, const float* beta, float eps,
                      float* y, int64_t ldy, float* stats, int64_t rows, int32_t F,
                      gcl_stream_t stream);
/* The same with the output written THROUGH a row map: row (b, i) of the [B][n_per] row space goes to
 * y[b * bsy + pos[i] * ldy] when pos[i] >= 0 and nowhere otherwise (stats are written for every row).  The processor's
 * final LayerNorm writes the rows the decoder reads straight into the decoder's input (src/models.py:860-862). */
int gcl_layernorm_fwd_map(const float* x, int64_t ldx, const float* gamma, const float* beta, float eps, float* y,
                          int64_t ldy, int64_t bsy, const int32_t* pos /*[n_per]*/, int32_t n_per, float* stats,
                          int64_t rows, int32_t F, gcl_stream_t stream);
int gcl_layernorm_bwd(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* gamma,
                      const float* stats, float* dx, int64_t lddx, float* dgamma, float* dbeta,
                      int32_t accumulate, int64_t rows, int32_t F, void* ws, size_t ws_bytes,
                      gcl_stream_t stream);
/* Same, and colsum_dx[j] (+)= sum over rows of dx[:, j] when colsum_dx != NULL: dx is the dY of the layer below,
 * so this is that layer's bias gradient (GCNConv.bias of the last conv under the stack's LayerNorm,
 * src/models.py:368-374,419) without a second pass over dx.  accumulate: GCL_ACC_DW covers dgamma and dbeta,
 * GCL_ACC_COLSUM the column sums. */
int gcl_layernorm_bwd_cs(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* gamma,
                         const float* stats, float* dx, int64_t lddx, float* dgamma, float* dbeta,
                         float* colsum_dx, int32_t accumulate, int64_t rows, int32_t F, void* ws,
                         size_t ws_bytes, gcl_stream_t stream);
/* Same with dy given through a row map: the rows are B samples of n_per rows, row (b, i) reads
 * dy[b * bsdy + pos[i] * lddy + :] when pos[i] >= 0 and a zero gradient otherwise - the output of the layer was only
 * consumed through a row gather (the decoder reads a subset of the processor's mesh rows, src/models.py:860-862), so
 * the zero-filled dense gradient never has to be formed.  pos == NULL: dy is dense as above. */
int gcl_layernorm_bwd_map(const float* dy, int64_t lddy, int64_t bsdy, const int32_t* pos, int32_t n_per,
                          const float* x, int64_t ldx, const float* gamma, const float* stats, float* dx,
                          int64_t lddx, float* dgamma, float* dbeta, float* colsum_dx, int32_t accumulate,
                          int64_t rows, int32_t F, void* ws, size_t ws_bytes, gcl_stream_t stream);
/* The mapped pair for a LayerNorm whose dropped rows (pos[i] < 0) have no reader at all: such a row is neither loaded nor
 * stored by either call.  Forward: rlist [n_list] lists the rows i with pos[i] >= 0; only those rows of every sample are
 * read, normalised, written through the map and given statistics (the same bits as gcl_layernorm_fwd_map gives them); the
 * statistics of the other rows are left as they were.  Backward: x, the statistics and dx of a dropped row are not
 * touched (its dx is exactly zero - the consumer takes the zero from the map, see gcl_aggregate_present); dx of the kept
 * rows, dgamma, dbeta and colsum_dx are bit-equal to gcl_layernorm_bwd_map on the same rows. */
int gcl_layernorm_fwd_map_skip(const float* x, int64_t ldx, const float* gamma, const float* beta, float eps, float* y,
                               int64_t ldy, int64_t bsy, const int32_t* pos /*[n_per]*/, int32_t n_per,
                               const int32_t* rlist /*[n_list]*/, int32_t n_list, float* stats, int64_t rows, int32_t F,
                               gcl_stream_t stream);
int gcl_layernorm_bwd_map_skip(const float* dy, int64_t lddy, int64_t bsdy, const int32_t* pos, int32_t n_per,
                               const float* x, int64_t ldx, const float* gamma, const float* stats, float* dx,
                               int64_t lddx, float* dgamma, float* dbeta, float* colsum_dx, int32_t accumulate,
                               int64_t rows, int32_t F, void* ws, size_t ws_bytes, gcl_stream_t stream);
size_t gcl_layernorm_bwd_ws_bytes(int64_t rows, int32_t F);
/* PyG LayerNorm(mode="graph"): statistics over all n*F elements of each sample, eps added to the
 * std.  stats [B,2] = (mean, 1/(std+eps)). */
int gcl_graphnorm_fwd(const float* x, int64_t ldx, int64_t bsx, const float* gamma, const float* beta,
                      float eps, float* y, int64_t ldy, int64_t bsy, float* stats, int32_t B,
                      int32_t n, int32_t F, void* ws, size_t ws_bytes, gcl_stream_t stream);
int gcl_graphnorm_bwd(const float* dy, int64_t lddy, int64_t bsdy, const float* x, int64_t ldx,
                      int64_t bsx, const float* gamma, const float* stats, float eps, float* dx,
                      int64_t lddx, int64_t bsdx, float* dgamma, float* dbeta, int32_t accumulate,
                      int32_t B, int32_t n, int32_t F, void* ws, size_t ws_bytes, gcl_stream_t stream);
size_t gcl_graphnorm_ws_bytes(int32_t B, int32_t n, int32_t F);

/* Column sums  out[c] (+)= sum_r x[r,c]  (bias gradients of the conv layers). */
int gcl_colsum(const float* x, int64_t ldx, int64_t rows, int32_t F, float* out, int32_t accumulate,
               void* ws, size_t ws_bytes, gcl_stream_t stream);
size_t gcl_colsum_ws_bytes(int64_t rows, int32_t F);
/* Column sums over the B * n rows of a two-part source (see gcl_aggregate_split; the same conditions): bit-equal to
 * gcl_colsum on the two parts copied into one [B * n, F] tensor.  Workspace: gcl_colsum_ws_bytes(B * n, F). */
int gcl_colsum_split(const float* a, int64_t lda, int64_t bsa, const float* b, int64_t ldb, int64_t bsb, int32_t head,
                     int32_t n, int32_t B, int32_t F, float* out, int32_t accumulate, void* ws, size_t ws_bytes,
                     gcl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Input assembly (src/models.py:776-806): out[b] = [ x[b] | grid_static ; 0 | mesh_static ],
 * out is [B, G+M, Cdyn+Cs].  The reference re-allocates the zero block and re-concatenates on
 * every forward.
 * ------------------------------------------------------------------------------------------- */
int gcl_assemble_input(const float* x /*[B,G,Cdyn]*/, const float* grid_static /*[G,Cs]*/,
                       const float* mesh_static /*[M,Cs]*/, float* out, int64_t ldo, int32_t B,
                       int32_t G, int32_t M, int32_t Cdyn, int32_t Cs, gcl_stream_t stream);
/* The same with the last r of the M mesh rows of every sample given whole, tail [B, r, Cdyn + Cs] contiguous (the
 * per-sample folded rows of the compact pipeline: each sample carries different ones).  mesh_static may be NULL when
 * r == M. */
int gcl_assemble_input_tail(const float* x, const float* grid_static, const float* mesh_static, const float* tail,
                            int32_t r, float* out, int64_t ldo, int32_t B, int32_t G, int32_t M, int32_t Cdyn,
                            int32_t Cs, gcl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Residual add + weighted MSE and its gradient (src/train.py:203-213, 85-102).
 *   out = x_last + delta (use_residual) or delta; loss = sum(w (out-y)^2) * inv_wsum;
 *   w[g,c] = node_w[g] * chan_w[c] (either may be NULL = 1);
 *   d_delta = 2 w (out-y) * inv_wsum * grad_scale.
 * x_last / y are addressed as base + b*bs + g*ld + c.  loss_out: one device float (overwritten).
 * out_state (may be NULL) receives `out` for autoregressive roll-forward.
 * ------------------------------------------------------------------------------------------- */
/* loss_prev (device float, may be NULL): *loss_out = *loss_prev + loss of this call - the running sum over the
 * autoregressive steps of one batch (src/train.py:213,231) without a separate add. */
int gcl_wmse_fwd_bwd(const float* delta, int64_t ldd, int64_t bsd, const float* x_last, int64_t ldx,
                     int64_t bsx, const float* y, int64_t ldy_, int64_t bsy, const float* node_w,
                     const float* chan_w, float inv_wsum, float grad_scale, float* d_delta,
                     float* out_state, const float* loss_prev, float* loss_out, int32_t B, int32_t G,
                     int32_t C, void* ws, size_t ws_bytes, gcl_stream_t stream);
/* The same with the gradient written in a caller-given layout: d_delta[b, g, c] goes to d_delta + b * bsd_out +
 * g * ldd_out + c, and the columns C <= c < ldd_out of every row are written as zeros (ldd_out >= C, bsd_out >=
 * G * ldd_out).  Loss, gradient values, partial sums and their order are those of gcl_wmse_fwd_bwd. */
int gcl_wmse_fwd_bwd_ld(const float* delta, int64_t ldd, int64_t bsd, const float* x_last, int64_t ldx,
                        int64_t bsx, const float* y, int64_t ldy_, int64_t bsy, const float* node_w,
                        const float* chan_w, float inv_wsum, float grad_scale, float* d_delta, int64_t ldd_out,
                        int64_t bsd_out, float* out_state, const float* loss_prev, float* loss_out, int32_t B,
                        int32_t G, int32_t C, void* ws, size_t ws_bytes, gcl_stream_t stream);
size_t gcl_wmse_ws_bytes(int32_t B, int32_t G, int32_t C);

/* torch.optim.Adam step (src/main.py:212, src/train.py:233) over one flat parameter buffer:
 * grad_scale multiplies the gradient first (1/world after the gradient all-reduce). */
int gcl_adam_step(float* p, const float* g, float* m, float* v, int64_t count, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int32_t step, float grad_scale,
                  gcl_stream_t stream);

/* Same update with the step counter kept ON THE DEVICE (step_dev: one int32, incremented by the
 * call; bc_dev: two floats of scratch), so a captured hipGraph of the training step can be replayed
 * without any step-dependent host value baked into it. */
int gcl_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t count, float lr, float beta1,
                      float beta2, float eps, float weight_decay, int32_t* step_dev, float* bc_dev,
                      float grad_scale, gcl_stream_t stream);

/* torch.optim.Adam with parameter groups (src/main.py:190-211) over the flat bucket, every table on the device so
 * that a captured hipGraph replays it.  count: bucket length, a multiple of 64 (p, g, m, v 16-byte aligned); each
 * parameter owns whole 64-float chunks and chunk_param[count / 64] names the owner of each chunk.  Per parameter
 * (num_params entries): active (0 = frozen: its p, m, v and step are neither read nor written), lr, step (int32,
 * incremented by the call for active parameters) and bc (2 floats of scratch: the bias corrections of its step,
 * computed in double).  beta1, beta2, eps, weight_decay are shared by all groups; grad_scale multiplies the gradient
 * first.  With every parameter active at one step the result is bit-equal to gcl_adam_step.  Two launches; none, and
 * no step counted, when count or num_params is 0. */
int gcl_adam_step_groups(float* p, const float* g, float* m, float* v, int64_t count, const int32_t* chunk_param,
                         int32_t num_params, const int32_t* active, const float* lr, int32_t* step, float* bc,
                         float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                         gcl_stream_t stream);

/* Strided row copy  dst[b, i, 0:F] = src[b, i, 0:F]  (stage glue: src/models.py:837-838,860-862). */
int gcl_copy_rows(const float* src, int64_t lds, int64_t bss, float* dst, int64_t ldd, int64_t bsd,
                  int32_t B, int32_t rows, int32_t F, gcl_stream_t stream);

/* One whole GCNConv layer forward (src/models.py:419) in one kernel, aggregate-first:
 *   y[b,i,:] = (sum_{e in row i} w_e act(x[b, col_e, :])) W^T + bias
 * - the same value as gcl_linear_fwd followed by gcl_aggregate up to fp32 rounding (the aggregation is
 * linear), without the intermediate h in memory (csrc/gcn_layer.hip: wave-independent gather -> LDS tile ->
 * exact-fp32 MFMA -> 16-byte row stores).  Columns [Fout, Fout_store) of y are written as zeros
 * (Fout_store = Fout rounded up to a multiple of 4 keeps 33- / 19-wide outputs on 16-byte rows).
 * Needs Fin % 4 == 0, Fin, Fout_store <= 64, 16-B aligned rows of x and y, and a graph without heavy rows
 * (in-degree <= 64); other shapes use gcl_linear_fwd + gcl_aggregate. */
int gcl_gcn_layer_fwd(const gcl_graph_t* g, const float* x, int64_t ldx, int64_t bsx, int32_t act,
                      const float* slope, const float* W /*[Fout,Fin]*/, const float* bias, float* y,
                      int64_t ldy, int64_t bsy, int32_t B, int32_t Fin, int32_t Fout, int32_t Fout_store,
                      gcl_stream_t stream);
/* Same, computing only the first rows_out rows of every sample (rows beyond are not written): the decoder keeps
 * only the grid rows of its last conv (src/models.py:870-872), whose mesh rows are dead. */
int gcl_gcn_layer_fwd_rows(const gcl_graph_t* g, const float* x, int64_t ldx, int64_t bsx, int32_t act,
                           const float* slope, const float* W /*[Fout,Fin]*/, const float* bias, float* y,
                           int64_t ldy, int64_t bsy, int32_t B, int32_t Fin, int32_t Fout, int32_t Fout_store,
                           int32_t rows_out, gcl_stream_t stream);
/* The layer with a TWO-PART destination: rows i < head of sample b go to ya + b * bsa + i * lda, the others to
 * yb + b * bsb + (i - head) * ldb (two readers that each want their rows in a tensor of their own - the encoder output's
 * grid rows in the decoder's input, its mesh rows compact - get them without a copy).  The per-edge kernel stores one
 * 32-row tile per wave, so with head % 32 == 0 only a tile's store base differs: every row gets the bits
 * gcl_gcn_layer_fwd gives it.  gcl_gcn_layer_fwd_split_ok returns 1 when the call would run; it returns 0, and the call
 * GCL_EINVAL without writing anything, when head % 32 != 0, head <= 0 or head >= n, when a stride is no multiple of 4
 * floats, when a part exceeds 32-bit byte offsets, when Fin % 16 != 0 (the fp32-operand instantiations have no two-part
 * form), or when the source-tile form or the two-kernel fallback would take the layer (the caller then writes one
 * tensor and copies).  Query and call read one plan (csrc/tile_plan.h, plan_gcn_layer). */
int gcl_gcn_layer_fwd_split(const gcl_graph_t* g, const float* x, int64_t ldx, int64_t bsx, int32_t act,
                            const float* slope, const float* W /*[Fout,Fin]*/, const float* bias, float* ya, int64_t lda,
                            int64_t bsa, float* yb, int64_t ldb, int64_t bsb, int32_t head, int32_t B, int32_t Fin,
                            int32_t Fout, int32_t Fout_store, gcl_stream_t stream);
int gcl_gcn_layer_fwd_split_ok(const gcl_graph_t* g, int64_t ldx, int64_t bsx, int64_t lda, int64_t bsa, int64_t ldb,
                               int64_t bsb, int32_t head, int32_t B, int32_t Fin, int32_t Fout, int32_t Fout_store);
/* The layer with an OUTPUT-ROW predicate: rows i with present[i] < 0 may be left unwritten (a stage boundary behind the
 * layer drops them); rows with present[i] >= 0 get the bits gcl_gcn_layer_fwd gives them.  The source-tile form of the
 * layer folds the table into its stores; every other form stores all rows, which honours the same contract. */
int gcl_gcn_layer_fwd_present(const gcl_graph_t* g, const float* x, int64_t ldx, int64_t bsx, int32_t act,
                              const float* slope, const float* W, const float* bias, float* y, int64_t ldy, int64_t bsy,
                              const int32_t* present /*[n]*/, int32_t B, int32_t Fin, int32_t Fout, int32_t Fout_store,
                              gcl_stream_t stream);
/* Same layer with its input rows read THROUGH a row table instead of from a materialised [B, n, Fin] tensor (the
 * stage split of src/models.py:837-838 - `mesh_node_features = encoded[..., G:, :]` - folded into the first processor
 * layer's loads): input row i of sample b is row tab[i] of sample b of x when tab[i] >= 0, and row ~tab[i] of x viewed
 * as ONE flat list of x_rows rows (a batch-invariant row, shared by all samples) when tab[i] < 0.  Source-tile graphs
 * only (gcn_halo_fwd_kernel): GCL_EUNSUPPORTED otherwise; gcl_gcn_layer_fwd_tab_ok returns 1 when the call would run.
 * The query reads the launcher's plan (csrc/tile_plan.h, plan_gcn_layer) and its scalar argument checks.  It has no
 * ldy: for the n * ldy * 4 < 2^31 limit of the output it assumes the contiguous [B, n, roundup(Fout, 4)] tensor
 * (ldy = Fout_store = roundup(Fout, 4)); a caller with a wider ldy keeps that limit itself. */
int gcl_gcn_layer_fwd_tab(const gcl_graph_t* g, const float* x, int64_t ldx, int64_t bsx, int64_t x_rows,
                          const int32_t* tab /*[n]*/, int32_t act, const float* slope, const float* W /*[Fout,Fin]*/,
                          const float* bias, float* y, int64_t ldy, int64_t bsy, int32_t B, int32_t Fin, int32_t Fout,
                          int32_t Fout_store, gcl_stream_t stream);
int gcl_gcn_layer_fwd_tab_ok(const gcl_graph_t* g, int64_t ldx, int64_t bsx, int64_t x_rows, int32_t B, int32_t Fin,
                             int32_t Fout);

/* ---------------------------------------------------------------------------------------------
 * Edge-wise glue of the InteractionNet processor (src/models.py:206-236); csrc/interaction.hip.
 * Index arrays are int32 device arrays; rows are [.., D] with D % 4 == 0 and 16-B alignment.
 * ------------------------------------------------------------------------------------------- */
/* out[b,i,:] = sum (mean != 0: mean, empty segment -> 0) over k in [rowptr[i], rowptr[i+1]) of
 * src[b, perm ? perm[k] : k, :].  scatter(edge_update, receivers, reduce="mean")
 * (src/models.py:221) on receiver-sorted edges, and the backward of the x[senders] /
 * x[receivers] gathers (src/models.py:216). */
int gcl_segment_reduce(const float* src, int64_t ld_src, int64_t bs_src, const int32_t* perm,
                       const int32_t* rowptr /*[n+1]*/, int32_t mean, float* out, int64_t ld_out,
                       int64_t bs_out, int32_t B, int32_t n, int32_t D, gcl_stream_t stream);
/* out[b,e,:] = base[b,e,:] + extra[b,e,:] + A[b, ia[e], :] * sa[ia[e]] + C[b, ic[e], :]
 * (every operand optional; base / extra / out contiguous [B,E,D]).  Forward: the sender /
 * receiver terms of the first edge-MLP layer; backward: d(aggregated)[receivers] / deg. */
int gcl_edge_combine(const float* base, const float* extra, const float* A, int64_t lda, int64_t bsa,
                     const int32_t* ia, const float* sa, const float* C, int64_t ldc, int64_t bsc,
                     const int32_t* ic, float* out, int32_t B, int64_t E, int32_t D,
                     gcl_stream_t stream);
/* Elementwise activation where its output must exist in memory (edge_encoder, src/models.py:251):
 * y = act(x);  dx = dy * act'(x), PReLU adds its slope gradient into *d_slope. */
int gcl_act_fwd(const float* x, float* y, int64_t count, int32_t act, const float* slope,
                gcl_stream_t stream);
int gcl_act_bwd(const float* x, const float* dy, float* dx, int64_t count, int32_t act,
                const float* slope, float* d_slope, void* ws, size_t ws_bytes, gcl_stream_t stream);
size_t gcl_act_bwd_ws_bytes(void);

/* Input windows from a device-resident fp16 time series - the reference's on-the-fly loader
 * (src/data/dataloader_chunked.py:179-223: fp16 memmap (T, lon, lat, Ct) -> first C channels ->
 * fp32 -> (x - mean) / std -> (lat, lon)-major transpose -> [G, obs*C] / [G, pred*C]), batched over
 * B window starts t0[b] (device int64).  n_lat = 1, n_lon = N reads the flat (T, N, Ct) layout
 * (:184-197).  Bit-identical to the numpy loader; frames outside [0, T) come back as NaN. */
int gcl_window_pack(const uint16_t* series /* IEEE binary16 */, int64_t T, int32_t n_lon, int32_t n_lat,
                    int32_t Ct, const int64_t* t0, const float* mean, const float* stdv, int32_t C,
                    int32_t obs, int32_t pred, float* X /*[B,G,obs*C]*/, float* Y /*[B,G,pred*C] or NULL*/,
                    int32_t B, gcl_stream_t stream);

/* One autoregressive advance of the observation window, fused (scripts/predict.py:512-535 and the
 * same steps in src/train.py:203-228): step_out = residual ? x_last + delta : delta; static channels
 * (chan_kind 1) carry x_last forward, forcing channels (chan_kind 2) take y_step when it is given;
 * step_out is appended to `out` at column out_off (out may be NULL) and the window
 * state [B,G,obs,C] is shifted by one step into new_state (must not alias state).
 * state / delta / new_state are contiguous; y_step and out are addressed with (ld, bs). */
int gcl_ar_advance(const float* state, const float* delta, int64_t ldd, int64_t bsd, const float* y_step,
                   int64_t ldy, int64_t bsy, const int32_t* chan_kind, float* new_state, float* out,
                   int64_t ldo, int64_t bso, int32_t out_off, int32_t B, int32_t G, int32_t obs, int32_t C,
                   int32_t residual, gcl_stream_t stream);
/* Backward of one autoregressive TRAINING step = gcl_wmse_fwd_bwd (loss of the step, dd = d loss / d pred for a unit
 * upstream gradient) + gcl_ar_advance (src/train.py:203-228), in one pass:
 *   d_delta = g_loss dd + [predicted channel] g_new[last slot]
 *   d_state = shift(g_new) + last slot: [residual] g_loss dd + [static, or predicted with residual] g_new[last slot]
 * g_loss: device float (upstream gradient of the loss sum), g_new: gradient of the advanced window [B,G,obs,C] or NULL
 * (last step), d_state may be NULL (the first window is data).  All tensors contiguous. */
int gcl_ar_step_bwd(const float* dd, const float* g_loss, const float* g_new, const int32_t* chan_kind,
                    int32_t has_y, int32_t residual, float* d_delta, float* d_state, int32_t B, int32_t G,
                    int32_t obs, int32_t C, gcl_stream_t stream);
/* The same with dd read as dd + b * bsd + g * ldd + c and d_delta written as d_delta + b * bsd_out + g * ldd_out + c, the
 * columns C <= c < ldd_out of every row as zeros (g_new and d_state stay contiguous).  Without d_state only the last
 * window slot is visited.  Element for element the values of gcl_ar_step_bwd. */
int gcl_ar_step_bwd_ld(const float* dd, int64_t ldd, int64_t bsd, const float* g_loss, const float* g_new,
                       const int32_t* chan_kind, int32_t has_y, int32_t residual, float* d_delta, int64_t ldd_out,
                       int64_t bsd_out, float* d_state, int32_t B, int32_t G, int32_t obs, int32_t C,
                       gcl_stream_t stream);

/* dst[b, i, c] = (i < rows_src && c < F_src) ? src[b, i, c] : 0 for i < rows_dst, c < F_dst: the gradient of a row /
 * column slice (decoder output: grid rows, first 33 / 19 columns - src/models.py:870-872) widened to the sliced
 * tensor's zero-padded layout, in one pass. */
int gcl_pad_rows(const float* src, int64_t lds, int64_t bss, int32_t rows_src, int32_t F_src, float* dst,
                 int64_t ldd, int64_t bsd, int32_t rows_dst, int32_t F_dst, int32_t B, gcl_stream_t stream);
/* hipMemsetAsync(ptr, 0, nbytes) on the stream (optimizer.zero_grad of the flat gradient bucket, src/train.py:166). */
int gcl_zero(void* ptr, size_t nbytes, gcl_stream_t stream);

/* Row gather from up to two sources (stage glue of src/models.py:837-838,860-862 restricted to the
 * rows that matter):  dst[b,i,:] = a[b, map_a[i], :] if map_a[i] >= 0 (map_a NULL = identity), else
 * b[b, map_b[i], :] if map_b[i] >= 0, else 0.  A source with batch stride 0 is broadcast.
 * sum_batch == 1:  dst[0,i,:] = sum_b a[b, map_a[i], :]  (gradient of a broadcast source);
 * sum_batch = R > 1: the same sums, row i stored at dst[i / R, i % R, :] (R rows dealt to each destination sample).
 * Maps are int32 device arrays of length nd; F % 4 == 0 and 16-B aligned rows. */
int gcl_gather2_rows(const float* a, int64_t lda, int64_t bsa, const int32_t* map_a, const float* b,
                     int64_t ldb, int64_t bsb, const int32_t* map_b, float* dst, int64_t ldd, int64_t bsd,
                     int32_t B, int32_t nd, int32_t F, int32_t sum_batch, gcl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * ROI residual head (src/roi_residual.py): glue around the dense layers and the InteractionNet
 * processor of the correction head.
 * ------------------------------------------------------------------------------------------- */
/* Row gather from up to three sources into one zero-padded row (src/roi_residual.py:165-169, the
 * `torch.cat([X[roi], latent[roi], pred[roi]])` that builds the head's skip input):
 *   dst[b, i, :] = [s0[b, g, :w0] | s1[b, g, :w1] | s2[b, g, :w2] | 0 ...]  for i < n, g = rows[i]
 * (rows NULL: g = i), Fp columns in all, Fp % 4 == 0 (the dense kernels read 16-byte rows).  Each
 * source has its own row stride ld* and batch stride bs* (0 broadcasts), so a column block of a
 * wider tensor - the encoder's grid latents inside the compact pipeline's output - is read in place;
 * a source with width 0 is unused (may be NULL).  An index outside [0, rows_src) gives a zero row.
 * With one source this is also the backward of gcl_roi_compose: d_corr[b, i] = d_out[b, roi[i]]. */
int gcl_roi_gather_rows(const int32_t* rows, int32_t n, int32_t rows_src, const float* s0, int64_t ld0,
                        int64_t bs0, int32_t w0, const float* s1, int64_t ld1, int64_t bs1, int32_t w1,
                        const float* s2, int64_t ld2, int64_t bs2, int32_t w2, float* dst, int64_t ldd,
                        int64_t bsd, int32_t Fp, int32_t B, gcl_stream_t stream);
/* Output composition (src/roi_residual.py:183-185, `pred + zeros_like(pred).index_add(0, roi, corr)`):
 *   out[b, g, :] = pred[b, g, :] + corr[b, pos[g], :]  where pos[g] >= 0 (g is ROI row pos[g]),
 *   out[b, g, :] = pred[b, g, :]                        elsewhere (a copy: bit-equal to pred).
 * pos is an int32 device array of length G (the inverse of the ROI index list, -1 outside). */
int gcl_roi_compose(const float* pred, int64_t ldp, int64_t bsp, const float* corr, int64_t ldc, int64_t bsc,
                    const int32_t* pos, float* out, int64_t ldo, int64_t bso, int32_t B, int32_t G, int32_t C,
                    gcl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Dual-mesh regional model (src/dual_mesh.py): glue around the dense layers and the shared-step
 * InteractionNet processor of the regional module.
 * ------------------------------------------------------------------------------------------- */
/* Weighted segment sum over a CSR (the RegionalEncoder mean, src/dual_mesh.py:421-425, and the
 * RegionalDecoder inverse-distance sum, src/dual_mesh.py:464-468; their backward through the
 * transposed CSR with the same weights):
 *   out[b, i, :] (+)= addend[b, i, :] + sum_{k in [rowptr[i], rowptr[i+1])} w[k] * act(src[b, idx[k], :])
 * idx NULL: k itself; w NULL: weight 1; addend NULL: none; accumulate != 0 adds to out.  act is
 * GCL_ACT_NONE or GCL_ACT_SILU (applied to the source row as it is read).  An empty segment gives
 * the addend (or 0).  src, addend and out have unit channel stride and any 16-B aligned row / batch
 * stride, so out may be a column block of a wider row.  An index outside [0, n_src) contributes
 * nothing.  D % 4 == 0. */
int gcl_segment_wsum(const float* src, int64_t ld_src, int64_t bs_src, int32_t n_src, int32_t act,
                     const int32_t* idx, const float* w, const int32_t* rowptr, const float* addend,
                     int64_t ld_add, int64_t bs_add, float* out, int64_t ld_out, int64_t bs_out,
                     int32_t accumulate, int32_t B, int32_t n, int32_t D, gcl_stream_t stream);
/* Cross-message node update, global -> regional (src/dual_mesh.py:356-357,786-787):
 *   pre[b, i, :] = h[b, i, :] + (1 / deg_i) sum_{k in [rowptr[i], rowptr[i+1])} msg[b, k, :]  (0 for deg 0)
 *   y[b, i, :]   = LayerNorm_node(pre[b, i, :]) * gamma + beta,  stats[b * n + i] = (mean, rstd)
 * msg rows are the cross edges in receiver-sorted (CSR) order.  pre, y are dense [B, n, D], stats
 * [B * n, 2]; D % 4 == 0, D <= 256.  The backward is gcl_layernorm_bwd with x = pre, then
 * d msg[k] = d pre[rcv_k] / deg (gcl_edge_combine). */
int gcl_cross_update_fwd(const float* h, int64_t ld_h, int64_t bs_h, const float* msg, int64_t ld_msg,
                         int64_t bs_msg, const int32_t* rowptr, const float* gamma, const float* beta,
                         float eps, float* pre, float* y, float* stats, int32_t B, int32_t n, int32_t D,
                         gcl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Data assimilation (src/assimilation/): nudging and matrix-free optimal interpolation (OI).
 * ------------------------------------------------------------------------------------------- */
/* Nudging blend (src/assimilation/nudging.py:87-92 NudgingAssimilator.apply, form 0, and :201-206
 * nudge_sequence_offline, form 1):
 *   out[b, g, c] = f + c1 (o - f)   (form 0)  or  c0 f + c1 o   (form 1)   where o = obs[b, g, c] is
 *   not NaN and chan_mask[c] != 0 (chan_mask NULL: every channel);  out = f elsewhere.
 * float32 with one rounding per operation, no FMA: bit-equal to torch CPU for c0 = fl32(1 - alpha),
 * c1 = fl32(alpha).  Strided [B, G, C] views (unit channel stride); out may alias f. */
int gcl_nudge(const float* f, int64_t ldf, int64_t bsf, const float* obs, int64_t ldo, int64_t bso,
              const uint8_t* chan_mask, float c0, float c1, int32_t form, float* out, int64_t ldt,
              int64_t bst, int32_t B, int32_t G, int32_t C, gcl_stream_t stream);
/* The sequential form (form 0) of gcl_nudge with one setting per batch row (the DA grid search: every row of
 * one rollout carries another setting).  alpha[B] float32 (c1 of gcl_nudge, already rounded), net_of_row[B]
 * the row's station network or -1 (the row is copied to out, or left untouched when out == f); station_mask
 * uint8 [n_net][G], 1 = grid row g is a station of that network.  A value is nudged iff its row has a network,
 * station_mask[net][g] != 0, chan_mask[c] != 0 (NULL: every channel) and the observation is not NaN;
 * observations are read at stations only, so the truth can be passed once with bso = 0.  Same arithmetic
 * as gcl_nudge. */
int gcl_nudge_rows(const float* f, int64_t ldf, int64_t bsf, const float* obs, int64_t ldo, int64_t bso,
                   const uint8_t* station_mask, int32_t n_net, const int32_t* net_of_row, const float* alpha,
                   const uint8_t* chan_mask, float* out, int64_t ldt, int64_t bst, int32_t B, int32_t G,
                   int32_t C, gcl_stream_t stream);
/* Largest station count the OI factor accepts. */
int gcl_oi_max_stations(void);
/* OI station covariance (the `H @ B @ H.T + R + 1e-5 I` of src/assimilation/optimal_interpolation.py:
 * 120-126, built from coordinates instead of B): S[a, b] = sb2 exp(-rl2 theta_ab^2) + (a == b) diag,
 * float64 row-major m x m, theta the haversine angle of stations a, b (lat / lon in radians). */
int gcl_oi_station_cov(const double* lat, const double* lon, int32_t m, double sb2, double rl2,
                       double diag, double* S, gcl_stream_t stream);
/* In-place factor of S (m x m, float64) for gcl_oi_solve (replaces the per-channel
 * `torch.linalg.inv` of optimal_interpolation.py:122-124): root-free Cholesky S = U^T D U with the
 * unit factor inverted during the elimination; M then holds D on the diagonal, X = U^-T in the strict
 * lower triangle and X^T in the strict upper one.  m launches; no pivoting (S is SPD by construction). */
int gcl_oi_factor(double* M, int32_t m, gcl_stream_t stream);
/* W = S^-1 rhs = X^T D^-1 X rhs (optimal_interpolation.py:125-128, K @ innovation without K):
 * rhs, tmp float64 [n][m], W float32 [n][m] (station index contiguous).  Each column is independent
 * of the others and of n. */
int gcl_oi_solve(const double* M, int32_t m, const double* rhs, double* tmp, float* W, int32_t n,
                 gcl_stream_t stream);
/* Innovation gather (optimal_interpolation.py:127, `y_obs_val - H @ x_b`):
 *   rhs[b * nch + q][k] = obs[b, obs_row[k], chans[q]] - x_b[b, node_row[k], chans[q]]  (float64). */
int gcl_oi_innovation(const float* obs, int64_t ldo, int64_t bso, const float* xb, int64_t ldx,
                      int64_t bsx, const int32_t* obs_row, const int32_t* node_row, const int32_t* chans,
                      int32_t m, int32_t nch, int32_t B, double* rhs, gcl_stream_t stream);
/* OI analysis (optimal_interpolation.py:128 and :143, `x_b + K @ innovation` with B's columns
 * evaluated from coordinates): for every OI node i (grid row node_row[i], NULL: i) and column
 * col = b * nch + q,
 *   xa[b, row, chans[q]] = xb[b, row, chans[q]] + sum_k sb2 exp(-rl2 theta_ik^2) W[col][k]
 * in float32; pairs with |dlat| > th_cut or haversine a > a_cut contribute 0 (their weight underflows).
 * Only those entries are written: the caller copies the rest when xa != xb (xa may alias xb). */
int gcl_oi_analysis(const float* xb, int64_t ldx, int64_t bsx, float* xa, int64_t lda, int64_t bsa,
                    const int32_t* chans, int32_t nch, const int32_t* node_row, const double* nlat,
                    const double* nlon, const float* ncos, int32_t n_nodes, const double* slat,
                    const double* slon, const float* scos, const float* W, int32_t m, float sb2, float rl2,
                    float th_cut, float a_cut, int32_t B, gcl_stream_t stream);
/* gcl_oi_analysis with one (sb2, rl2) per sample: sb2_row[B], rl2_row[B] float32 device tables, sample
 * b = col / nch.  (th_cut, a_cut) are those of the longest correlation length among the samples; samples
 * with equal rl2 should be adjacent (the exponential is evaluated once per run of equal rl2 inside a block
 * of columns, the pair geometry once per block).  Every sample gets the bits gcl_oi_analysis gives it with
 * its own (sb2, rl2, th_cut, a_cut). */
int gcl_oi_analysis_rows(const float* xb, int64_t ldx, int64_t bsx, float* xa, int64_t lda, int64_t bsa,
                         const int32_t* chans, int32_t nch, const int32_t* node_row, const double* nlat,
                         const double* nlon, const float* ncos, int32_t n_nodes, const double* slat,
                         const double* slon, const float* scos, const float* W, int32_t m,
                         const float* sb2_row, const float* rl2_row, float th_cut, float a_cut, int32_t B,
                         gcl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Forecast scoring and global -> regional blending (scripts/predict.py, scripts/predict_pipeline.py).
 * ------------------------------------------------------------------------------------------- */
/* Workspace of gcl_verify_colstats for n rows, K columns, npred predictions, B samples. */
size_t gcl_verify_colstats_ws_bytes(int32_t n, int32_t K, int32_t npred, int32_t B);
/* Column statistics of StreamingMetrics.update (scripts/predict.py:53-122, the per-column loop at
 * :73-85 and the aggregate at :88-93; scripts/predict_pipeline.py:165-180): for every sample b,
 * prediction q < npred (1..4) and column k < K, over the n rows r = rows[i] (rows NULL: r = i),
 *   stats[((b * npred + q) * K + k) * 3 + 0] = sum (p - t)^2,   + 1 = sum |p - t|,
 *   + 2 = sum (t - tm)(p - pm) / (||t - tm|| ||p - pm|| + 1e-8)     (float64)
 * with t = truth[b * bst + r * ldt + k] and p = p_q[b * bs_q + r * ld_q + map_q[k]] (map_q NULL: k).
 * Fixed-order two-stage reduction (two kernels, no atomics): a column's result depends only on its
 * own data and n.  No allocation, no host synchronisation. */
int gcl_verify_colstats(const float* truth, int64_t ldt, int64_t bst, int32_t K, int32_t npred,
                        const float* p0, int64_t ld0, int64_t bs0, const int32_t* map0,
                        const float* p1, int64_t ld1, int64_t bs1, const int32_t* map1,
                        const float* p2, int64_t ld2, int64_t bs2, const int32_t* map2,
                        const float* p3, int64_t ld3, int64_t bs3, const int32_t* map3,
                        const int32_t* rows, int32_t n, int32_t B, double* stats, void* ws,
                        size_t ws_bytes, gcl_stream_t stream);
/* The accumulation of StreamingMetrics.update (scripts/predict.py:78-94): one job per metrics object,
 * jobs int64 [njobs][8] = {stats offset of the object's first column for sample 0 (doubles), doubles
 * between samples, columns, channels C, state offset (doubles), exclude-mask offset into masks
 * (bytes, -1: none), rows per column, samples}.  The state of an object is float64
 * [sum_se, sum_ae, n, total_elem, sum_se_per_ch[C], sum_acc[C], elem_per_ch[C], acc_count[C]];
 * each sample adds in the reference's order.  One launch for all objects (their states disjoint). */
int gcl_verify_accumulate(const double* stats, const int64_t* jobs, int32_t njobs, double* state,
                          const uint8_t* masks, gcl_stream_t stream);
/* Bilinear regrid (scripts/predict_pipeline.py:95-132 interpolate_global_to_region; scripts/
 * interpolate_to_region.py:64-73; the RegularGridInterpolator of scripts/evaluate_full_pipeline.py:
 * 134-145) with host-built tables: target i reads the source nodes n00 = cell[2i] * nlat +
 * cell[2i+1], n00 + 1, n00 + nlat, n00 + nlat + 1 with the float64 weights w[4i..4i+3] and
 *   g[b, i, k] = fp32(((v00 w0 + v01 w1) + v10 w2) + v11 w3)   (float64, each product rounded alone)
 * src float32 (src_f64 = 0) or float64 rows of stride lds.  With out != NULL also the taper blend of
 * scripts/predict_pipeline.py:326 in the same launch, out = m[i] r + (1 - m[i]) g (float32, no FMA);
 * g may be NULL then. */
int gcl_regrid_blend(const void* src, int32_t src_f64, int64_t lds, int64_t bss, int32_t nlat,
                     const int32_t* cell, const double* w, int32_t nt, int32_t K, float* g, int64_t ldg,
                     int64_t bsg, const float* mask, const float* r, int64_t ldr, int64_t bsr, float* out,
                     int64_t ldo, int64_t bso, int32_t B, gcl_stream_t stream);
/* Taper blend alone (scripts/predict_pipeline.py:326): out = m[i] r + (1 - m[i]) g, float32. */
int gcl_taper_blend(const float* mask, const float* r, int64_t ldr, int64_t bsr, const float* g,
                    int64_t ldg, int64_t bsg, float* out, int64_t ldo, int64_t bso, int32_t nt, int32_t K,
                    int32_t B, gcl_stream_t stream);

/* ---- MOS correction of t2m (csrc/mos.hip; src/postprocessing/mos_correction.py) ----
 * Forests are flattened HistGradientBoostingRegressors: 16-byte nodes {double v; uint32 left; uint32 meta}, meta =
 * right (bits 0-23) | feature << 24 | missing_go_to_left << 29 | is_leaf << 30, v the threshold or the leaf value;
 * roots[t] is the node index of tree t.  Predictions are rows pred[b * bs + g * gs + s * ss + c], float32 or float64
 * (f64 = 1), channels contiguous. */
/* sklearn's HistGradientBoostingRegressor.predict on n float64 rows X[n, 20] (the `model.predict` of
 * mos_correction.py:319): y[r] = ((baseline + v0) + v1) + ..., NaN follows missing_go_to_left. */
int gcl_mos_forest_eval(const void* nodes, const int32_t* roots, int32_t ntrees, double baseline, const double* X,
                        int32_t n, double* y, gcl_stream_t stream);
/* Station bias recurrence of apply_learned_mos_t2m (mos_correction.py:307-323 with the features of
 * _build_features_from_forecast :98-173): for every sample b and group q (stations group_start[q] ..
 * group_start[q+1] - 1 sharing grid row grid_idx[q]) and step s in order, each station's features (forecast ones
 * from channels c_* of the row, -1 = absent; host ones tfeat[b, station, s, 0..7] = hour sin / cos, doy sin / cos,
 * solar elevation, station lat / lon / elev; lags from the group's previous corrected t2m) go through the forest,
 * and bias[b, q, s] = numpy mean of the group.  feat_out[b, station, s, 20] (optional) receives the features.
 * n_corrected[b] (optional) is set to 0 for gcl_mos_idw_apply to count into.  At most 128 groups and 128 stations
 * per group. */
int gcl_mos_forest_predict(const void* nodes, const int32_t* roots, int32_t ntrees, double baseline,
                           const void* pred, int32_t pred_f64, int64_t bs, int64_t gs, int64_t ss, int32_t steps,
                           int32_t c_t2m, int32_t c_u, int32_t c_v, int32_t c_sp, int32_t c_tp,
                           const int32_t* grid_idx, const int32_t* group_start, int32_t ngroups, int32_t nst,
                           const double* tfeat, double* bias, double* feat_out, int32_t* n_corrected, int32_t B,
                           gcl_stream_t stream);
/* Spread and apply (mos_correction.py:187-241 _idw_interpolate_bias and :325-338): out[.., t2m] = in + field in
 * float64, rounded to the input's type.  idw = 1: field = the IDW of bias[b, k, s] over the K points pt_idx[k]
 * (haversine km from node_lat / node_lon, points within `radius`, weights 1 / max(d, 0.1)^power normalised; a
 * point's own row takes its bias), n_corrected[b] += rows with max |field| > 1e-6.  idw = 0: only the K point rows
 * change, n_corrected[b] += K.  out != in also copies every other element. */
int gcl_mos_idw_apply(const void* in, int32_t f64, int64_t bs, int64_t gs, int64_t ss, void* out, int64_t obs,
                      int64_t ogs, int64_t oss, int32_t G, int32_t steps, int32_t C, int32_t t2m,
                      const double* node_lat, const double* node_lon, const int32_t* pt_idx, int32_t K,
                      const double* bias, int32_t idw, double power, double radius, int32_t* n_corrected, int32_t B,
                      gcl_stream_t stream);
/* IDW parameter sweep (mos_correction.py:187-241, :326-338 as called by scripts/mos_idw_sweep.py:260-272 and
 * scripts/mos_idw_sweep_v2.py:288-299): the squared t2m error of P settings (power[p], radius[p]) - float64 device
 * arrays - in one launch, without the corrected forecasts.  For every setting p and row (b, g, s) the corrected value
 * y_p is bit for bit what gcl_mos_idw_apply writes for that setting (idw = 0: the station-only result for every p);
 * acc[p, h0 + s] += sum over b, g of (y_p - truth[b * tbs + g * tgs + s * tss])^2 with the difference and the square
 * in the forecast's type, each rounded on its own, and the sum in float64 in a fixed order (no floating-point atomics:
 * block partials in ws, then one fixed-order sum), so a repeated call repeats its bits.  acc is float64 [P, H].
 * fields_out (optional) [P, B, G, steps] in the forecast's type receives y_p; n_corrected (optional) int32 [P, B],
 * zeroed by the caller, counts as gcl_mos_idw_apply does.  ws holds gcl_mos_idw_sweep_ws_bytes(G, P, steps, B) bytes.
 * P above gcl_mos_idw_sweep_max_configs() and K above 128 are argument errors. */
size_t gcl_mos_idw_sweep_ws_bytes(int32_t G, int32_t P, int32_t steps, int32_t B);
int gcl_mos_idw_sweep_max_configs(void);
int gcl_mos_idw_sweep(const void* in, int32_t f64, int64_t bs, int64_t gs, int64_t ss, const void* truth, int64_t tbs,
                      int64_t tgs, int64_t tss, int32_t G, int32_t steps, int32_t t2m, const double* node_lat,
                      const double* node_lon, const int32_t* pt_idx, int32_t K, const double* bias, int32_t idw,
                      const double* power, const double* radius, int32_t P, double* acc, int32_t H, int32_t h0,
                      void* fields_out, int32_t* n_corrected, void* ws, size_t ws_bytes, int32_t B,
                      gcl_stream_t stream);
/* Table MOS (mos_correction.py:34-69 apply_mos_t2m): out[.., s, t2m] = in + step_bias[s] for s < nvalid, float32
 * f32(x + f32(b)) (numpy's weak Python-float scalar) or float64 x + b.  out != in also copies every other element. */
int gcl_mos_table_apply(const void* in, int32_t f64, int64_t bs, int64_t gs, int64_t ss, void* out, int64_t obs,
                        int64_t ogs, int64_t oss, int32_t G, int32_t steps, int32_t C, int32_t t2m,
                        const double* step_bias, int32_t nvalid, int32_t B, gcl_stream_t stream);

/* ---- Fitting the learned-MOS forest (csrc/mos_fit.hip; scripts/build_learned_mos.py:357-369) ----
 * The reference's `HistGradientBoostingRegressor(...).fit(X_train, y_train)` for squared error on rows without missing
 * values: histogram gradient boosting with a constant hessian of 1.  Features are binned into uint8 bins[F, ld]
 * (feature-major), histograms are two planes hist_sum float64 [F, 256] and hist_cnt uint32 [F, 256] (sum of hessians =
 * count), rows of a node are a segment [start, start + count) of the int32 partition array.  thr is float64 [F, 256]
 * (nthr[f] <= 255 used per feature).  No floating-point atomics: a repeated call repeats its bits.  Every workspace
 * holds gcl_mos_fit_ws_bytes(n, n_val, F, max_leaf_nodes, max_iter) bytes (n >= start + count for the segment calls;
 * max_leaf_nodes 2 .. 256, F <= 32; 0 for arguments outside that). */
size_t gcl_mos_fit_ws_bytes(int32_t n, int32_t n_val, int32_t F, int32_t max_leaf_nodes, int32_t max_iter);
/* build_learned_mos.py:357-369, sklearn's _BinMapper.transform: bins[f, i] = #{k < nthr[f] : thr[f, k] < X[i, f]}, so a
 * value equal to a threshold goes left.  X float64 [n, F] without NaN. */
int gcl_mos_fit_bin(const double* X, int32_t n, int32_t F, const double* thr, const int32_t* nthr, void* bins,
                    int64_t ld, gcl_stream_t stream);
/* build_learned_mos.py:357-369, the half squared error's gradient: g[i] = float32(raw[i] - y[i]), the difference in
 * float64. */
int gcl_mos_fit_gradients(const double* raw, const double* y, float* g, int32_t n, gcl_stream_t stream);
/* build_learned_mos.py:357-369, sklearn's compute_histograms_brute: hist[f, b] = {sum of g[row], number of rows} over
 * the rows part[start .. start + count) with bins[f, row] == b.  The rows of at most 256 row ranges are added one
 * after the other, then the ranges in order. */
int gcl_mos_fit_histogram(const void* bins, int64_t ld, int32_t F, const int32_t* part, const float* g, int32_t start,
                          int32_t count, double* hist_sum, void* hist_cnt, void* ws, size_t ws_bytes,
                          gcl_stream_t stream);
/* build_learned_mos.py:357-369, sklearn's compute_histograms_subtraction: large = parent - small, element-wise. */
int gcl_mos_fit_hist_subtract(const double* parent_sum, const void* parent_cnt, const double* small_sum,
                              const void* small_cnt, double* large_sum, void* large_cnt, int32_t F,
                              gcl_stream_t stream);
/* build_learned_mos.py:357-369, sklearn's find_node_split (left-to-right scan): the best split of a node of n rows and
 * gradient sum sum_g.  A candidate "bins <= b go left" needs both sides >= min_samples_leaf; value(g, h) = -g / (h + l2
 * + 1e-15), gain = g_P v_P - g_L v_L - g_R v_R in that order; only a strictly larger gain replaces the best (lowest bin,
 * then lowest feature).  out = {gain (-1: no split), sum_g_left}, iout = {feature, bin, n_left, missing_go_to_left =
 * n_left > n_right}, both on the device. */
int gcl_mos_fit_split(const double* hist_sum, const void* hist_cnt, int32_t F, const int32_t* nthr, int32_t n,
                      double sum_g, int32_t min_samples_leaf, double l2, double* out, int32_t* iout, void* ws,
                      size_t ws_bytes, gcl_stream_t stream);
/* build_learned_mos.py:357-369, sklearn's split_indices: the stable partition of part[start .. start + count) by
 * bins[feat, row] <= bin (left rows first, both sides in their old order).  *n_left (device, optional) receives the
 * left side's length. */
int gcl_mos_fit_partition(const void* bins, int64_t ld, int32_t* part, int32_t start, int32_t count, int32_t feat,
                          int32_t bin, int32_t* n_left, void* ws, size_t ws_bytes, gcl_stream_t stream);
/* build_learned_mos.py:357-369, the early-stopping score of the squared error: *score = -0.5 mean((raw - y)^2) in
 * float64, summed in a fixed order.  ws as for n_val = n. */
int gcl_mos_fit_score(const double* raw, const double* y, int32_t n, double* score, void* ws, size_t ws_bytes,
                      gcl_stream_t stream);
/* build_learned_mos.py:357-369, one boosting iteration (sklearn's TreeGrower.grow with the histogram, split and
 * partition rules above): gradients from raw and y, a tree grown best-first (the splittable leaf with the largest gain
 * next; max_leaf_nodes; children at max_depth and nodes of fewer than 2 min_samples_leaf rows are leaves; only the
 * smaller child's histogram is built, the right one on a tie, the other is parent - smaller), leaf values times
 * learning_rate.  The tree is appended to `nodes` (16-byte MOSForest nodes with numeric thresholds, children after
 * their parent) at node state[1], roots[state[0]] = state[1]; raw[row] += leaf value for every training row; the n_val
 * validation rows (bins_val, may be 0 rows) walk the tree into raw_val and scores[state[0] + 1] = the score of
 * gcl_mos_fit_score; then state[0] += 1, state[1] += the tree's nodes.  state is int32 [2] on the device, zeroed by the
 * caller before the first tree; a call with state[0] >= max_iter changes nothing.  The launch sequence depends on the
 * arguments only, never on the data (it can be captured); nothing is read back. */
int gcl_mos_fit_tree(const void* bins, int64_t ld, int32_t n, int32_t F, const int32_t* nthr, const double* thr,
                     const double* y, double* raw, const void* bins_val, int64_t ld_val, int32_t n_val,
                     const double* y_val, double* raw_val, int32_t max_leaf_nodes, int32_t max_depth,
                     int32_t min_samples_leaf, double l2, double learning_rate, int32_t max_iter, void* nodes,
                     int32_t* roots, double* scores, int32_t* state, void* ws, size_t ws_bytes, gcl_stream_t stream);

/* ---- Multi-resolution input (csrc/multires.hip) ----
 * Windows of the flat multires node set - the n_kept global points outside the box in (lat, lon)-major order, then
 * n_reg regional points - packed from the device-resident fp16 series without the flat series ever existing.  Replaces
 * scripts/build_multires_dataset.py:151-234 (build_interpolate_mode) / :270-345 (build_merge_mode) followed by the
 * flat branch of src/data/dataloader_chunked.py:186-200, and scripts/evaluate_full_pipeline.py:113-144
 * (build_multires_frame) with the z-score of :463.
 *   gseries (Tg, n_lon, n_lat, Ctg); rank[lat * n_lon + lon] = output row of a global point or -1 (removed).
 *   rseries != NULL (merge): regional rows are rseries (Tr, rn_lon, rn_lat, Ctr) in (lat, lon)-major order.
 *   rseries == NULL (interpolate): regional row i is the bilinear value of the global frame at its four corners
 *     corner[i, 0..3] (positions lon * n_lat + lat) with float64 weights w[i, 0..3], added in that order onto 0.0 in
 *     float64 with every product rounded on its own (scipy RegularGridInterpolator((lats, lons)), float32 values), then
 *     rounded to float32 and, with quantize = 1, through float16 (what the builder stores and the loader reads back).
 *   Window b holds the frames t0[b] + off_g (global) / t0[b] + off_r (regional) + 0 .. obs + pred - 1; a frame outside
 *   its series comes back as NaN.  mean / stdv (both or neither): (x - mean[c]) / std[c] in float32 on the first C
 *   channels.  out_f16 = 1: X / Y are binary16 buffers.  X [B, n_kept + n_reg, obs * C], Y [.., pred * C] or NULL. */
int gcl_multires_window_pack(const uint16_t* gseries, int64_t Tg, int32_t n_lon, int32_t n_lat, int32_t Ctg,
                             const uint16_t* rseries, int64_t Tr, int32_t rn_lon, int32_t rn_lat, int32_t Ctr,
                             const int32_t* rank, int32_t n_kept, int32_t n_reg, const int32_t* corner,
                             const double* w, const int64_t* t0, int64_t off_g, int64_t off_r, const float* mean,
                             const float* stdv, int32_t C, int32_t obs, int32_t pred, int32_t quantize,
                             int32_t out_f16, void* X, void* Y, int32_t B, gcl_stream_t stream);

/* ---- Full-pipeline evaluation glue (csrc/pipeline.hip; scripts/evaluate_full_pipeline.py:449-666) ----
 * ROI rows in physical units (:502-511, :545): raw[g, c] = v * std[c] + mean[c] in float32, product and sum rounded
 * separately, v = pred[r, c] (+ x_last[r, c] first when x_last is given), r = rows[g] or row0 + g when rows is NULL;
 * lapse (optional) = raw with column t_idx replaced by t2m + (z_surf - elev) * 6.5e-3 from the row's own z_idx column
 * (t_idx = z_idx = -1: plain copy).  lapse_f64 = 0: every step in float32 (numpy with a Python-float elevation);
 * 1: difference and product in float64, (double) t2m + delta rounded to float32 once (an np.float64 elevation). */
int gcl_pipeline_roi_phys(const float* pred, int64_t ldp, const float* x_last, int64_t ldx, const int32_t* rows,
                          int32_t row0, int32_t G, int32_t C, const float* mean, const float* stdv, int32_t t_idx,
                          int32_t z_idx, double elev, int32_t lapse_f64, float* raw, float* lapse,
                          gcl_stream_t stream);
/* apply_lapse (:184-200) on contiguous in [G, S, C] -> out (must not alias): column t_idx of every step corrected
 * with z_idx of step 0; lapse_f64 as above. */
int gcl_pipeline_lapse(const float* in, float* out, int32_t G, int32_t S, int32_t C, int32_t t_idx, int32_t z_idx,
                       double elev, int32_t lapse_f64, gcl_stream_t stream);
/* apply_lapse_correction of scripts/mos_idw_sweep_v2.py:73-84 on contiguous in [G, S, C] -> out (must not alias):
 * column t_idx of every step becomes t2m + f32(6.5e-3 * f32(f32(z / 9.80665) - elev)), z the geopotential in column
 * z_idx of step 0, elev a Python float there: every operation float32, each rounded on its own. */
int gcl_pipeline_lapse_geopotential(const float* in, float* out, int32_t G, int32_t S, int32_t C, int32_t t_idx,
                                    int32_t z_idx, double elev, gcl_stream_t stream);
/* simulate_station_obs (:203-222): obs [G, C] = truth rows at the S grid points stn[], NaN elsewhere. */
int gcl_pipeline_station_obs(const float* truth, int64_t ldt, const int32_t* stn, int32_t S, int32_t G, int32_t C,
                             float* obs, gcl_stream_t stream);
/* Error sums of V variants preds[v * vs + g * ldp + c] against truth (:644-652) at horizon h:
 * acc_grid[v, h, c] += sum_g (p - t)^2, acc_stn[v, h, c] (optional) += the same over the rows stn[0..S) as listed.
 * Difference and square in float32, sums in float64 in a fixed order (no atomics); C <= 256. */
int gcl_pipeline_sqerr(const float* preds, int64_t vs, int64_t ldp, int32_t V, const float* truth, int64_t ldt,
                       const int32_t* stn, int32_t S, int32_t G, int32_t C, int32_t H, int32_t h, double* acc_grid,
                       double* acc_stn, gcl_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Per-grid-point error maps (csrc/maps.hip; scripts/metrics_maps.py).
 * Shared arguments: truth[b * bst + r * ldt + k] and pred[b * bsp + r * ldp + pmap[k]] (pmap NULL: k)
 * for the n scored rows r = rows[i] (rows NULL: r = i) and the columns k = lead * C + c.  Every value
 * is converted to physical units on its own in float32, in the order of inverse_standardize
 * (scripts/metrics_maps.py:40-44) and apply_units (:65-73), each operation rounded alone:
 *   v = x * conv[4k];  v = v + conv[4k+1]   (flags[k] & 1)
 *   v = v / 9.80665f                        (flags[k] & 2, true division)
 *   v = v * conv[4k+2];  v = v + conv[4k+3]
 * conv == NULL (then flags == NULL too): values are used as they are.
 * ------------------------------------------------------------------------------------------- */
/* Workspace of gcl_maps_colstats for n rows, K columns, B samples. */
size_t gcl_maps_colstats_ws_bytes(int32_t n, int32_t K, int32_t B);
/* The per-sample field statistics of compute_stat's ACC branch (scripts/metrics_maps.py:84-89,
 * `pred.mean(dim=1)` / `pred.std(dim=1)`): cs[(b * K + k) * 4 + {0: mean_p, 1: std_p, 2: mean_t,
 * 3: std_t}] over the n scored rows of the converted values, float64, std unbiased (n == 1: NaN, as
 * torch.std).  Sums shifted by the column's first scored row; two kernels, fixed order, no atomics: a
 * column's result depends only on its own data and n. */
int gcl_maps_colstats(const float* truth, int64_t ldt, int64_t bst, const float* pred, int64_t ldp,
                      int64_t bsp, const int32_t* pmap, int32_t K, const float* conv, const int32_t* flags,
                      const int32_t* rows, int32_t n, int32_t B, double* cs, void* ws, size_t ws_bytes,
                      gcl_stream_t stream);
/* The sums behind compute_stat (scripts/metrics_maps.py:75-90), streamed: for every element (lead, i,
 * c) the B samples are added in sample order into state[(lead * nsums + s) * n * C + i * C + c]
 * (float64), s counting the set bits of `sums` in ascending order: 1 sum e, 2 sum e^2, 4 sum |e|,
 * 8 sum p^ t^ with e = (double)vp - (double)vt, p^ = (vp - mean_p) / (std_p + 1e-8), t^ likewise (cs
 * of gcl_maps_colstats, needed only with bit 8).  At most 2^31 - 1 elements (leads * n * C) per call.  *count (device) += B.  One thread owns an element:
 * no atomics; 16-byte loads when rows are exactly K floats, unmapped and aligned. */
int gcl_maps_accumulate(const float* truth, int64_t ldt, int64_t bst, const float* pred, int64_t ldp,
                        int64_t bsp, const int32_t* pmap, int32_t leads, int32_t C, const float* conv,
                        const int32_t* flags, const int32_t* rows, int32_t n, int32_t B, const double* cs,
                        int32_t sums, double* state, int64_t* count, gcl_stream_t stream);
/* State -> float32 map out[lead * nelem + e] from sum `plane` of `nsums` (scripts/metrics_maps.py:
 * 78-89 with N = *count): kind 0 rmse = sqrt(S / N), 1 mae, 2 bias, 3 acc = S / N; N == 0 gives 0.
 * kind 4: skill = 1 - rmse / max(rmse_ref, 1e-9) per element from the two float32 RMSE values (the
 * clip of scripts/eval_real_freeze6.py:178-180), `plane` / `ref_plane` being the sum-e^2 planes. */
int gcl_maps_finalize(const double* state, const int64_t* count, int32_t plane, int32_t nsums,
                      int32_t leads, int64_t nelem, int32_t kind, const double* ref_state,
                      const int64_t* ref_count, int32_t ref_plane, int32_t ref_nsums, float* out,
                      gcl_stream_t stream);
/* inverse_standardize / apply_units alone (scripts/metrics_maps.py:40-44, :65-73) on `total`
 * contiguous values whose column is index % K: out = converted x (out may alias x). */
int gcl_maps_convert(const float* x, float* out, int64_t total, int32_t K, const float* conv,
                     const int32_t* flags, gcl_stream_t stream);

/* ---- Live forecast glue (csrc/live.hip; scripts/live_gdas_forecast.py) ----
 * One analysis cycle into window slots (:378-407 build_interpolator / interp_to_nodes, :460-483
 * extract_live_channels, :486-487 normalize_frame, :617-620): all C channels of all G nodes in one launch, the
 * channel the fastest index of a thread's work.  chan [C, 3] (device): kind 0 = zero fill, 1 = source field at arena
 * + chan[c, 1] using point table chan[c, 2], 2 = static template row chan[c, 1] of statics [n_static, G].  pos / w
 * [n_tab, G, 4]: per node the four positions into the field as the source stores it (unsorted, without the wrap
 * column) and their float64 weights, corners (lat, lon), (lat, lon+1), (lat+1, lon), (lat+1, lon+1).  A field value is
 * the four products, each rounded on its own, added in that order onto 0.0 in float64 (what scipy's
 * RegularGridInterpolator does on float32 values), rounded to float32 and divided by chan_div[c] in float32 (:480-481,
 * 100 for msl / sp).  Every channel is then z-scored, (x - mean[c]) / std[c] in float32 with the subtraction and the
 * division rounded separately, and stored at out + dest_off[d] + g * ldo + c for every d < nd.  dest_off is a HOST
 * array of nd <= gcl_live_max_dest() element offsets (it travels in the kernel arguments); the caller guarantees that
 * every position lies inside its field and every destination inside out.  No atomics; arena / pos / w may be NULL
 * together when no channel is a field. */
int gcl_live_max_dest(void);
int gcl_live_frame_pack(const float* arena, const float* statics, const int64_t* chan, const float* chan_div,
                        const int32_t* pos, const double* w, const float* mean, const float* stdv, float* out,
                        const int64_t* dest_off, int32_t nd, int64_t ldo, int32_t G, int32_t C,
                        gcl_stream_t stream);
/* The city-box summary (:543-559 summarize_city): out [B, S, nc, 3] float64 = mean, min, max over the n rows `rows`
 * of v = pred[b, rows[i], s, chans[k]] (+ offs[k] in float32 when offs[k] != 0: -273.15 for t2m, :552-553).  pred is
 * float32 with unit channel stride and element strides bs, gs, ss.  One block per (b, s, k), rows reduced in a fixed
 * order: the mean is a float64 sum of the float32 values over n, min / max the float32 values (NaN propagates).
 * n == 0 is an argument error (the reference writes no city block then).  The caller guarantees 0 <= rows[i] < G and
 * 0 <= chans[k] < C: both are device arrays the entry point cannot read. */
int gcl_live_region_stats(const float* pred, int64_t bs, int64_t gs, int64_t ss, const int32_t* rows, int32_t n,
                          const int32_t* chans, const float* offs, int32_t nc, int32_t S, double* out, int32_t B,
                          gcl_stream_t stream);

/* ---- Building, repairing and extending datasets (csrc/dataset.hip) ----
 * The arithmetic core of scripts/build_dataset_512x256.py, recompute_wb2_scalers.py, repair_dataset.py,
 * add_time_features.py and check_23f_data.py on the fp16 series (T, n_lon, n_lat, Ct) in device memory; n_lat = 1 is
 * the flat (T, N, Ct) layout.  No entry point allocates or synchronises; offsets are int64; no floating-point atomics;
 * every reduction has two stages with a fixed order (a block's share of the data and the order of the partial records
 * follow from the shapes alone), so a result depends only on the data and the shapes.  `ws` is a device scratch buffer
 * of at least gcl_dataset_ws_bytes(Ct) bytes, the caller's until the call has run. */
size_t gcl_dataset_ws_bytes(int32_t C);
/* The most sources one gcl_dataset_pack call takes (they travel in the kernel arguments). */
int gcl_dataset_max_sources(void);
/* One time block into the series, with the block's sums (scripts/build_dataset_512x256.py:288-324, the repair of
 * scripts/repair_dataset.py:163-184, and with series == NULL the statistics alone of
 * scripts/recompute_wb2_scalers.py:71-79).  src / tstride / chan / scale are HOST arrays of nsrc entries: src[j] a
 * device float32 plane [nt, P], P = n_lon * n_lat in (time, lon, lat) order, whose time steps are tstride[j] elements
 * apart (0: a time-invariant field, the expand_dims of :159-166 without the copy).  v = x * scale[j] rounded to float32
 * on its own (numpy's `arr *= 0.01`; 1.0f leaves the bits), series[t0 + t, p, chan[j]] = fp16(v) round to nearest even
 * (overflow to +-inf, subnormals kept: ndarray.astype(np.float16)), sum[chan[j]] = sum of (double)v and sumsq[chan[j]]
 * = sum of (double)(float)(v * v) - the square rounded to float32 first, as (arr * arr).sum(dtype=np.float64) has it.
 * NaN and inf reach the sums as in numpy.  Channels are distinct.  With all Ct channels listed the block is one
 * contiguous span, staged through LDS and written with 16-byte stores; with fewer, the bytes of the other channels and
 * their entries of sum / sumsq are not touched. */
int gcl_dataset_pack(const float* const* src, const int64_t* tstride, const int32_t* chan, const float* scale,
                     int32_t nsrc, int32_t nt, int32_t n_lon, int32_t n_lat, uint16_t* series, int64_t T, int32_t Ct,
                     int64_t t0, double* sum, double* sumsq, void* ws, size_t ws_bytes, gcl_stream_t stream);
/* Per-channel statistics of rows [t_s, t_e) of a series (the resume pass scripts/build_dataset_512x256.py:238-253,
 * the good channels of scripts/repair_dataset.py:142-147, the scaler pass of scripts/add_time_features.py:111-121, the
 * printouts of scripts/check_23f_data.py): sum and sumsq of v = (float)h by the rounding rule of gcl_dataset_pack,
 * vmin / vmax over the finite values (+inf / -inf when there is none), and the counts of NaN and of +-inf.  flags
 * bit 0: NaN counts as 0 in the sums, bit 1: +-inf does (repair_dataset.py:144 sets both); the counts and min / max do
 * not depend on the flags. */
int gcl_dataset_stats(const uint16_t* series, int64_t T, int32_t n_lon, int32_t n_lat, int32_t Ct, int64_t t_s,
                      int64_t t_e, int32_t flags, double* sum, double* sumsq, float* vmin, float* vmax,
                      int64_t* n_nan, int64_t* n_inf, void* ws, size_t ws_bytes, gcl_stream_t stream);
/* welford_update (scripts/build_dataset_512x256.py:126-136) for C channels, state mean[C], m2[C] and *n on the
 * device, block_sum / block_sumsq device arrays (what the two entry points above leave): the operations of the numpy
 * expression in its order, each rounded alone in float64.  One thread per channel. */
int gcl_dataset_welford(double* mean, double* m2, int64_t* n, const double* block_sum, const double* block_sumsq,
                        int64_t block_n, int32_t C, gcl_stream_t stream);
/* dst (T, P, Ct_new) from src (T, P, Ct_old): the old channels bit for bit, channel Ct_old + k of every point of
 * time step t = extra[t, k] (fp16 bits, [T, Ct_new - Ct_old]) - scripts/add_time_features.py:94-101. */
int gcl_dataset_widen(const uint16_t* src, int64_t T, int32_t n_lon, int32_t n_lat, int32_t Ct_old,
                      const uint16_t* extra, int32_t Ct_new, uint16_t* dst, gcl_stream_t stream);

/* ---- The WRF benchmark (csrc/wrf.hip; scripts/compare_wrf_era5.py, scripts/compare_wrf.py) ----
 * No entry point allocates or synchronises; no floating-point atomics; every reduction has a fixed order, so a result
 * has the same bits on every run.  A point table is pos int32 [P, 4] / w float64 [P, 4]: per WRF point the node numbers
 * of the corners (lon, lat), (lon, lat+1), (lon+1, lat), (lon+1, lat+1) of its source cell and their weights
 * (1 * w_lon) * w_lat; pos[4 i] < 0 marks a point outside the source axes.  A source is float32 (half = 0) or fp16
 * (half = 1, widened exactly); node p of the field at element offset `off` is read at off + p * node_stride, so a
 * channel of a (T, n_lon, n_lat, C) series and a column of an [n, G, P * C] forecast are read in place.  The caller
 * guarantees that every position lies inside its field.
 *
 * interpolate_era5_to_wrf (compare_wrf_era5.py:127-152) for nf fields: out [nf, P] float64, out[f, i] = the four
 * products (double)v_k * w_k, each rounded on its own, added in corner order onto 0.0 - scipy's
 * RegularGridInterpolator on float32 values - or NaN outside (bounds_error=False, fill_value=nan).  With mul / add
 * (device float32 [nf], both or neither) v = x * mul[f], then v + add[f], each rounded in float32 first: the
 * denormalisation of compare_wrf.py:162.  field_off: device int64 [nf]. */
int gcl_wrf_sample(const void* src, int32_t half, int64_t node_stride, const int64_t* field_off, const float* mul,
                   const float* add, int32_t nf, const int32_t* pos, const double* w, int32_t P, double* out,
                   gcl_stream_t stream);
/* compute_metrics (compare_wrf_era5.py:155-164) for J jobs over the same P points, nothing sampled being stored.
 * jobs: device int64 [J, 6] = kind a, offset a, kind b, offset b, gated, delta; conv: device float32 [J, 4] = mul a,
 * add a, mul b, add b.  kind & 3: 0 = a point field pts[offset + i] (float32; with kind & 4 times mul, rounded in
 * float32: WRF psfc_Pa * 0.01, :247), 1 / 2 = a field of source 0 / 1 at that element offset, sampled as
 * gcl_wrf_sample samples it (kind & 4: with the conversion), 3 = a float64 point field pts64[offset + i] as it is
 * (a field gcl_wrf_sample left).  d = a - b in float64 over the points where neither side
 * is NaN (infinities stay, as in the reference); a job yields {n, sum d, sum d^2, sum |d|, sum a, sum b}: 256 points
 * per block combined in a fixed order, the blocks of a job added in order.  The J jobs fill S slots, job j slot j % S
 * (J = S * samples): stats [S, 6] float64 = (accumulate ? stats : 0) + the slot's jobs in job order.  A gated job
 * counts only when offsets[j / S] (device int64, one per sample) == target + delta and filled[slot] (device int32 [S])
 * is still 0, which it then sets: the first sample at that offset (compare_wrf.py:670-681).  offsets / filled may be
 * NULL when no job is gated.  ws: at least gcl_wrf_scores_ws_bytes(J, P) bytes of device scratch. */
size_t gcl_wrf_scores_ws_bytes(int32_t J, int32_t P);
int gcl_wrf_scores(const void* src0, int32_t half0, int64_t stride0, const int32_t* pos0, const double* w0,
                   const void* src1, int32_t half1, int64_t stride1, const int32_t* pos1, const double* w1,
                   const float* pts, const double* pts64, const int64_t* jobs, const float* conv, int32_t J,
                   int32_t S, int32_t P, const int64_t* offsets, int64_t target, int32_t* filled, int32_t accumulate,
                   double* stats, void* ws, size_t ws_bytes, gcl_stream_t stream);
/* pred_region.mean(axis=1) of compare_wrf.py:160-170, :202-203, :385-386: out[first + s, k], k < K = P * C, = the
 * float32 sum over the R listed rows in their listed order of x[s, rows[r], k] * stdv[k % C] + mean[k % C] (product
 * and sum rounded separately, no FMA), divided by (float)R - the order of numpy's float32 reduction over a non-last
 * axis.  x float32 with unit column stride and element strides bs, gs; out rows ldo apart; first = *count (device
 * int64) or 0 when count is NULL; rows at or past `cap` are not written.  One thread per (s, k).  R == 0 is an
 * argument error.  The caller guarantees 0 <= rows[r] < G. */
int gcl_wrf_box_means(const float* x, int64_t bs, int64_t gs, const int32_t* rows, int32_t R, const float* stdv,
                      const float* mean, int32_t C, int32_t K, int32_t B, float* out, int64_t ldo,
                      const int64_t* count, int64_t cap, gcl_stream_t stream);

/* ---- The downscaler data layer (csrc/downscale.hip; scripts/build_downscaler_dataset.py,
 * scripts/generate_gnn_predictions.py, DownscalerDataset and compute_metrics of scripts/train_downscaler.py) ----
 * No entry point allocates or synchronises; no floating-point atomics; every reduction has a fixed order.  A point
 * table is pos int32 [P, 4] / w float64 [P, 4] in OUTPUT order (p = j * n_lat_f + i, the lon-first storage): the node
 * rows of the four corners of a point's source cell and their weights, in the corner order of the interpolator that
 * is reproduced.  The caller guarantees that every position lies inside its source.  An archive is fp16
 * (T, n_lon, n_lat, C); a frame is one contiguous span of P * C halves, which may start off a 16-byte boundary.
 *
 * build_downscaler_dataset.py:137-157 for frames t0 .. t0 + nt - 1 of `series` (fp16, T frames of N nodes, node
 * lon * n_lat + lat): out[to0 + t, p, c] = the four corner values widened exactly to float64, each times its weight
 * (every product rounded on its own, a zero weight included: 0 * inf = NaN), added in corner order onto 0.0, and that
 * float64 rounded to binary16 ONCE (nearest even, overflow to +-inf, subnormals kept), as
 * ndarray.astype(np.float16) does.  pos == w == NULL (then P == N): the frames are copied bit for bit (:125-127).
 * A frame holds fewer than 2^32 halves (N * C), N fewer than 2^31 nodes. */
int gcl_downscale_coarse(const uint16_t* series, int64_t T, int64_t N, int32_t C, const int32_t* pos, const double* w,
                         int64_t P, int64_t t0, int64_t nt, uint16_t* out, int64_t T_out, int64_t to0,
                         gcl_stream_t stream);
/* generate_gnn_predictions.py:226-254 for B samples: v = pred[b, g, c] (float32, element strides bs / gs, unit
 * channel stride), with `last` (its own strides lbs / lgs) v = last + pred rounded in float32; the float64 corner
 * sum of gcl_downscale_coarse over the node rows of the table, rounded to float32; times stdv[c], plus mean[c], each
 * rounded in float32 (no FMA); rounded to fp16 into out[dest[b], p, c].  dest: device int64 [B]; a sample whose dest is
 * below 0 or at or past T_out is skipped and its frame keeps its bytes (the t_pred < T rule of :249). */
int gcl_downscale_pred(const float* pred, int64_t bs, int64_t gs, const float* last, int64_t lbs, int64_t lgs,
                       const int32_t* pos, const double* w, int64_t P, int32_t C, int32_t B, const float* stdv,
                       const float* mean, const int64_t* dest, uint16_t* out, int64_t T_out, gcl_stream_t stream);
/* DownscalerDataset.__getitem__ (train_downscaler.py:137-183) for B samples, t: device int64 [B].  coarse / fine:
 * archives (T, W = n_lon, H = n_lat, C), C <= 64.  X float32 [B, obs * C + Ns, H, W]: frames t - obs + 1 .. t of
 * coarse in order, every value (x - mean[c]) / (std[c] + 1e-8f) with the sum, the difference and the quotient each
 * rounded in float32, then X[b, obs * C + s, h, w] = stat[w, h, s] (float32 [W, H, Ns], as it is; stat NULL when
 * Ns == 0).  Y float32 [B, C, H, W]: frame t of fine, normalised alike.  flip (device int32 [B] or NULL) != 0 mirrors
 * X and Y in w, and the channels c with neg[c] != 0 (device int32 [C] or NULL) are negated in every obs frame of X and
 * in Y; statics are mirrored, not negated.  noise (float32 [B, obs * C, H, W] or NULL): X += noise * sigma, product
 * and sum rounded in float32.  A sample whose frames do not all lie in [0, T) is left untouched. */
int gcl_downscale_batch(const uint16_t* coarse, const uint16_t* fine, int64_t T, int32_t W, int32_t H, int32_t C,
                        const int64_t* t, int32_t B, int32_t obs, const float* mean, const float* stdv, const float* stat,
                        int32_t Ns, const int32_t* flip, const int32_t* neg, const float* noise, float sigma, float* X,
                        float* Y, gcl_stream_t stream);
/* The coarse baseline of compute_metrics (train_downscaler.py:288-305) over the n frames t[i] (device int64; a frame
 * outside [0, T) is skipped): stats float64 [C, 2] = {number of elements, sum of d^2}, d = xa - xb in float32 on the
 * normalised values as gcl_downscale_batch forms them, d^2 and the sum in float64.  Two stages in a fixed order: the
 * bits depend only on the data and the shapes.  ws: at least gcl_downscale_ws_bytes(C) bytes of device scratch. */
size_t gcl_downscale_ws_bytes(int32_t C);
int gcl_downscale_pair_mse(const uint16_t* xa, const uint16_t* xb, int64_t T, int64_t P, int32_t C, const int64_t* t,
                           int32_t n, const float* mean, const float* stdv, double* stats, void* ws, size_t ws_bytes,
                           gcl_stream_t stream);

/* ---- The downscaler's objective and scores (csrc/downscale_loss.hip; the losses, train_epoch and compute_metrics of
 * scripts/train_downscaler.py) ----
 * No entry point allocates or synchronises; offsets are int64; no floating-point atomics; every reduction has a fixed
 * order (bit-equal from run to run).  out, Y, dOut: contiguous float32 [B, C, H, W].  x_last: the channel slice
 * X[:, (obs - 1) * C : obs * C] of the input as a pointer to its first element and the batch stride xbs of X in
 * elements (channel stride H * W, rows contiguous), or NULL: o = out, or o = x_last + out rounded once in float32
 * (train_downscaler.py:236-240).  mask: float32 [C] or NULL (all ones).  rec: float64 [3] on the device = {mse, grad,
 * spec}; an entry point writes only the terms it computes.  ws: at least gcl_downscale_loss_ws_bytes(B, C, H, W) bytes
 * of 16-byte aligned device scratch.  2 <= H, W <= 256 and C <= 64, else GCL_EINVAL. */
size_t gcl_downscale_loss_ws_bytes(int32_t B, int32_t C, int32_t H, int32_t W);
/* masked_mse_loss (train_downscaler.py:189-193) and gradient_loss (:207-220) in one pass: with e = o - Y in float32 and
 * float64 sums, rec[0] = sum m_c e^2 / (B C H W) (masked channels stay in the denominator) and rec[1] =
 * sum m_c (e[h+1,w] - e[h,w])^2 / (B C (H-1) W) + sum m_c (e[h,w+1] - e[h,w])^2 / (B C H (W-1)).  A term whose weight
 * is not > 0 is skipped and its record untouched (:243-246); at least one must run.  dOut (or NULL) takes
 * d(mse_weight * mse + gradient_weight * grad) / d out, every element written exactly once: a tile of rows is staged
 * with one halo row either side. */
int gcl_downscale_loss_fwd_bwd(const float* out, const float* x_last, int64_t xbs, const float* Y, const float* mask,
                               int32_t B, int32_t C, int32_t H, int32_t W, float mse_weight, float gradient_weight,
                               double* rec, float* dOut, void* ws, size_t ws_bytes, gcl_stream_t stream);
/* spectral_loss (train_downscaler.py:196-204): rec[2] = sum | |P| - |T| | / (B C H (W/2+1)), P = rfft2(m_c o,
 * norm="ortho") and T the same of Y, every half-spectrum bin once; a separable direct DFT in float64, rows then
 * columns.  tw_h / tw_w: float64 [H, 2] / [W, 2] = (cos, sin)(2 pi k / n), built in double by the caller.  dOut (or
 * NULL) takes spectral_weight times the gradient, the adjoint of the real transform applied to sign(|P| - |T|) P / |P|
 * / count (0 where |P| = 0 or |P| = |T|): added to what dOut holds when accumulate != 0, stored otherwise. */
int gcl_downscale_spectral_fwd_bwd(const float* out, const float* x_last, int64_t xbs, const float* Y, const float* mask,
                                   const double* tw_h, const double* tw_w, int32_t B, int32_t C, int32_t H, int32_t W,
                                   float spectral_weight, int32_t accumulate, double* rec, float* dOut, void* ws,
                                   size_t ws_bytes, gcl_stream_t stream);
/* One batch of compute_metrics (train_downscaler.py:280-298): state float64 [C, 2] += the means over (B, H, W) of
 * (o - Y)^2 and of (x_last - Y)^2 (differences in float32, squares and sums in float64), o with x_last added when
 * residual != 0; count (device int64) += 1.  Per-batch means are averaged, as the reference does: a short last batch
 * weighs as much as a full one.  Everything stays on the device, so a captured graph can replay it. */
int gcl_downscale_metrics(const float* out, const float* x_last, int64_t xbs, const float* Y, int32_t residual, int32_t B,
                          int32_t C, int32_t H, int32_t W, double* state, int64_t* count, void* ws, size_t ws_bytes,
                          gcl_stream_t stream);
/* loss.backward() of train_downscaler.py:248 through the saved dOut: out[i] = dOut[i] * g[0], g the incoming gradient
 * on the device (no host sync).  In place is fine. */
int gcl_downscale_loss_scale(const float* dOut, const float* g, int64_t n, float* out, gcl_stream_t stream);

/* ---- Fused validation step (csrc/eval_step.hip; test() of src/train.py:241-309 for one batch) ----
 * No entry point allocates, synchronises or reads back; no atomics; every reduction has a fixed order, so results are
 * bit-equal from run to run.  The one-step prediction is formed as gcl_ar_advance forms step_out (src/train.py:273-292):
 * o = residual ? x_last + delta : delta in float32, static channels (chan_kind 1) take x_last, forcing channels
 * (chan_kind 2) take y; chan_kind NULL: all predicted.  delta / x_last / y / out are addressed with (ld, bs): x_last is
 * the last slot of the [B,G,obs*C] window (ldx = obs*C), y step 0 of [B,G,P*C] (ldy = P*C). */
size_t gcl_eval_colstats_ws_bytes(int32_t B, int32_t G, int32_t C);
/* stats[b,c,0..6] (float64) = sums over the G nodes of (o-y)^2, node_w[g] (o-y)^2 (node_w NULL = 1; the weights of
 * src/train.py:85-100), o', o'^2, y', y'^2, o' y' with o' = o - o[b,0,c], y' = y - y[b,0,c] (the sums behind
 * src/train.py:123-125; the shift removes the cancellation of one-pass variances).  o is stored to out [B,G,C] when
 * out is given, with the bits of gcl_ar_advance's step_out.  G >= 2 (torch's unbiased std is NaN below), B, C <= 65535;
 * ws: at least gcl_eval_colstats_ws_bytes(B, G, C) bytes of 8-byte aligned device scratch. */
int gcl_eval_colstats(const float* delta, int64_t ldd, int64_t bsd, const float* x_last, int64_t ldx, int64_t bsx,
                      const float* y, int64_t ldy, int64_t bsy, const float* node_w, const int32_t* chan_kind,
                      int32_t residual, float* out, int64_t ldo, int64_t bso, double* stats, int32_t B, int32_t G,
                      int32_t C, void* ws, size_t ws_bytes, gcl_stream_t stream);
/* Folds stats [B,C,7] into state (float64 [4] on the device) += {loss, acc, raw_mse, 1} of the batch
 * (src/train.py:295-303): loss = inv_wsum sum_b sum_c chan_w[c] stats[b,c,1] (chan_w NULL = 1), raw_mse =
 * sum stats[b,c,0] / (B G C), acc = the mean over b of the mean over the kept channels of cov / ((std_o + 1e-8)
 * (std_y + 1e-8)), cov = (S_o'y' - S_o' S_y' / G) / G, std = sqrt(max(S_x'x' - S_x'^2 / G, 0) / (G - 1)); kept channels
 * are those of chan_kind 0, or all of them when that leaves none (src/train.py:126-130). */
int gcl_eval_accumulate(const double* stats, const float* chan_w, const int32_t* chan_kind, double inv_wsum, int32_t B,
                        int32_t G, int32_t C, double* state, gcl_stream_t stream);

/* Batches from the stored legacy tensors (csrc/dataset.hip; src/data/dataloader.py:116-139, WeatherDataset.__getitem__
 * :22-23 under a DataLoader): X [N,G,Wx,F] and Y [N,G,Wy,F] contiguous float32 as the files hold them, idx device int64
 * [B].  outX[b,g,w*Fu+f] = X[idx[b], g, Wx-Wxu+w, f] for w < Wxu, f < Fu, and outY the same from Y with (Wy, Wyu); Y and
 * outY may both be NULL.  outX / outY are addressed with (ld, bs).  Copies are bit-exact; an idx[b] outside [0, N) gives
 * NaN rows for that sample.  One launch. */
int gcl_tensor_batch_pack(const float* X, int32_t Wx, int32_t Wxu, const float* Y, int32_t Wy, int32_t Wyu, int64_t N,
                          int32_t G, int32_t F, int32_t Fu, const int64_t* idx, int32_t B, float* outX, int64_t ldx,
                          int64_t bsx, float* outY, int64_t ldy, int64_t bsy, gcl_stream_t stream);

/* ---- Training and scoring the regional heads (csrc/region_train.hip; scripts/train_dual_mesh.py) ----
 * No entry point allocates, synchronises or reads back; no atomics; every reduction has a fixed order, so results are
 * bit-equal from run to run.
 *
 * The cache of the frozen global model's outputs (`--precompute`, scripts/train_dual_mesh.py:548-580) on the device.  One
 * record per sample, float32, four parts whose rows are zero-padded to a multiple of 4 floats (so every part is 16-byte
 * aligned in a 16-byte aligned cache), with XF = obs * C:
 *   roi3 [n_roi, roundup(XF + D, 4)] = [X[rows[i]] | latent[rows[i]] | 0]    (the roi_input of src/dual_mesh.py:683-686)
 *   send [half_E, roundup(Dm, 4)]    = [mesh[snd[k]] | 0]                    (the cross senders' rows, :774-777)
 *   pred [n_roi, roundup(C, 4)]      = [pred[rows[i]] | 0]
 *   y    [n_roi, roundup(P * C, 4)]  = [y[rows[i]] | 0]
 * gcl_region_cache_record_bytes: the size of one record (a multiple of 16), 0 for a shape that is not supported. */
size_t gcl_region_cache_record_bytes(int32_t n_roi, int32_t half_E, int32_t XF, int32_t D, int32_t Dm, int32_t C,
                                     int32_t P);
/* precompute_global (src/dual_mesh.py:731-752) for a batch of B samples in one launch: record slots[b] (device int64,
 * distinct within a call) of `cache` (n_slots records) is written from the dense global prediction pred [B,G,C], the
 * grid latents lat [B,G,D], the processed mesh latents mesh [B,M,Dm], the input window X [B,G,XF] and the target y
 * [B,G,P*C], each addressed with (ld, bs) as in gcl_roi_gather_rows.  rows: int32 [n_roi] grid rows; snd: int32 [half_E]
 * mesh rows in the order the regional module takes them.  A row index outside its source gives a zero row; a slot
 * outside [0, n_slots) is skipped.  Copies are bit-exact and pad columns are zero. */
int gcl_region_cache_store(const float* pred, int64_t ldp, int64_t bsp, const float* lat, int64_t ldl, int64_t bsl,
                           const float* mesh, int64_t ldm, int64_t bsm, const float* X, int64_t ldx, int64_t bsx,
                           const float* y, int64_t ldy, int64_t bsy, const int32_t* rows, const int32_t* snd,
                           const int64_t* slots, float* cache, int64_t n_slots, int32_t B, int32_t G, int32_t M,
                           int32_t n_roi, int32_t half_E, int32_t XF, int32_t D, int32_t Dm, int32_t C, int32_t P,
                           gcl_stream_t stream);
/* `cache[batch_idx]` and its `.to(device)` calls (scripts/train_dual_mesh.py:180-185) in one launch: the four parts of
 * the records slots[0..B) (device int64; a slot may repeat) go to roi3 / send / pred / y, each a [B, rows, padded width]
 * buffer with a sample stride bs (floats, a multiple of 4) and 16-byte alignment; a NULL destination is left out.  A
 * slot outside [0, n_slots) reads nothing and gives zero rows. */
int gcl_region_cache_fetch(const float* cache, int64_t n_slots, const int64_t* slots, int32_t B, int32_t n_roi,
                           int32_t half_E, int32_t XF, int32_t D, int32_t Dm, int32_t C, int32_t P, float* roi3,
                           int64_t bs_roi, float* send, int64_t bs_send, float* pred, int64_t bs_pred, float* y,
                           int64_t bs_y, gcl_stream_t stream);
/* One autoregressive step of eval_dual (scripts/train_dual_mesh.py:318-356; cached mode :289-308) for nq = 1 or 2
 * predictions - the corrected one and the global-only one - that advance in lock-step.  Per prediction q: delta_q
 * [B,G,C] and its input window win_q [B,G,obs*C], both with (ld, bs); step_out is formed as gcl_ar_advance forms it,
 * with the same bits (residual add of the window's last slot, static channels carried, forcing channels from y_step
 * [B,G,C]; chan_kind NULL: all predicted); new_win_q (contiguous [B,G,obs,C], or NULL: no window traffic) takes the
 * shifted window and out_q (with (ld, bs), or NULL; never delta_q or win_q themselves: the loss pass forms step_out
 * from them again) the step_out.  acc[q] (device float64) += weight * mean over
 * B * n * C of (step_out - y_step)^2 on the rows rows[0..n) (int32; NULL: rows 0..n), which is
 * weighted_mse_loss(out_roi, y_roi, None); weight = 1 / steps adds the mean over the AR steps.  A row index outside
 * [0, G) adds nothing.  Two-stage sum in float64: fixed chunks of 2048 elements, then the chunks in ascending order.
 * ws: at least gcl_region_eval_pair_ws_bytes(nq, B, n, C) bytes of 8-byte aligned device scratch. */
size_t gcl_region_eval_pair_ws_bytes(int32_t nq, int32_t B, int32_t n, int32_t C);
int gcl_region_eval_pair(int32_t nq, const float* delta0, int64_t ldd0, int64_t bsd0, const float* win0, int64_t ldw0,
                         int64_t bsw0, float* new_win0, float* out0, int64_t ldo0, int64_t bso0, const float* delta1,
                         int64_t ldd1, int64_t bsd1, const float* win1, int64_t ldw1, int64_t bsw1, float* new_win1,
                         float* out1, int64_t ldo1, int64_t bso1, const float* y_step, int64_t ldy, int64_t bsy,
                         const int32_t* chan_kind, int32_t residual, const int32_t* rows, int32_t n, double weight,
                         double* acc, int32_t B, int32_t G, int32_t obs, int32_t C, void* ws, size_t ws_bytes,
                         gcl_stream_t stream);

/* ---- Station observations and regional scoring of a saved forecast (csrc/predict.hip) ----
 * No entry point allocates, synchronises or reads back; no atomics; every reduction has a fixed order, so results are
 * bit-equal from run to run.
 *
 * The sparse observation tensor of scripts/create_obs.py:79-144 (and the inline draw of scripts/predict.py:394-421,
 * :471-483) in one launch: obs[b,g,k] = keep_row[g] && keep_chan[k % C] ? y[b,g,k] : NaN for k < K, NaN the quiet NaN
 * that float('nan') gives (bits 0x7fc00000).  y / obs [B,G,K] are addressed with (ld, bs); keep_row uint8 [G], keep_chan
 * uint8 [C].  Rows move as 16-byte accesses when K, the strides and both bases allow it, element by element otherwise;
 * kept values are copied bit for bit and a row that is not kept is never read.  obs may be y itself. */
int gcl_obs_pack(const float* y, int64_t ldy, int64_t bsy, const uint8_t* keep_row, const uint8_t* keep_chan, int32_t B,
                 int32_t G, int32_t K, int32_t C, float* obs, int64_t ldo, int64_t bso, gcl_stream_t stream);
/* The interpolation loop and the sums behind every score of scripts/interpolate_to_region.py:168-249.  pred [N,Gg,>=P*C]
 * float32 with (ld, bs), longitude-major with nlat latitudes; cell int32 [nr,2] / w float64 [nr,4]: the tables of the
 * regional nodes (longitude-major) as gcl_regrid_blend takes them; series fp16 [n_time,nr,n_feat], n_feat >= C; t0 device
 * int32 [N]: the regional step of horizon 0 of every sample, a sample with t0 < 1 or t0 + P > n_time (-1 by convention)
 * is skipped; first: the index of the first sample that is not skipped; mean / std float64 [C].  Per sample s, horizon p,
 * node i, channel c:
 *   v = the bilinear value of pred[s, :, p*C + c] in float64, four products rounded one by one and added in the order of
 *       gcl_regrid_blend (scipy's);  t = ((double)series[t0 + p, i, c] - mean[c]) / std[c];  b the same at t0 - 1.
 * sums float64 [P,C,11] = sum (v-t)^2, sum |v-t|, sum (b-t)^2, the count, sum t', sum t'^2, sum v', sum v'^2, sum t'v'
 * with t' = t - tp, v' = v - vp, and the pivots tp, vp: t and v at node 0 of sample `first` for that (p, c) (0 when
 * that sample is skipped).  vout / tout (both or neither; float32 [N,P,nr,C]) take (float)v and (float)t of the samples
 * that are not skipped; the other samples' rows are left as they are.  A cell outside the Gg source rows gives NaN.
 * C <= 256; N, P <= 65535.  Two stages: fixed node chunks per (sample, horizon), then the partials of a (p, c) in a fixed
 * tree.  ws: at least gcl_region_interp_scores_ws_bytes(N, P, nr, C) bytes of 8-byte aligned device scratch. */
size_t gcl_region_interp_scores_ws_bytes(int32_t N, int32_t P, int32_t nr, int32_t C);
int gcl_region_interp_scores(const float* pred, int64_t ldp, int64_t bsp, int32_t Gg, int32_t nlat, const int32_t* cell,
                             const double* w, const void* series, int32_t n_feat, int32_t n_time, const int32_t* t0,
                             int32_t first, const double* mean, const double* std, int32_t N, int32_t P, int32_t nr,
                             int32_t C, double* sums, float* vout, float* tout, void* ws, size_t ws_bytes,
                             gcl_stream_t stream);

/* ---- WeatherUNet inference and the cascade scores (csrc/unet.hip) ----
 * The eval-mode forward of src/unet/model.py:11-98 as one launch per convolution, and the per-step refinement and scores
 * of scripts/predict_cascade.py:338-372.  No entry point allocates, synchronises or reads back; no floating-point
 * atomics; every sum has an order fixed by the layer's shape, never by B or a sample's place in the batch.
 *
 * Activations between layers are channels-last [B,H,W,C] float32.  MaxPool2d(2), Upsample(bilinear, align_corners),
 * the pad to the skip's size and the concatenation (model.py:32-56) are not launches or tensors: they are ways the next
 * convolution reads its input, described by gcl_unet_src_t:
 *   PLANAR  a = the caller's [B,Cin,H,W] tensor (the first layer).
 *   ROWS    a = [B,H,W,Cin].
 *   POOL    a = [B,Hs,Ws,Cin]; the input is its 2x2 maximum, H = Hs / 2, W = Ws / 2 (a last odd row / column is dropped,
 *           a NaN in a window gives NaN: torch's max_pool2d).
 *   UPCAT   channels 0 .. C1-1 are a = the skip [B,H,W,C1]; channels C1 .. C1+C2-1 are the bilinear interpolation of
 *           b = [B,Hs,Ws,C2] to 2 Hs x 2 Ws (align_corners=True: s = dst * (in-1)/(out-1) in float32, i0 = floor(s),
 *           i1 = min(i0+1, in-1), l = s - i0), zero at rows >= 2 Hs or columns >= 2 Ws.  C1 + C2 = Cin. */
#define GCL_UNET_SRC_PLANAR 0
#define GCL_UNET_SRC_ROWS 1
#define GCL_UNET_SRC_POOL 2
#define GCL_UNET_SRC_UPCAT 3
typedef struct gcl_unet_src {
  const float* a;
  const float* b;
  int32_t kind;
  int32_t C1, C2; /* UPCAT */
  int32_t Hs, Ws; /* POOL: the source's size; UPCAT: the low tensor's */
} gcl_unet_src_t;
/* torch's Conv2d weight [Cout,Cin,3,3] (model.py:16,19) into the order gcl_unet_conv3x3 streams: per 32 output channels,
 * tap and 8 input channels one 1 KiB record holding each lane's four B operands of v_mfma_f32_32x32x2_f32, zero where
 * Cin or Cout is padded.  packed: gcl_unet_packed_floats(Cin, Cout) floats, 16-byte aligned.  One launch. */
int64_t gcl_unet_packed_floats(int32_t Cin, int32_t Cout);
int gcl_unet_pack_weights(const float* w, int32_t Cin, int32_t Cout, float* packed, gcl_stream_t stream);
/* One 3x3 convolution (padding 1, no bias) with BatchNorm2d in eval mode and the exact (erf) GELU behind it
 * (model.py:15-22), one launch: y[b,y,x,co] = gelu((acc - mean[co]) * (gamma[co] / sqrt(var[co] + eps)) + beta[co]) from
 * the four vectors as they are at the call (no folded copy); gamma == NULL (then all four are ignored): y = acc.
 * An implicit GEMM on the fp32-operand matrix instruction: a block owns 4 x 8 output pixels of one sample and 32 output
 * channels; the input tile with its one-pixel halo is staged in LDS 32 channels at a time and all nine taps are read
 * from there; the block's four waves take 8 channels of a chunk each and their partial sums are added in LDS as
 * (w0 + w1) + (w2 + w3) (from Cin = 256 on: eight waves, chunks of 64 channels, + ((w4 + w5) + (w6 + w7))).  Cin >= 1, Cout % 4 == 0, H, W >= 1, B <= 65535; y [B,H,W,Cout] and packed 16-byte aligned.
 * A NaN or Inf reaches only the outputs of its own sample. */
int gcl_unet_conv3x3(const gcl_unet_src_t* src, const float* packed, const float* gamma, const float* beta,
                     const float* mean, const float* var, float eps, float* y, int32_t B, int32_t H, int32_t W,
                     int32_t Cin, int32_t Cout, gcl_stream_t stream);
/* The 1x1 output convolution (model.py:85,98): x [B,H,W,F] times w [Cout,F] plus bias [Cout], written as the planar
 * y [B,Cout,H,W]; the products are added in ascending f.  residual (may be NULL): a planar tensor whose sample stride is
 * res_bs floats and whose channel co is added, y = (conv + bias) + residual, each sum rounded in float32: the x_last of
 * predict_cascade.py:357-359 read from the network's own input.  F % 4 == 0, x and w 16-byte aligned, Cout any. */
int gcl_unet_conv1x1_out(const float* x, const float* w, const float* bias, const float* residual, int64_t res_bs,
                         float* y, int32_t B, int32_t H, int32_t W, int32_t F, int32_t Cout, gcl_stream_t stream);
/* How many kernels the entry points of this section have launched in this process (a counter for tests). */
int64_t gcl_unet_launches(void);
/* predict_cascade.py:346-354 for B samples in one launch.  coarse [B,H,W,C] in GNN-normalised space;
 * coarse_phys [B,H,W,C] = coarse * gnn_std + gnn_mean, product and sum rounded one by one; X [B,obs*C+Ns,H,W]: channel
 * o*C + c = (coarse_phys - ds_mean[c]) / ds_std[c] (each operation rounded, no epsilon) for o < obs, channel obs*C + s =
 * static_fine[x,y,s] (static_fine [W,H,Ns], NULL when Ns == 0).  The four vectors are float32 [C]. */
int gcl_cascade_pack(const float* coarse, const float* gnn_mean, const float* gnn_std, const float* ds_mean,
                     const float* ds_std, const float* static_fine, float* coarse_phys, float* X, int32_t B, int32_t H,
                     int32_t W, int32_t C, int32_t obs, int32_t Ns, gcl_stream_t stream);
/* predict_cascade.py:360-372.  out [B,C,H,W]: the network's planar output (residual applied); coarse_phys [B,H,W,C];
 * fine: fp16 [T,W,H,n_feat], n_feat >= C; t_fine / t_persist: device int64 [B].  cascade_phys = out * ds_std + ds_mean
 * (float32, rounded one by one).  Per (sample, channel): the mean over H*W of (coarse_phys - f)^2, (cascade_phys - f)^2
 * and (p - f)^2, f = (float)fine[t_fine], p = (float)fine[t_persist]; differences and squares in float32, the sum over
 * the pixels in float64 (fixed chunks of pixels, then the chunks in a fixed order), divided by H*W.  state float64
 * [AR,C,3] (gnn, cascade, persistence): state[step] += the samples' means one after the other in batch order, so that
 * the batch size does not reach the bits; count int64 [AR]: count[step] += the samples scored.  A sample whose t_fine or
 * t_persist is outside [0, T) is skipped.  ws: gcl_cascade_scores_ws_bytes(B, H, W, C) bytes, 8-byte aligned.
 * Two launches. */
size_t gcl_cascade_scores_ws_bytes(int32_t B, int32_t H, int32_t W, int32_t C);
int gcl_cascade_scores(const float* out, const float* coarse_phys, const void* fine, int32_t T, int32_t n_feat,
                       const int64_t* t_fine, const int64_t* t_persist, const float* ds_mean, const float* ds_std,
                       double* state, int64_t* count, int32_t step, int32_t AR, int32_t B, int32_t H, int32_t W,
                       int32_t C, void* ws, size_t ws_bytes, gcl_stream_t stream);

/* ---- WeatherUNet training (csrc/unet_train.hip) ----
 * model.py:11-98 in .train(): BatchNorm2d on batch statistics, and the backward pass of every layer.  Activations stay
 * channels-last [B,H,W,C] float32 (n = B*H*W rows of C values).  No entry point allocates, synchronises or reads back.
 * No atomics.  Every per-channel sum runs in float64 in two stages: fixed chunks of rows (the chunking of the scorers,
 * a function of n alone), then a column's chunks in a fixed order; so two calls give equal bits.  The counter below is
 * this section's own: gcl_unet_launches does not see these launches. */
int64_t gcl_unet_train_launches(void);
/* Workspace of a two-stage column sum over n rows and ncols columns (float64 partials), 8-byte aligned:
 * gcl_unet_bn_stats and gcl_unet_bn_gelu_bwd take ncols = 2 C. */
size_t gcl_unet_colsum_ws_bytes(int64_t n, int64_t ncols);
/* The batch statistics of z [n,C] (model.py:17,20 in training): mean[c], and invstd[c] = 1 / sqrt(var + eps) with the
 * biased variance, from sum z and sum z^2 in float64, stored as float32 [C].  running_mean / running_var (may be NULL)
 * are updated in place as nn.BatchNorm2d does, r = (1 - momentum) r + momentum * (mean | var * n / (n - 1)), and
 * *num_batches (device int64, may be NULL) is incremented.  n >= 2 (torch refuses one value per channel too).
 * Two launches. */
int gcl_unet_bn_stats(const float* z, int64_t n, int32_t C, float eps, float momentum, float* mean, float* invstd,
                      float* running_mean, float* running_var, int64_t* num_batches, void* ws, size_t ws_bytes,
                      gcl_stream_t stream);
/* a = gelu_erf(gamma * (z - mean) * invstd + beta).  C % 4 == 0, every tensor 16-byte aligned.  One launch. */
int gcl_unet_bn_gelu(const float* z, const float* gamma, const float* beta, const float* mean, const float* invstd, float* a,
                     int64_t n, int32_t C, gcl_stream_t stream);
/* The backward of the two above.  xhat = (z - mean) * invstd, u = gamma * xhat + beta, g = dA * gelu'(u);
 * dbeta[c] = S1 = sum g, dgamma[c] = S2 = sum g * xhat (float64, two stages: the reduce), then
 * dZ = gamma * invstd * (g - S1 / n - xhat * S2 / n) (the apply).  dZ may be dA.  Three launches. */
int gcl_unet_bn_gelu_bwd(const float* z, const float* dA, const float* gamma, const float* beta, const float* mean,
                         const float* invstd, float* dZ, float* dgamma, float* dbeta, int64_t n, int32_t C, void* ws,
                         size_t ws_bytes, gcl_stream_t stream);
/* The weight gradient of gcl_unet_conv3x3: dW[co][ci][ty][tx] = sum over b, y, x of dZ[b,y,x,co] * in(b, y+ty-1, x+tx-1, ci),
 * `in` read through the same source descriptor as the forward (zero outside the image), dW in torch's [Cout,Cin,3,3]
 * layout.  An implicit GEMM on the fp32-operand matrix instruction with M = 32 output channels, N = 32 input channels and
 * K = pixels: a one-wave block owns a (32 co, 32 ci) tile for all nine taps and a chunk of consecutive 4 x 8 pixel tiles
 * (numbered over the whole batch); the chunks' partial tiles go to ws and a second launch adds them per element in
 * ascending chunk order in float64.  The chunk count - gcl_unet_wgrad_chunks, at most 256 - is a function of
 * (B, H, W, Cin, Cout) alone.  Cout % 4 == 0; dZ and ws 16-byte aligned; ws: gcl_unet_wgrad_ws_bytes bytes, every byte of
 * which that is read is written first.  Two launches. */
int32_t gcl_unet_wgrad_chunks(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout);
size_t gcl_unet_wgrad_ws_bytes(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout);
int gcl_unet_conv3x3_wgrad(const gcl_unet_src_t* src, const float* dZ, float* dW, int32_t B, int32_t H, int32_t W,
                           int32_t Cin, int32_t Cout, void* ws, size_t ws_bytes, gcl_stream_t stream);
/* w [Cout,Cin,3,3] transposed and tap-flipped, w'[ci][co][t] = w[co][ci][8 - t], in the record order gcl_unet_conv3x3
 * streams: the data gradient of a convolution is gcl_unet_conv3x3(ROWS(dZ), packed', gamma = NULL) with Cin' = Cout and
 * Cout' = Cin (a multiple of 4).  packed: gcl_unet_packed_floats(Cout, Cin) floats.  One launch. */
int gcl_unet_pack_weights_dgrad(const float* w, int32_t Cin, int32_t Cout, float* packed, gcl_stream_t stream);
/* The data gradient of a POOL source back at the source's size: dA[b,y,x,c] = skip[b,y,x,c] + (pixel is its 2x2 window's
 * argmax ? dpooled[b,y/2,x/2,c] : 0).  act [B,Hs,Ws,C] is the saved activation; the argmax is recomputed by torch's scan
 * (row-major; a value replaces the running maximum if v > m or v != v).  skip (may be NULL): rows of skip_ld floats whose
 * first C are added - the first C1 channels of an UPCAT data gradient, read in place.  A dropped odd last row or column
 * receives the skip part only.  Every element of dA is written exactly once.  C % 4 == 0.  One launch. */
int gcl_unet_pool_bwd(const float* act, const float* dpooled, const float* skip, int64_t skip_ld, float* dA, int32_t B,
                      int32_t Hs, int32_t Ws, int32_t C, gcl_stream_t stream);
/* The adjoint of the UPCAT source's bilinear read (align_corners=True) and zero pad, in gather form:
 * dlow [B,Hs,Ws,C2] from channels c_off .. c_off+C2-1 of d [B,H,W,ld]; a low element adds the contributions of the
 * pixels below (2 Hs, 2 Ws) that read it in ascending (y, x) order, the weights formed by the read's float32 rule.
 * C2 % 4 == 0, c_off % 4 == 0, ld % 4 == 0.  One launch. */
int gcl_unet_upsample_bwd(const float* d, int64_t ld, int32_t c_off, float* dlow, int32_t B, int32_t H, int32_t W, int32_t Hs,
                          int32_t Ws, int32_t C2, gcl_stream_t stream);
/* The backward of gcl_unet_conv1x1_out from the planar dY [B,Cout,H,W]: dA [B,H,W,F] = sum over c (ascending) of
 * dY[c] * w[c,f]; dW [Cout,F] = sum over pixels of dY[c] * a[f] and db [Cout] = sum dY[c], as two-stage float64 column
 * sums.  F % 4 == 0.  Three launches. */
size_t gcl_unet_conv1x1_out_bwd_ws_bytes(int32_t B, int32_t H, int32_t W, int32_t F, int32_t Cout);
int gcl_unet_conv1x1_out_bwd(const float* dY, const float* a, const float* w, float* dA, float* dW, float* db, int32_t B,
                             int32_t H, int32_t W, int32_t F, int32_t Cout, void* ws, size_t ws_bytes, gcl_stream_t stream);

/* ---- WeatherUNetV2 inference (csrc/unet_v2.hip) ----
 * What src/unet/model_v2.py has around its 3x3 convolutions (those are gcl_unet_conv3x3 with gamma == NULL): GroupNorm,
 * the residual 1x1 skip, the squeeze-and-excitation gate, self-attention over the bottleneck pixels and the Fourier-mode
 * convolution.  Activations are channels-last [B,H,W,C] float32 (HW = H * W pixels, a token of the attention is a
 * pixel).  No entry point allocates, synchronises or reads back; no atomics; every sum has an order fixed by the layer's
 * shape, never by B or a sample's place in the batch, so a sample's bits repeat; a NaN or Inf stays in its sample.  This
 * section's launch counter is its own: gcl_unet_launches does not see these launches. */
int64_t gcl_unet_v2_launches(void);
/* GroupNorm statistics of z [B,HW,C], G groups of C / G adjacent channels: mean [B,G] and invstd [B,G] =
 * 1 / sqrt(biased variance + eps).  One block per (sample, group): the mean first, then the second moment about it, both
 * summed in float64 (thread-strided partial sums, then a fixed tree), so |mean| >> spread costs nothing.  HW * C < 2^31.
 * One launch. */
int gcl_unet_v2_gn_stats(const float* z, int32_t B, int32_t HW, int32_t C, int32_t G, float eps, float* mean, float* invstd,
                         gcl_stream_t stream);
/* out = gelu(((z - mean[b,g]) * invstd[b,g]) * gamma[c] + beta[c]), the erf GELU; out is not z.  C % 4 == 0; z and
 * out 16-byte aligned.  One launch. */
int gcl_unet_v2_gn_gelu(const float* z, const float* gamma, const float* beta, const float* mean, const float* invstd,
                        float* out, int32_t B, int32_t HW, int32_t C, int32_t G, gcl_stream_t stream);
/* The 1x1 convolution of a source of any kind (the input is read as gcl_unet_conv3x3 reads it, never materialised):
 * out[b,y,x,co] = sum over ci (ascending, one fmaf chain) of w[co,ci] * in(b,y,x,ci), then + bias[co] when bias is given,
 * then res[b,y,x,co] + that when res (contiguous [B,H,W,Cout]) is given.  Pixels of out are ldo floats apart (ldo >= Cout:
 * a channel slice of wider rows), so out is the pointer to the slice's first channel.  w == NULL: the identity (Cin ==
 * Cout, no bias, no res): out = the source.  Cout % 4 == 0, ldo % 4 == 0, out 16-byte aligned.  With a ROWS source of
 * H x W = N x 1 tokens this is nn.Linear.  One launch. */
int gcl_unet_v2_conv1x1(const gcl_unet_src_t* src, const float* w, const float* bias, const float* res, float* out,
                        int64_t ldo, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, gcl_stream_t stream);
/* The tail of a ResConvBlock (model_v2.py:35-37,60): u = gelu(GroupNorm(z)) + skip; m[b,c] = mean over the pixels of u;
 * gate = sigmoid(w2 gelu(w1 m + b1) + b2), w1 [hidden,C], w2 [C,hidden]; out = u * gate.  Two launches: the first writes
 * u and, per chunk of pixels (gcl_unet_v2_tail_chunks(HW) chunks, at most 256, a function of HW alone), the float64
 * channel sums; every block of the second adds the chunks in ascending order, forms the gate itself and scales its own
 * chunk of out in place.  C % 4 == 0, C <= 2048, hidden <= 512, HW * C < 2^31; z, skip, out 16-byte aligned; out may be z
 * or skip.  ws: gcl_unet_v2_tail_ws_bytes(B, HW, C) bytes, 8-byte aligned. */
int32_t gcl_unet_v2_tail_chunks(int32_t HW);
size_t gcl_unet_v2_tail_ws_bytes(int32_t B, int32_t HW, int32_t C);
int gcl_unet_v2_block_tail(const float* z, const float* gamma, const float* beta, const float* mean, const float* invstd,
                           const float* skip, const float* w1, const float* b1, const float* w2, const float* b2,
                           float* out, int32_t B, int32_t HW, int32_t C, int32_t G, int32_t hidden, void* ws,
                           size_t ws_bytes, gcl_stream_t stream);
/* nn.LayerNorm over the last dimension of x [rows,C] (biased variance about the mean), a wave per row.  One launch. */
int gcl_unet_v2_layernorm(const float* x, const float* gamma, const float* beta, float eps, float* out, int64_t rows,
                          int32_t C, gcl_stream_t stream);
/* model_v2.py:81-87: qkv [B,N,3,heads,head_dim] -> out [B,N,heads*head_dim] = softmax(q k^T head_dim^-1/2) v per (sample,
 * head).  A wave per query: the row maximum first, then exp(score - max) key by key, the value sum in ascending key
 * order, divided by the sum of the exponentials at the end.  Any N <= 4096 (written for N <= 64).  One launch. */
int gcl_unet_v2_attention(const float* qkv, float* out, int32_t B, int32_t N, int32_t heads, int32_t head_dim,
                          gcl_stream_t stream);
/* SpectralConv2d (model_v2.py:95-122) on x [B,Hb,Wb,C] by direct sums over the kept modes kh < mh <= Hb, kw < mw <=
 * Wb / 2 + 1 (mode = kh * mw + kw), with theta = 2 pi (kh h / Hb + kw w / Wb) formed from (kh h mod Hb, kw w mod Wb):
 *   pack  w_re, w_im [Cin,Cout,modes_h,modes_w] -> packed [mode][Cin][Cout] complex (re, im interleaved);
 *   fwd   X[b,mode,i] = (Hb Wb)^-1/2 sum over the pixels (ascending) of x[b,h,w,i] exp(-i theta), complex [B,modes,C];
 *   mix   O[b,mode,o] = sum over i of X[b,mode,i] * packed[mode,i,o]: eight waves take an eighth of Cin each in ascending
 *         i, their sums are added as a fixed tree; the weights are read once per four samples;
 *   inv   y[b,h,w,o] = (Hb Wb)^-1/2 sum over the modes (ascending) of c_kw Re(O[b,mode,o] exp(+i theta)), c_kw = 1 for
 *         kw = 0 and for kw = Wb / 2 when Wb is even, else 2; pixels of y are ldo floats apart.
 * Hb, Wb <= 32768, Hb * Wb <= 2^24, at most 1024 modes.  X, packed, O 8-byte aligned.  One launch each. */
int gcl_unet_v2_spectral_pack(const float* w_re, const float* w_im, int32_t Cin, int32_t Cout, int32_t modes_h,
                              int32_t modes_w, int32_t mh, int32_t mw, float* packed, gcl_stream_t stream);
int gcl_unet_v2_spectral_fwd(const float* x, float* X, int32_t B, int32_t Hb, int32_t Wb, int32_t C, int32_t mh, int32_t mw,
                             gcl_stream_t stream);
int gcl_unet_v2_spectral_mix(const float* X, const float* packed, float* O, int32_t B, int32_t nmodes, int32_t Cin,
                             int32_t Cout, gcl_stream_t stream);
int gcl_unet_v2_spectral_inv(const float* O, float* out, int64_t ldo, int32_t B, int32_t Hb, int32_t Wb, int32_t C,
                             int32_t mh, int32_t mw, gcl_stream_t stream);

/* ---- The regional U-Net forecaster's loop around its network (csrc/unet_forecast.hip) ----
 * src/unet/predict.py and predict_v2.py (the same script but for the model built): the window as a planar 2-D grid and one
 * autoregressive step's carry-forward, shift and scores, batched over B window starts t0[b] (device int64).  No entry
 * point allocates, synchronises or reads back; no atomics; every sum has an order fixed by (H, W, C) alone, never by B or
 * a sample's place in the batch; a NaN or Inf stays in its sample.  series: IEEE binary16 [T, n_lon, n_lat, Ct]; the
 * planar tensors are [.., H = n_lat, W = n_lon] float32, so every read of the series is a transpose, staged through LDS
 * in tiles of 32 columns x 8 rows: 16-byte reads of the series, and 16-byte accesses of the planes when W % 4 == 0 (one
 * float per lane otherwise).  mean, std: float32 [C], C <= Ct.  This section's launch counter is its own. */
int64_t gcl_unet_forecast_launches(void);
/* src/data/dataloader_chunked.py:202-218 followed by Grid2DDataset.__getitem__ (predict_v2.py:36-40), the input half:
 * X [B, obs*C, H, W], channel o*C + c at (h, w) = ((float)series[t0+o, w, h, c] - mean[c]) / std[c], bit-identical to
 * the numpy loader (the contract of gcl_window_pack, planar).  A sample whose window [t0, t0 + obs) is not inside [0, T)
 * is filled with NaN.  B, obs <= 65535.  One launch. */
int gcl_grid_window_pack(const uint16_t* series /* IEEE binary16 */, int64_t T, int32_t n_lon, int32_t n_lat, int32_t Ct,
                         const int64_t* t0, const float* mean, const float* stdv, int32_t C, int32_t obs,
                         float* X /*[B,obs*C,H,W]*/, int32_t B, gcl_stream_t stream);
/* predict_v2.py:138-180 for B samples at autoregressive step `step` (0 <= step < AR).  out [B,C,H,W]: the network's
 * planar output with x_last added (residual_from); X [B,obs*C,H,W]: the current window; chan_kind uint8 [C]: 0 dynamic,
 * 1 static, 2 forcing (a channel in both of the script's lists is forcing, its later assignment).
 *   carry    out' = out (dynamic), X[:, (obs-1)*C + c] (static, :142-144), or the normalised truth
 *            ((float)series[t0+obs+step, w, h, c] - mean[c]) / std[c] (forcing, :145-148); bit-exact in all three;
 *   shift    X_next [B,obs*C,H,W] = channels C .. obs*C of X, then out' (:180); X_next is not X.  pred [B,C,H,W] (may be
 *            NULL) receives out' alone;
 *   scores   per (sample, channel), with g = the normalised truth frame t0+obs+step and bl = the normalised frame
 *            t0+obs-1, both read from the series: sum (out'*std+mean - (g*std+mean))^2, the same for bl (:156-160),
 *            sum (out'-g)^2 and sum (bl-g)^2 (:162-163) - products, sums, differences and squares in float32 one by one
 *            as numpy forms them, the sums over the pixels in float64; the field means of out' and g in float64, then
 *            about them sum p^2, sum t^2 and sum p t in float64 (a second pass: |mean| >> spread costs nothing) and
 *            corr = sum p t / (sqrt(sum p^2) * sqrt(sum t^2)), counted when both norms exceed 1e-8 (:166-175);
 *   state    float64 [AR,C,5] (se_phys, se_base_phys, se_norm, se_base_norm, acc_sum), acc_count int64 [AR,C], count
 *            int64 [AR]: state[step] += the samples' values one after the other in batch order, so that the batch size
 *            does not reach the bits (the rule of gcl_cascade_scores); count[step] += H*W per sample scored.
 * A sample whose t0 < 0 or whose truth frame is outside [0, T) is skipped: nothing is scored and its X_next / pred stay
 * unwritten (a fixed-B graph takes a tail batch with t0 = -1 rows).  B <= 65535, obs <= 4096; with W % 4 == 0
 * out, X, X_next and pred are 16-byte aligned.  ws: gcl_grid_forecast_step_ws_bytes(B, H, W, C) bytes, 8-byte aligned;
 * on return it holds, for the samples scored, float64 [B][C][6][n] (the four squared-error sums, sum out', sum g) followed
 * by [B][C][3][n] (sum p^2, sum t^2, sum p t about the means), n = the byte count / (72 B C) chunks of tiles to be added.
 * Three launches: carry + shift + the squared errors and field sums per chunk of tiles; the centred sums per chunk of
 * tiles; the chunks of a (sample, channel) in a fixed order into the state. */
size_t gcl_grid_forecast_step_ws_bytes(int32_t B, int32_t H, int32_t W, int32_t C);
int gcl_grid_forecast_step(const float* out, const float* X, const uint16_t* series /* IEEE binary16 */, int64_t T,
                           int32_t n_lon, int32_t n_lat, int32_t Ct, const int64_t* t0, const uint8_t* chan_kind,
                           const float* mean, const float* stdv, int32_t C, int32_t obs, int32_t step, int32_t AR,
                           float* X_next, float* pred, double* state, int64_t* acc_count, int64_t* count, int32_t B,
                           void* ws, size_t ws_bytes, gcl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GCL_H */
