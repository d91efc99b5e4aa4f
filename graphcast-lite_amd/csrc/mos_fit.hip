// Fitting the learned-MOS forest: histogram gradient boosting (scripts/build_learned_mos.py:357-369, the
// HistGradientBoostingRegressor.fit of the reference) with squared error, no missing values and a constant hessian.
//
// One tree is a FIXED sequence of launches: every decision (which leaf to split, whether a child is a leaf, which child
// gets its histogram built) is taken on the device and handed from kernel to kernel through a small `Job` record, so the
// host reads nothing back per split and the sequence can be replayed from a hipGraph.  A round that has nothing left to
// split turns into launches whose blocks return at once.
//
// Reproducibility: no floating-point atomic anywhere.  A histogram pass cuts the segment into at most kRanges row ranges;
// inside a range one wave owns one feature and one lane owns four bins, and adds the rows one after the other in
// partition order (registers, float64).  The range partials are stored and then summed in range order by one thread per
// bin ("store-and-sum").  Gains, leaf values and scores therefore repeat bit for bit from run to run.
#include "common.h"

namespace {

constexpr int kBins = 256;      // bins of one feature (255 thresholds at most)
constexpr int kMaxF = 32;       // MOSForest's feature limit
constexpr int kMaxLeaves = 256; // max_leaf_nodes supported
constexpr int kRanges = 256;    // row ranges of one histogram pass
constexpr int kMinRange = 256;  // rows of a range at least (short segments use fewer ranges)
constexpr int kChunk = 1024;    // rows of one partition / raw-update / score block (256 threads x 4)
constexpr int kNoBin = 1 << 20; // bin of a lane past the end of its range: owned by nobody

enum : int32_t { kUnset = 0, kSplittable = 1, kLeaf = 2, kSplit = 3 };

struct Job {  // what the segment kernels of one round work on
  int32_t active;             // 0: every kernel of the round returns at once
  int32_t start, count;       // partition: the segment of the partition array
  int32_t feat, bin;          // partition: rows with bins[feat][row] <= bin go left
  int32_t build;              // 1: build the histogram of [hstart, hstart + hcount)
  int32_t hstart, hcount;
  int32_t small, large, parent;  // histogram slots: built, parent - built (-1: none), parent
  int32_t split[2];           // slots to find the best split of (-1: none)
  int32_t split_n[2];
  double split_g[2];
};

struct Node {
  int32_t start, count, depth, state;
  int32_t feat, bin, n_left, left, right, missing_left;
  double sum_g, gain, sum_g_left, value;
};

struct Best {  // best split of one feature of one node
  double gain, sum_g_left;
  int32_t bin, n_left;
};

struct Tree {
  int32_t n_nodes, n_leaves, skip, n_final_leaves;
  int32_t pending[2];  // nodes whose per-feature bests wait in `best`
  int32_t pad[2];
};

struct Layout {
  size_t job, tree, nodes, best, leaf_start, leaf_count, leaf_value, part, tmp, grad, cnts, psum, pcnt, hsum, hcnt,
      spart, total;
  int slots;
};

size_t up256(size_t x) { return (x + 255) & ~size_t(255); }

Layout layout(int64_t n, int64_t n_val, int F, int max_leaf_nodes) {
  Layout L;
  size_t o = 0;
  auto take = [&](size_t bytes) {
    size_t at = o;
    o += up256(bytes);
    return at;
  };
  L.slots = 2 * max_leaf_nodes - 1;
  L.job = take(sizeof(Job));
  L.tree = take(sizeof(Tree));
  L.nodes = take(sizeof(Node) * L.slots);
  L.best = take(sizeof(Best) * 2 * kMaxF);
  L.leaf_start = take(4 * kMaxLeaves);
  L.leaf_count = take(4 * kMaxLeaves);
  L.leaf_value = take(8 * kMaxLeaves);
  L.part = take(4 * (size_t)n);
  L.tmp = take(4 * (size_t)n);
  L.grad = take(4 * (size_t)n);
  L.cnts = take(4 * (size_t)gcl::cdiv(n > 0 ? n : 1, kChunk));
  L.psum = take(8 * (size_t)kRanges * F * kBins);
  L.pcnt = take(4 * (size_t)kRanges * F * kBins);
  L.hsum = take(8 * (size_t)L.slots * F * kBins);
  L.hcnt = take(4 * (size_t)L.slots * F * kBins);
  L.spart = take(8 * (size_t)gcl::cdiv(n_val > 0 ? n_val : 1, kChunk));
  L.total = o;
  return L;
}

template <class T>
T* at(void* ws, size_t off) {
  return reinterpret_cast<T*>(static_cast<char*>(ws) + off);
}

// sklearn's compute_node_value without bounds: -g / (h + l2 + 1e-15)
__device__ __forceinline__ double node_value(double g, double h, double l2) { return -g / ((h + l2) + 1e-15); }

__device__ __forceinline__ int ranges_of(int count) {
  int nr = (count + kMinRange - 1) / kMinRange;
  return nr < 1 ? 1 : (nr > kRanges ? kRanges : nr);
}

// exclusive prefix of v over the 256 threads of the block (thread order), and the block total
__device__ __forceinline__ int block_excl_scan(int v, int& total) {
  __shared__ int wsum[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int u = __shfl_up(inc, off, 64);
    if (lane >= off) inc += u;
  }
  __syncthreads();
  if (lane == 63) wsum[w] = inc;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k < w) before += wsum[k];
    total += wsum[k];
  }
  return before + inc - v;
}

// ---- 1. binning: bin = #{thresholds < x} (sklearn's _map_col_to_bins, a value equal to a threshold goes left) --------
__global__ void __launch_bounds__(256) fit_bin_kernel(const double* __restrict__ X, int n, int F,
                                                      const double* __restrict__ thr, const int32_t* __restrict__ nthr,
                                                      uint8_t* __restrict__ bins, int64_t ld) {
  const int64_t total = (int64_t)n * F;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int i = (int)(e / F), f = (int)(e - (int64_t)i * F);
    const double x = X[e];
    const double* t = thr + (size_t)f * kBins;
    int lo = 0, hi = nthr[f];  // first index with t[idx] >= x
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (t[mid] < x) lo = mid + 1; else hi = mid;
    }
    bins[(size_t)f * ld + i] = (uint8_t)lo;
  }
}

// ---- 2. gradients of the half squared error: float32(raw - y), the difference in float64 -----------------------------
__global__ void __launch_bounds__(256) fit_grad_kernel(const double* __restrict__ raw, const double* __restrict__ y,
                                                       float* __restrict__ g, int32_t* __restrict__ part, int n) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    g[i] = (float)(raw[i] - y[i]);
    if (part) part[i] = i;
  }
}

// ---- 3. histogram -----------------------------------------------------------------------------------------------------
// grid (kRanges, ceil(F / 4)), 256 threads: wave w of block (r, q) owns feature 4 q + w over row range r of the segment;
// lane l owns bins l, l + 64, l + 128, l + 192 and adds the range's rows in order.
__global__ void __launch_bounds__(256) fit_hist_kernel(const Job* __restrict__ job, const uint8_t* __restrict__ bins,
                                                       int64_t ld, int F, const int32_t* __restrict__ part,
                                                       const float* __restrict__ grad, double* __restrict__ psum,
                                                       uint32_t* __restrict__ pcnt) {
  if (!job->active || !job->build) return;
  const int count = job->hcount, start = job->hstart;
  const int nr = ranges_of(count), r = blockIdx.x;
  if (r >= nr) return;
  const int lane = threadIdx.x & 63, f = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (f >= F) return;
  const int len = (((count + nr - 1) / nr + 63) / 64) * 64;
  const int lo = r * len, hi = min(count, lo + len);
  const uint8_t* col = bins + (size_t)f * ld;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  for (int i0 = lo; i0 < hi; i0 += 64) {
    const int i = i0 + lane;
    int bv = kNoBin;
    float gv = 0.f;
    if (i < hi) {
      const int row = part[start + i];
      bv = col[row];
      gv = grad[row];
    }
    const int gi = __float_as_int(gv);
#pragma unroll
    for (int j = 0; j < 64; ++j) {
      const int b = __builtin_amdgcn_readlane(bv, j);  // wave-uniform
      const float g = __int_as_float(__builtin_amdgcn_readlane(gi, j));
      const bool mine = (b & 63) == lane;
      const double ad = (double)(mine ? g : 0.f);
      const uint32_t ci = mine ? 1u : 0u;
      switch (b >> 6) {
        case 0: a0 += ad; c0 += ci; break;
        case 1: a1 += ad; c1 += ci; break;
        case 2: a2 += ad; c2 += ci; break;
        case 3: a3 += ad; c3 += ci; break;
        default: break;
      }
    }
  }
  const size_t o = ((size_t)r * F + f) * kBins + lane;
  psum[o] = a0; psum[o + 64] = a1; psum[o + 128] = a2; psum[o + 192] = a3;
  pcnt[o] = c0; pcnt[o + 64] = c1; pcnt[o + 128] = c2; pcnt[o + 192] = c3;
}

// grid F, 256 threads: the range partials summed in range order into slot `small`; slot `large` = parent - small
// (sklearn's compute_histograms_subtraction, element-wise in float64)
__global__ void __launch_bounds__(256) fit_hist_finish_kernel(const Job* __restrict__ job, int F,
                                                              const double* __restrict__ psum,
                                                              const uint32_t* __restrict__ pcnt,
                                                              double* __restrict__ hsum, uint32_t* __restrict__ hcnt) {
  if (!job->active || !job->build) return;
  const int nr = ranges_of(job->hcount);
  const int f = blockIdx.x, b = threadIdx.x;
  const size_t fb = (size_t)f * kBins + b, slot = (size_t)F * kBins;
  double s = psum[fb];
  uint32_t c = pcnt[fb];
  for (int r = 1; r < nr; ++r) {
    s += psum[(size_t)r * slot + fb];
    c += pcnt[(size_t)r * slot + fb];
  }
  hsum[job->small * slot + fb] = s;
  hcnt[job->small * slot + fb] = c;
  if (job->large >= 0) {
    hsum[job->large * slot + fb] = hsum[job->parent * slot + fb] - s;
    hcnt[job->large * slot + fb] = hcnt[job->parent * slot + fb] - c;
  }
}

// ---- 4. best split of a node, per feature -----------------------------------------------------------------------------
// grid (F, 2), 256 threads.  Thread 0 forms the left sums bin after bin (sklearn's scan order), thread b evaluates the
// split after bin b: gain = loss(node) - loss(left) - loss(right), loss = g * value, every product rounded on its own.
__global__ void __launch_bounds__(256) fit_split_kernel(const Job* __restrict__ job, int F,
                                                        const int32_t* __restrict__ nthr,
                                                        const double* __restrict__ hsum,
                                                        const uint32_t* __restrict__ hcnt, int min_samples_leaf, double l2,
                                                        Best* __restrict__ best) {
  if (!job->active) return;
  const int which = blockIdx.y, slot = job->split[which];
  if (slot < 0) return;
  __shared__ double sl[kBins];
  __shared__ int cl[kBins];
  __shared__ double gn[kBins];
  __shared__ int gb[kBins];
  const int f = blockIdx.x, b = threadIdx.x;
  const int n = job->split_n[which];
  const double G = job->split_g[which];
  const size_t base = ((size_t)slot * F + f) * kBins;
  const int nt = nthr[f];
  sl[b] = hsum[base + b];
  cl[b] = (int)hcnt[base + b];
  __syncthreads();
  if (b == 0) {
    double s = 0.0;
    int c = 0;
    for (int k = 0; k < nt; ++k) {
      s += sl[k];
      c += cl[k];
      sl[k] = s;
      cl[k] = c;
    }
  }
  __syncthreads();
  double gain = -1.0;
  if (b < nt) {
    const int nl = cl[b], nrr = n - nl;
    if (nl >= min_samples_leaf && nrr >= min_samples_leaf) {
      const double gL = sl[b], gR = G - gL;
      const double vP = node_value(G, (double)n, l2);
      const double vL = node_value(gL, (double)nl, l2), vR = node_value(gR, (double)n - (double)nl, l2);
      double t = gcl::rounded(G * vP);
      t -= gcl::rounded(gL * vL);
      t -= gcl::rounded(gR * vR);
      if (t > 0.0) gain = t;
    }
  }
  gn[b] = gain;
  gb[b] = b;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {  // largest gain, the lowest bin among equals
    if (b < off) {
      const double g2 = gn[b + off];
      const int b2 = gb[b + off];
      if (g2 > gn[b] || (g2 == gn[b] && b2 < gb[b])) {
        gn[b] = g2;
        gb[b] = b2;
      }
    }
    __syncthreads();
  }
  if (b == 0) {
    Best o;
    o.gain = gn[0];
    o.bin = gb[0];
    o.n_left = gn[0] > 0.0 ? cl[gb[0]] : 0;
    o.sum_g_left = gn[0] > 0.0 ? sl[gb[0]] : 0.0;
    best[which * kMaxF + f] = o;
  }
}

// the best feature of a node: a later feature wins only with a strictly larger gain
__device__ int pick_feature(const Best* best, int F) {
  int bf = 0;
  for (int f = 1; f < F; ++f)
    if (best[f].gain > best[bf].gain) bf = f;
  return bf;
}

__device__ void absorb(Tree* t, Node* nodes, const Best* best, int F) {
  for (int w = 0; w < 2; ++w) {
    const int nd = t->pending[w];
    if (nd < 0) continue;
    const Best* bb = best + w * kMaxF;
    const int f = pick_feature(bb, F);
    Node& N = nodes[nd];
    N.gain = bb[f].gain;
    if (bb[f].gain > 0.0) {
      N.state = kSplittable;
      N.feat = f;
      N.bin = bb[f].bin;
      N.n_left = bb[f].n_left;
      N.sum_g_left = bb[f].sum_g_left;
    } else {
      N.state = kLeaf;
    }
    t->pending[w] = -1;
  }
}

// ---- 6a. start of a tree: the root's histogram job ---------------------------------------------------------------------
__global__ void fit_tree_begin_kernel(Job* job, Tree* t, Node* nodes, const int32_t* state, int max_iter, int n) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  Job j = {};
  t->skip = state[0] >= max_iter;
  t->n_nodes = 1;
  t->n_leaves = 1;
  t->pending[0] = t->pending[1] = -1;
  Node r = {};
  r.start = 0;
  r.count = n;
  r.state = kUnset;
  nodes[0] = r;
  j.active = !t->skip;
  j.build = 1;
  j.hstart = 0;
  j.hcount = n;
  j.small = 0;
  j.large = j.parent = -1;
  j.split[0] = j.split[1] = -1;  // the root's sum of gradients is known only after the histogram: fit_root_kernel
  *job = j;
}

// the root: sum of gradients = its histogram's feature 0 summed in bin order; a split is looked for unless
// n < 2 min_samples_leaf
__global__ void fit_root_kernel(Job* job, Tree* t, Node* nodes, const double* hsum, int min_samples_leaf, double l2) {
  if (threadIdx.x != 0 || blockIdx.x != 0 || t->skip) return;
  double s = 0.0;
  for (int b = 0; b < kBins; ++b) s += hsum[b];
  Node& r = nodes[0];
  r.sum_g = s;
  r.value = node_value(s, (double)r.count, l2);
  job->build = 0;
  if (r.count < 2 * min_samples_leaf) {
    r.state = kLeaf;
    return;
  }
  job->split[0] = 0;
  job->split_n[0] = r.count;
  job->split_g[0] = s;
  t->pending[0] = 0;
}

// ---- 6b. one round: take in the last round's splits, pick the leaf with the largest gain, make its children ------------
__global__ void fit_select_kernel(Job* job, Tree* t, Node* nodes, const Best* best, int F, int max_leaf_nodes,
                                  int max_depth, int min_samples_leaf, double l2, int last) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  Job j = {};
  j.split[0] = j.split[1] = -1;
  j.large = j.parent = -1;
  if (t->skip) {
    *job = j;
    return;
  }
  absorb(t, nodes, best, F);
  int pick = -1;
  if (!last)
    for (int k = 0; k < t->n_nodes; ++k)
      if (nodes[k].state == kSplittable && (pick < 0 || nodes[k].gain > nodes[pick].gain)) pick = k;
  if (pick < 0) {  // nothing (more) to split: what is still splittable stays a leaf
    for (int k = 0; k < t->n_nodes; ++k)
      if (nodes[k].state == kSplittable) nodes[k].state = kLeaf;
    *job = j;
    return;
  }
  Node& P = nodes[pick];
  const int li = t->n_nodes, ri = li + 1;
  t->n_nodes += 2;
  t->n_leaves += 1;
  Node Lc = {}, Rc = {};
  Lc.start = P.start;
  Lc.count = P.n_left;
  Rc.start = P.start + P.n_left;
  Rc.count = P.count - P.n_left;
  Lc.depth = Rc.depth = P.depth + 1;
  Lc.sum_g = P.sum_g_left;
  Rc.sum_g = P.sum_g - P.sum_g_left;
  Lc.value = node_value(Lc.sum_g, (double)Lc.count, l2);
  Rc.value = node_value(Rc.sum_g, (double)P.count - (double)Lc.count, l2);
  P.state = kSplit;
  P.left = li;
  P.right = ri;
  P.missing_left = Lc.count > Rc.count;
  j.active = 1;
  j.start = P.start;
  j.count = P.count;
  j.feat = P.feat;
  j.bin = P.bin;
  if (t->n_leaves == max_leaf_nodes) {
    Lc.state = Rc.state = kLeaf;
    for (int k = 0; k < li; ++k)
      if (nodes[k].state == kSplittable) nodes[k].state = kLeaf;
  } else if (Lc.depth == max_depth) {
    Lc.state = Rc.state = kLeaf;
  } else {
    Lc.state = Lc.count < 2 * min_samples_leaf ? kLeaf : kUnset;
    Rc.state = Rc.count < 2 * min_samples_leaf ? kLeaf : kUnset;
  }
  if (Lc.state == kUnset || Rc.state == kUnset) {  // the smaller child is built (the right one on a tie)
    const bool left_small = Lc.count < Rc.count;
    const Node& S = left_small ? Lc : Rc;
    j.build = 1;
    j.hstart = S.start;
    j.hcount = S.count;
    j.small = left_small ? li : ri;
    j.large = left_small ? ri : li;
    j.parent = pick;
    if (Lc.state == kUnset) {
      j.split[0] = li;
      j.split_n[0] = Lc.count;
      j.split_g[0] = Lc.sum_g;
      t->pending[0] = li;
    }
    if (Rc.state == kUnset) {
      j.split[1] = ri;
      j.split_n[1] = Rc.count;
      j.split_g[1] = Rc.sum_g;
      t->pending[1] = ri;
    }
  }
  nodes[li] = Lc;
  nodes[ri] = Rc;
  *job = j;
}

// ---- 5. stable partition of the job's segment ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) fit_part_count_kernel(const Job* __restrict__ job,
                                                             const uint8_t* __restrict__ bins, int64_t ld,
                                                             const int32_t* __restrict__ part, int32_t* __restrict__ cnts) {
  if (!job->active) return;
  const int count = job->count, c0 = blockIdx.x * kChunk;
  if (c0 >= count) return;
  const uint8_t* col = bins + (size_t)job->feat * ld;
  const int bin = job->bin, start = job->start;
  int v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = c0 + threadIdx.x * 4 + k;
    if (i < count) v += col[part[start + i]] <= bin;
  }
  int total;
  block_excl_scan(v, total);
  if (threadIdx.x == 0) cnts[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) fit_part_scatter_kernel(const Job* __restrict__ job,
                                                               const uint8_t* __restrict__ bins, int64_t ld,
                                                               const int32_t* __restrict__ part,
                                                               const int32_t* __restrict__ cnts, int32_t* __restrict__ tmp,
                                                               int32_t* __restrict__ n_left_out) {
  if (!job->active) return;
  const int count = job->count, c0 = blockIdx.x * kChunk;
  if (c0 >= count) return;
  const int nchunks = (count + kChunk - 1) / kChunk;
  int before = 0, all = 0;  // left rows of the chunks before this one, and of the segment
  for (int c = threadIdx.x; c < nchunks; c += 256) {
    const int v = cnts[c];
    all += v;
    if (c < (int)blockIdx.x) before += v;
  }
  __shared__ int red[2][4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    before += __shfl_xor(before, off, 64);
    all += __shfl_xor(all, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = before;
    red[1][threadIdx.x >> 6] = all;
  }
  __syncthreads();
  before = red[0][0] + red[0][1] + red[0][2] + red[0][3];
  all = red[1][0] + red[1][1] + red[1][2] + red[1][3];
  const uint8_t* col = bins + (size_t)job->feat * ld;
  const int bin = job->bin, start = job->start;
  int rows[4], fl[4], v = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = c0 + threadIdx.x * 4 + k;
    rows[k] = i < count ? part[start + i] : 0;
    fl[k] = i < count ? (int)(col[rows[k]] <= bin) : 0;
    v += fl[k];
  }
  int total;
  int lrank = before + block_excl_scan(v, total);  // left rows before this thread's first row
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = c0 + threadIdx.x * 4 + k;
    if (i < count) {
      const int dst = fl[k] ? lrank : all + (i - lrank);
      tmp[start + dst] = rows[k];
      lrank += fl[k];
    }
  }
  if (n_left_out && blockIdx.x == 0 && threadIdx.x == 0) *n_left_out = all;
}

__global__ void __launch_bounds__(256) fit_part_copy_kernel(const Job* __restrict__ job, const int32_t* __restrict__ tmp,
                                                            int32_t* __restrict__ part) {
  if (!job->active) return;
  const int count = job->count, start = job->start;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = blockIdx.x * kChunk + k * 256 + threadIdx.x;
    if (i < count) part[start + i] = tmp[start + i];
  }
}

// ---- 6c. end of a tree: the nodes in MOSForest's 16-byte layout, the leaf table -----------------------------------------
struct PackedNode {
  double v;
  uint32_t left, meta;
};

__global__ void fit_tree_end_kernel(Tree* t, Node* nodes, const double* __restrict__ thr, double learning_rate,
                                    const int32_t* state, PackedNode* out, int32_t* roots, int32_t* leaf_start,
                                    int32_t* leaf_count, double* leaf_value) {
  if (threadIdx.x != 0 || blockIdx.x != 0 || t->skip) return;
  const int base = state[1];
  int nl = 0;
  for (int k = 0; k < t->n_nodes; ++k) {
    Node& N = nodes[k];
    PackedNode p;
    if (N.state == kSplit) {
      p.v = thr[(size_t)N.feat * kBins + N.bin];
      p.left = (uint32_t)(base + N.left);
      p.meta = (uint32_t)(base + N.right) | ((uint32_t)N.feat << 24) | ((uint32_t)N.missing_left << 29);
    } else {
      N.value = gcl::rounded(N.value * learning_rate);
      p.v = N.value;
      p.left = 0;
      p.meta = 1u << 30;
      leaf_start[nl] = N.start;
      leaf_count[nl] = N.count;
      leaf_value[nl] = N.value;
      ++nl;
    }
    out[base + k] = p;
  }
  t->n_final_leaves = nl;
  roots[state[0]] = base;
}

// raw[row] += value of the leaf whose segment holds the row's position (the leaves tile [0, n): once per row)
__global__ void __launch_bounds__(256) fit_update_raw_kernel(const Tree* __restrict__ t, const int32_t* __restrict__ part,
                                                             const int32_t* __restrict__ leaf_start,
                                                             const int32_t* __restrict__ leaf_count,
                                                             const double* __restrict__ leaf_value,
                                                             double* __restrict__ raw, int n) {
  if (t->skip) return;
  __shared__ int ls[kMaxLeaves], lc[kMaxLeaves];
  __shared__ double lv[kMaxLeaves];
  const int nl = t->n_final_leaves;
  for (int k = threadIdx.x; k < nl; k += 256) {
    ls[k] = leaf_start[k];
    lc[k] = leaf_count[k];
    lv[k] = leaf_value[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = blockIdx.x * kChunk + k * 256 + threadIdx.x;
    if (i >= n) continue;
    for (int q = 0; q < nl; ++q)
      if (i >= ls[q] && i < ls[q] + lc[q]) {
        raw[part[i]] += lv[q];
        break;
      }
  }
}

// the validation rows walk the new tree on their bins (sklearn's predict_binned); block partial of (raw - y)^2
__global__ void __launch_bounds__(256) fit_val_kernel(const Tree* __restrict__ t, const Node* __restrict__ nodes,
                                                      const uint8_t* __restrict__ bins, int64_t ld,
                                                      double* __restrict__ raw, const double* __restrict__ y, int n,
                                                      double* __restrict__ spart, int walk) {
  if (walk && t->skip) return;
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = blockIdx.x * kChunk + k * 256 + threadIdx.x;
    if (i >= n) continue;
    double r = raw[i];
    if (walk) {
      int nd = 0;
      while (nodes[nd].state == kSplit)
        nd = bins[(size_t)nodes[nd].feat * ld + i] <= nodes[nd].bin ? nodes[nd].left : nodes[nd].right;
      r += nodes[nd].value;
      raw[i] = r;
    }
    const double d = r - y[i];
    s += gcl::rounded(d * d);
  }
  __shared__ double ws4[4];
  s = gcl::wave_sum(s);
  if ((threadIdx.x & 63) == 0) ws4[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) spart[blockIdx.x] = ((ws4[0] + ws4[1]) + ws4[2]) + ws4[3];
}

// one block: the block partials in a fixed order; score = -0.5 mean (sklearn's validation score of the squared error).
// With `state` it also closes the iteration: state[0] += 1 tree, state[1] += its nodes.
__global__ void __launch_bounds__(256) fit_score_kernel(const Tree* t, const double* __restrict__ spart, int nparts,
                                                        int n, double* scores, int32_t* state) {
  if (state && t->skip) return;
  if (n > 0) {
    double s = 0.0;
    for (int k = threadIdx.x; k < nparts; k += 256) s += spart[k];
    __shared__ double ws4[4];
    s = gcl::wave_sum(s);
    if ((threadIdx.x & 63) == 0) ws4[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      const double tot = ((ws4[0] + ws4[1]) + ws4[2]) + ws4[3];
      scores[state ? state[0] + 1 : 0] = -0.5 * (tot / (double)n);
    }
  }
  if (state && threadIdx.x == 0) {
    state[0] += 1;
    state[1] += t->n_nodes;
  }
}

__global__ void fit_set_job_kernel(Job* job, Job v) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *job = v;
}

__global__ void fit_split_out_kernel(const Best* best, int F, int n, double* out, int32_t* iout) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int f = pick_feature(best, F);
  out[0] = best[f].gain;
  out[1] = best[f].sum_g_left;
  iout[0] = f;
  iout[1] = best[f].bin;
  iout[2] = best[f].n_left;
  iout[3] = best[f].n_left > n - best[f].n_left;
}

__global__ void __launch_bounds__(256) fit_hist_sub_kernel(const double* ps, const uint32_t* pc, const double* ss,
                                                           const uint32_t* sc, double* ls, uint32_t* lc, int total) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < total) {
    ls[i] = ps[i] - ss[i];
    lc[i] = pc[i] - sc[i];
  }
}

unsigned chunks(int64_t n) { return (unsigned)gcl::cdiv(n > 0 ? n : 1, kChunk); }

}  // namespace

extern "C" {

size_t gcl_mos_fit_ws_bytes(int32_t n, int32_t n_val, int32_t F, int32_t max_leaf_nodes, int32_t max_iter) {
  (void)max_iter;  // the node buffer is the caller's
  if (n < 0 || n_val < 0 || F < 1 || F > kMaxF || max_leaf_nodes < 2 || max_leaf_nodes > kMaxLeaves) return 0;
  return layout(n, n_val, F, max_leaf_nodes).total;
}

int gcl_mos_fit_bin(const double* X, int32_t n, int32_t F, const double* thr, const int32_t* nthr, void* bins, int64_t ld,
                    gcl_stream_t stream) {
  GCL_CHECK_ARG(X && thr && nthr && bins, "gcl_mos_fit_bin: null pointer");
  GCL_CHECK_ARG(n >= 1 && F >= 1 && F <= kMaxF && ld >= n, "gcl_mos_fit_bin: bad n=%d F=%d ld=%lld", n, F, (long long)ld);
  fit_bin_kernel<<<gcl::grid_for((int64_t)n * F), 256, 0, (hipStream_t)stream>>>(X, n, F, thr, nthr, (uint8_t*)bins, ld);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_mos_fit_gradients(const double* raw, const double* y, float* g, int32_t n, gcl_stream_t stream) {
  GCL_CHECK_ARG(raw && y && g && n >= 1, "gcl_mos_fit_gradients: bad arguments");
  fit_grad_kernel<<<gcl::grid_for(n), 256, 0, (hipStream_t)stream>>>(raw, y, g, nullptr, n);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_mos_fit_histogram(const void* bins, int64_t ld, int32_t F, const int32_t* part, const float* g, int32_t start,
                          int32_t count, double* hist_sum, void* hist_cnt, void* ws, size_t ws_bytes,
                          gcl_stream_t stream) {
  GCL_CHECK_ARG(bins && part && g && hist_sum && hist_cnt && ws, "gcl_mos_fit_histogram: null pointer");
  GCL_CHECK_ARG(F >= 1 && F <= kMaxF && start >= 0 && count >= 1 && (int64_t)start + count <= INT32_MAX,
                "gcl_mos_fit_histogram: bad F=%d start=%d count=%d", F, start, count);
  const Layout L = layout(0, 0, F, 2);
  GCL_CHECK_ARG(ws_bytes >= L.total, "gcl_mos_fit_histogram: workspace of %zu bytes, %zu needed", ws_bytes, L.total);
  hipStream_t st = (hipStream_t)stream;
  Job j = {};
  j.active = j.build = 1;
  j.hstart = start;
  j.hcount = count;
  j.small = 0;
  j.large = j.parent = -1;
  j.split[0] = j.split[1] = -1;
  Job* job = at<Job>(ws, L.job);
  fit_set_job_kernel<<<1, 1, 0, st>>>(job, j);
  fit_hist_kernel<<<dim3(kRanges, (F + 3) / 4), 256, 0, st>>>(job, (const uint8_t*)bins, ld, F, part, g,
                                                              at<double>(ws, L.psum), at<uint32_t>(ws, L.pcnt));
  fit_hist_finish_kernel<<<F, 256, 0, st>>>(job, F, at<double>(ws, L.psum), at<uint32_t>(ws, L.pcnt),
                                            at<double>(ws, L.hsum), at<uint32_t>(ws, L.hcnt));
  GCL_CHECK_LAUNCH();
  GCL_CHECK_HIP(hipMemcpyAsync(hist_sum, at<double>(ws, L.hsum), 8 * (size_t)F * kBins, hipMemcpyDeviceToDevice, st));
  GCL_CHECK_HIP(hipMemcpyAsync(hist_cnt, at<uint32_t>(ws, L.hcnt), 4 * (size_t)F * kBins, hipMemcpyDeviceToDevice, st));
  return GCL_OK;
}

int gcl_mos_fit_hist_subtract(const double* parent_sum, const void* parent_cnt, const double* small_sum,
                              const void* small_cnt, double* large_sum, void* large_cnt, int32_t F,
                              gcl_stream_t stream) {
  GCL_CHECK_ARG(parent_sum && parent_cnt && small_sum && small_cnt && large_sum && large_cnt && F >= 1 && F <= kMaxF,
                "gcl_mos_fit_hist_subtract: bad arguments");
  fit_hist_sub_kernel<<<F, 256, 0, (hipStream_t)stream>>>(parent_sum, (const uint32_t*)parent_cnt, small_sum,
                                                          (const uint32_t*)small_cnt, large_sum, (uint32_t*)large_cnt,
                                                          F * kBins);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_mos_fit_split(const double* hist_sum, const void* hist_cnt, int32_t F, const int32_t* nthr, int32_t n,
                      double sum_g, int32_t min_samples_leaf, double l2, double* out, int32_t* iout, void* ws,
                      size_t ws_bytes, gcl_stream_t stream) {
  GCL_CHECK_ARG(hist_sum && hist_cnt && nthr && out && iout && ws, "gcl_mos_fit_split: null pointer");
  GCL_CHECK_ARG(F >= 1 && F <= kMaxF && n >= 1 && min_samples_leaf >= 1, "gcl_mos_fit_split: bad F=%d n=%d", F, n);
  const Layout L = layout(0, 0, F, 2);
  GCL_CHECK_ARG(ws_bytes >= L.total, "gcl_mos_fit_split: workspace of %zu bytes, %zu needed", ws_bytes, L.total);
  hipStream_t st = (hipStream_t)stream;
  GCL_CHECK_HIP(hipMemcpyAsync(at<double>(ws, L.hsum), hist_sum, 8 * (size_t)F * kBins, hipMemcpyDeviceToDevice, st));
  GCL_CHECK_HIP(hipMemcpyAsync(at<uint32_t>(ws, L.hcnt), hist_cnt, 4 * (size_t)F * kBins, hipMemcpyDeviceToDevice, st));
  Job j = {};
  j.active = 1;
  j.large = j.parent = -1;
  j.split[0] = 0;
  j.split[1] = -1;
  j.split_n[0] = n;
  j.split_g[0] = sum_g;
  Job* job = at<Job>(ws, L.job);
  fit_set_job_kernel<<<1, 1, 0, st>>>(job, j);
  fit_split_kernel<<<dim3(F, 2), 256, 0, st>>>(job, F, nthr, at<double>(ws, L.hsum), at<uint32_t>(ws, L.hcnt),
                                               min_samples_leaf, l2, at<Best>(ws, L.best));
  fit_split_out_kernel<<<1, 1, 0, st>>>(at<Best>(ws, L.best), F, n, out, iout);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_mos_fit_partition(const void* bins, int64_t ld, int32_t* part, int32_t start, int32_t count, int32_t feat,
                          int32_t bin, int32_t* n_left, void* ws, size_t ws_bytes, gcl_stream_t stream) {
  GCL_CHECK_ARG(bins && part && ws, "gcl_mos_fit_partition: null pointer");
  GCL_CHECK_ARG(start >= 0 && count >= 1 && (int64_t)start + count <= INT32_MAX && feat >= 0 && feat < kMaxF &&
                    bin >= 0 && bin < kBins,
                "gcl_mos_fit_partition: bad start=%d count=%d feat=%d bin=%d", start, count, feat, bin);
  const Layout L = layout((int64_t)start + count, 0, 1, 2);
  GCL_CHECK_ARG(ws_bytes >= L.total, "gcl_mos_fit_partition: workspace of %zu bytes, %zu needed", ws_bytes, L.total);
  hipStream_t st = (hipStream_t)stream;
  Job j = {};
  j.active = 1;
  j.start = start;
  j.count = count;
  j.feat = feat;
  j.bin = bin;
  j.large = j.parent = -1;
  j.split[0] = j.split[1] = -1;
  Job* job = at<Job>(ws, L.job);
  const unsigned nb = chunks(count);
  fit_set_job_kernel<<<1, 1, 0, st>>>(job, j);
  fit_part_count_kernel<<<nb, 256, 0, st>>>(job, (const uint8_t*)bins, ld, part, at<int32_t>(ws, L.cnts));
  fit_part_scatter_kernel<<<nb, 256, 0, st>>>(job, (const uint8_t*)bins, ld, part, at<int32_t>(ws, L.cnts),
                                              at<int32_t>(ws, L.tmp), n_left);
  fit_part_copy_kernel<<<nb, 256, 0, st>>>(job, at<int32_t>(ws, L.tmp), part);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_mos_fit_score(const double* raw, const double* y, int32_t n, double* score, void* ws, size_t ws_bytes,
                      gcl_stream_t stream) {
  GCL_CHECK_ARG(raw && y && score && ws && n >= 1, "gcl_mos_fit_score: bad arguments");
  const Layout L = layout(0, n, 1, 2);
  GCL_CHECK_ARG(ws_bytes >= L.total, "gcl_mos_fit_score: workspace of %zu bytes, %zu needed", ws_bytes, L.total);
  hipStream_t st = (hipStream_t)stream;
  const unsigned nb = chunks(n);
  fit_val_kernel<<<nb, 256, 0, st>>>(nullptr, nullptr, nullptr, 0, const_cast<double*>(raw), y, n,
                                     at<double>(ws, L.spart), 0);
  fit_score_kernel<<<1, 256, 0, st>>>(nullptr, at<double>(ws, L.spart), (int)nb, n, score, nullptr);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

int gcl_mos_fit_tree(const void* bins, int64_t ld, int32_t n, int32_t F, const int32_t* nthr, const double* thr,
                     const double* y, double* raw, const void* bins_val, int64_t ld_val, int32_t n_val,
                     const double* y_val, double* raw_val, int32_t max_leaf_nodes, int32_t max_depth,
                     int32_t min_samples_leaf, double l2, double learning_rate, int32_t max_iter, void* nodes,
                     int32_t* roots, double* scores, int32_t* state, void* ws, size_t ws_bytes, gcl_stream_t stream) {
  GCL_CHECK_ARG(bins && nthr && thr && y && raw && nodes && roots && state && ws, "gcl_mos_fit_tree: null pointer");
  GCL_CHECK_ARG(n >= 1 && F >= 1 && F <= kMaxF && ld >= n, "gcl_mos_fit_tree: bad n=%d F=%d ld=%lld", n, F,
                (long long)ld);
  GCL_CHECK_ARG(max_leaf_nodes >= 2 && max_leaf_nodes <= kMaxLeaves && max_depth >= 1 && min_samples_leaf >= 1 &&
                    max_iter >= 1,
                "gcl_mos_fit_tree: bad max_leaf_nodes=%d max_depth=%d min_samples_leaf=%d max_iter=%d", max_leaf_nodes,
                max_depth, min_samples_leaf, max_iter);
  GCL_CHECK_ARG(n_val == 0 || (n_val > 0 && bins_val && y_val && raw_val && scores && ld_val >= n_val),
                "gcl_mos_fit_tree: bad validation arguments (n_val=%d)", n_val);
  const Layout L = layout(n, n_val, F, max_leaf_nodes);
  GCL_CHECK_ARG(ws_bytes >= L.total, "gcl_mos_fit_tree: workspace of %zu bytes, %zu needed", ws_bytes, L.total);
  hipStream_t st = (hipStream_t)stream;
  Job* job = at<Job>(ws, L.job);
  Tree* t = at<Tree>(ws, L.tree);
  Node* nd = at<Node>(ws, L.nodes);
  Best* best = at<Best>(ws, L.best);
  int32_t* part = at<int32_t>(ws, L.part);
  int32_t* tmp = at<int32_t>(ws, L.tmp);
  float* grad = at<float>(ws, L.grad);
  int32_t* cnts = at<int32_t>(ws, L.cnts);
  double* psum = at<double>(ws, L.psum);
  uint32_t* pcnt = at<uint32_t>(ws, L.pcnt);
  double* hsum = at<double>(ws, L.hsum);
  uint32_t* hcnt = at<uint32_t>(ws, L.hcnt);
  const uint8_t* b8 = (const uint8_t*)bins;
  const unsigned nb = chunks(n);
  const dim3 hgrid(kRanges, (F + 3) / 4), sgrid(F, 2);

  fit_grad_kernel<<<gcl::grid_for(n), 256, 0, st>>>(raw, y, grad, part, n);
  fit_tree_begin_kernel<<<1, 1, 0, st>>>(job, t, nd, state, max_iter, n);
  fit_hist_kernel<<<hgrid, 256, 0, st>>>(job, b8, ld, F, part, grad, psum, pcnt);
  fit_hist_finish_kernel<<<F, 256, 0, st>>>(job, F, psum, pcnt, hsum, hcnt);
  fit_root_kernel<<<1, 1, 0, st>>>(job, t, nd, hsum, min_samples_leaf, l2);
  fit_split_kernel<<<sgrid, 256, 0, st>>>(job, F, nthr, hsum, hcnt, min_samples_leaf, l2, best);
  for (int r = 0; r < max_leaf_nodes; ++r) {  // the last pass only takes in the last split's results
    const int last = r == max_leaf_nodes - 1;
    fit_select_kernel<<<1, 1, 0, st>>>(job, t, nd, best, F, max_leaf_nodes, max_depth, min_samples_leaf, l2, last);
    if (last) break;
    fit_part_count_kernel<<<nb, 256, 0, st>>>(job, b8, ld, part, cnts);
    fit_part_scatter_kernel<<<nb, 256, 0, st>>>(job, b8, ld, part, cnts, tmp, nullptr);
    fit_part_copy_kernel<<<nb, 256, 0, st>>>(job, tmp, part);
    fit_hist_kernel<<<hgrid, 256, 0, st>>>(job, b8, ld, F, part, grad, psum, pcnt);
    fit_hist_finish_kernel<<<F, 256, 0, st>>>(job, F, psum, pcnt, hsum, hcnt);
    fit_split_kernel<<<sgrid, 256, 0, st>>>(job, F, nthr, hsum, hcnt, min_samples_leaf, l2, best);
  }
  fit_tree_end_kernel<<<1, 1, 0, st>>>(t, nd, thr, learning_rate, state, (PackedNode*)nodes, roots,
                                       at<int32_t>(ws, L.leaf_start), at<int32_t>(ws, L.leaf_count),
                                       at<double>(ws, L.leaf_value));
  fit_update_raw_kernel<<<nb, 256, 0, st>>>(t, part, at<int32_t>(ws, L.leaf_start), at<int32_t>(ws, L.leaf_count),
                                            at<double>(ws, L.leaf_value), raw, n);
  const unsigned nbv = chunks(n_val);
  if (n_val > 0)
    fit_val_kernel<<<nbv, 256, 0, st>>>(t, nd, (const uint8_t*)bins_val, ld_val, raw_val, y_val, n_val,
                                        at<double>(ws, L.spart), 1);
  fit_score_kernel<<<1, 256, 0, st>>>(t, at<double>(ws, L.spart), (int)nbv, n_val, scores, state);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

}  // extern "C"
