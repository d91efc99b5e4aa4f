// MOS correction of 2 m temperature (src/postprocessing/mos_correction.py).
//
// Forest.  A HistGradientBoostingRegressor flattened into 16-byte nodes (see MosNode): a split holds its threshold, a
// leaf its value.  sklearn's walk (_predictor.pyx): NaN follows missing_go_to_left, otherwise x <= threshold goes
// left.  The raw prediction is ((baseline + v0) + v1) + ... in float64, tree order, as _raw_predict adds it.
//
// Station recurrence (gcl_mos_forest_predict, mos_correction.py:307-323).  One block per (sample, station group),
// the steps in order: the lag features of step s are the group's corrected t2m of step s - 1.  Per step the block
// builds every station's 20 features in LDS, walks every (station, tree) pair over its lanes into an LDS leaf table,
// sums each station's leaves in tree order (one lane per station), and one lane averages the group in numpy's
// pairwise order.
//
// IDW spread and apply (gcl_mos_idw_apply, mos_correction.py:176-241 and :325-338).  One thread per grid row.  The
// station points' coordinates and a tile of their per-step biases sit in LDS.  The weights 1 / max(d, 0.1)^p of the
// points within the radius are normalised by their numpy sum; the field is sum_k w_k b_k[s], added point by point in
// float64 (numpy's axis-0 sum; a single step sums pairwise).  A station's own grid row takes its exact bias.
//
// hipcc contracts a product into the following add even through __dmul_rn, so every product whose rounding the
// reference keeps passes through `rounded` (an empty asm volatile, as in assim.hip / verify.hip).
#include <math.h>

#include "common.h"

namespace {

using gcl::rounded;  // products rounded on their own, never contracted (common.h)

constexpr int kNumFeat = 20;   // FEATURE_COLUMNS of build_learned_mos.py
constexpr int kNumTime = 8;    // host features per (sample, station, step): hour sin/cos, doy sin/cos, solar
                               // elevation, station lat / lon / elev
constexpr int kMaxPoints = 128;     // station groups (IDW points) and stations per group
constexpr int kForestThreads = 256;
constexpr int kLeafBudget = 48 * 1024;  // bytes of leaf table per pass of the forest kernel
constexpr int kIdwThreads = 128;
constexpr int kStepTile = 16;           // steps per LDS bias tile of the IDW kernel
constexpr int kSweepRows = 64;          // grid rows per block of the sweep kernel: one per lane of a wave
constexpr int kSweepThreads = 256;      // its block: four waves share the distances, wave 0 walks the settings
constexpr int kSweepMaxConfigs = 64;    // settings per launch
constexpr int kSweepFinalThreads = 256;

// One forest node: v = threshold (split) or value (leaf); a = left child; b = right child (bits 0-23), feature
// (24-28), missing_go_to_left (29), is_leaf (30).  Child indices are global (into the whole forest).
struct __attribute__((aligned(16))) MosNode {
  double v;
  uint32_t a, b;
};

__device__ __forceinline__ double walk_tree(const MosNode* __restrict__ nodes, int root, const double* f) {
  int i = root;
  for (;;) {
    const MosNode n = nodes[i];
    if (n.b & (1u << 30)) return n.v;
    const double x = f[(n.b >> 24) & 31u];
    const bool left = isnan(x) ? ((n.b >> 29) & 1u) != 0 : x <= n.v;
    i = left ? (int)n.a : (int)(n.b & 0xFFFFFFu);
  }
}

// numpy's float64 add.reduce of n (< 129) values streamed in order: sequential below 8, else eight interleaved
// accumulators, combined in a fixed tree, then the remainder (pairwise_sum, n <= PW_BLOCKSIZE).
struct NpSum {
  double r[8];
  double res;
  int n, i, body;
  __device__ explicit NpSum(int n_) : res(0.0), n(n_), i(0), body(n_ - n_ % 8) {
    for (int j = 0; j < 8; ++j) r[j] = 0.0;
  }
  __device__ void add(double x) {
    if (n < 8) {
      res += x;
    } else if (i < body) {
      // a select per accumulator instead of a dynamic register index (no scratch)
      const int lane = i & 7;
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = j == lane ? (i < 8 ? x : r[j] + x) : r[j];
    } else {
      if (i == body) res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
      res += x;
    }
    ++i;
  }
  __device__ double sum() const {
    // numpy starts the reduction from the identity: an all -0.0 input sums to +0.0 on every path
    if (n >= 8 && body == n) return 0.0 + (((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7])));
    return 0.0 + res;
  }
};

__device__ __forceinline__ double load_val(const void* p, int f64, int64_t off) {
  return f64 ? static_cast<const double*>(p)[off] : (double)static_cast<const float*>(p)[off];
}

// ------------------------------------------------------------------------------------------------------------------
// Forest on feature rows (sklearn predict)
// ------------------------------------------------------------------------------------------------------------------
__global__ void forest_eval_kernel(const MosNode* __restrict__ nodes, const int32_t* __restrict__ roots, int ntrees,
                                   double baseline, const double* __restrict__ X, int n, double* __restrict__ y) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  double f[kNumFeat];
#pragma unroll
  for (int j = 0; j < kNumFeat; ++j) f[j] = X[(int64_t)r * kNumFeat + j];
  double acc = baseline;
  for (int t = 0; t < ntrees; ++t) {
    int i = roots[t];
    for (;;) {
      const MosNode nd = nodes[i];
      if (nd.b & (1u << 30)) break;
      const int fi = (nd.b >> 24) & 31u;
      double x = f[0];
      // a select chain instead of a dynamic register index (no scratch)
#pragma unroll
      for (int j = 1; j < kNumFeat; ++j) x = fi == j ? f[j] : x;
      const bool left = isnan(x) ? ((nd.b >> 29) & 1u) != 0 : x <= nd.v;
      i = left ? (int)nd.a : (int)(nd.b & 0xFFFFFFu);
    }
    acc += nodes[i].v;
  }
  y[r] = acc;
}

// ------------------------------------------------------------------------------------------------------------------
// Station recurrence
// ------------------------------------------------------------------------------------------------------------------
struct Chans {
  int t2m, u, v, sp, tp;
};

__global__ void __launch_bounds__(kForestThreads)
forest_station_kernel(const MosNode* __restrict__ nodes, const int32_t* __restrict__ roots, int ntrees,
                      double baseline, const void* __restrict__ pred, int f64, int64_t bs, int64_t gs, int64_t ss,
                      int steps, Chans ch, const int32_t* __restrict__ grid_idx, const int32_t* __restrict__ gstart,
                      int nst, const double* __restrict__ tfeat, double* __restrict__ bias, double* __restrict__ fout,
                      int32_t* __restrict__ ncorr, int pass_max) {
  extern __shared__ double smem[];
  double* feat = smem;                            // [pass_max][kNumFeat]
  double* leaves = feat + pass_max * kNumFeat;    // [pass_max][ntrees]
  double* sbias = leaves + (size_t)pass_max * ntrees;  // [kMaxPoints]
  __shared__ double prev_s;

  const int g = blockIdx.x, b = blockIdx.y, ng = gridDim.x, tid = threadIdx.x;
  const int s0 = gstart[g], gsize = gstart[g + 1] - s0;
  if (g == 0 && tid == 0 && ncorr) ncorr[b] = 0;  // the IDW kernel that follows counts into it
  const char* row = (const char*)pred + (size_t)(f64 ? 8 : 4) * (size_t)(b * bs + (int64_t)grid_idx[g] * gs);
  const double qnan = __builtin_nan("");
  if (tid == 0) prev_s = qnan;
  __syncthreads();

  for (int s = 0; s < steps; ++s) {
    const int64_t so = s * ss;
    for (int p0 = 0; p0 < gsize; p0 += pass_max) {
      const int np = min(pass_max, gsize - p0);
      if (tid < np) {
        // _build_features_from_forecast (mos_correction.py:98-173), forecast part in float64
        const int st = s0 + p0 + tid;
        const double* tf = tfeat + (((int64_t)b * nst + st) * steps + s) * kNumTime;
        const double prev = prev_s;
        const double t2m_c = load_val(row, f64, so + ch.t2m) - 273.15;
        const double u = ch.u >= 0 ? load_val(row, f64, so + ch.u) : qnan;
        const double v = ch.v >= 0 ? load_val(row, f64, so + ch.v) : qnan;
        double ws = qnan, wsin = qnan, wcos = qnan;
        if (!isnan(u) && !isnan(v)) {
          ws = sqrt(rounded(u * u) + rounded(v * v));
          const double wd = atan2(-u, -v);
          wsin = sin(wd);
          wcos = cos(wd);
        }
        const double sp = ch.sp >= 0 ? load_val(row, f64, so + ch.sp) / 100.0 : qnan;
        const double tp = ch.tp >= 0 ? load_val(row, f64, so + ch.tp) : qnan;
        double* f = feat + tid * kNumFeat;
        f[0] = t2m_c;   f[1] = qnan;  f[2] = ws;     f[3] = wsin;   f[4] = wcos;
        f[5] = sp;      f[6] = qnan;  f[7] = qnan;   f[8] = tp;
        f[9] = tf[0];   f[10] = tf[1]; f[11] = tf[2]; f[12] = tf[3]; f[13] = tf[4];
        f[14] = qnan;   f[15] = prev;  f[16] = s == 0 ? qnan : t2m_c - prev;
        f[17] = tf[5];  f[18] = tf[6]; f[19] = tf[7];
        if (fout) {
          double* o = fout + (((int64_t)b * nst + st) * steps + s) * kNumFeat;
          for (int j = 0; j < kNumFeat; ++j) o[j] = f[j];
        }
      }
      __syncthreads();
      for (int idx = tid; idx < np * ntrees; idx += blockDim.x) {
        const int q = idx / ntrees, t = idx - q * ntrees;
        leaves[(size_t)q * ntrees + t] = walk_tree(nodes, roots[t], feat + q * kNumFeat);
      }
      __syncthreads();
      if (tid < np) {
        const double* lv = leaves + (size_t)tid * ntrees;
        double acc = baseline;
        for (int t = 0; t < ntrees; ++t) acc += lv[t];
        sbias[p0 + tid] = acc;
      }
      __syncthreads();
    }
    if (tid == 0) {
      // float(np.mean(biases)); prev_t2m_c = float(pred + bias) - 273.15 (mos_correction.py:320-322)
      NpSum m(gsize);
      for (int q = 0; q < gsize; ++q) m.add(sbias[q]);
      const double mean = m.sum() / (double)gsize;
      bias[((int64_t)b * ng + g) * steps + s] = mean;
      prev_s = (load_val(row, f64, so + ch.t2m) + mean) - 273.15;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------------------
// IDW spread and apply
// ------------------------------------------------------------------------------------------------------------------
// mos_correction.py:176-184, node (lat1, lon1) to point (lat2, lon2), float64, Python's operation order.
__device__ __forceinline__ double haversine_km(double lat1, double lon1, double lat2, double lon2) {
  const double d2r = 0.017453292519943295;  // math.radians: x * (pi / 180)
  const double dlat = rounded((lat2 - lat1) * d2r), dlon = rounded((lon2 - lon1) * d2r);
  const double sa = sin(dlat / 2), sb = sin(dlon / 2);
  const double cc = rounded(rounded(cos(rounded(lat1 * d2r)) * cos(rounded(lat2 * d2r))) * rounded(sb * sb));
  const double a = rounded(sa * sa) + cc;
  return rounded(6371.0 * 2 * atan2(sqrt(a), sqrt(1 - a)));
}

__device__ __forceinline__ double idw_raw_weight(double d, double power) {
  d = fmax(d, 0.1);
  const double dp = power == 2.0 ? rounded(d * d) : (power == 1.0 ? d : pow(d, power));
  return 1.0 / dp;
}

// The per-row IDW field, shared by idw_apply_kernel and idw_sweep_kernel so that the two cannot drift apart.  `dist(k)`
// is the row's haversine distance to point k, `wgt(k, d)` its raw weight idw_raw_weight(d, power); a kernel may
// compute them on the spot or read them back from where it kept them: the values, and so the bits, are the same.
//
// The points within the radius and the numpy sum of their raw weights, in point order (mos_correction.py:225-231).
template <class Dist, class Wgt>
__device__ __forceinline__ double idw_weight_sum(Dist dist, Wgt wgt, int K, double radius, int& nmask) {
  nmask = 0;
  for (int k = 0; k < K; ++k) nmask += dist(k) < radius;
  NpSum ws(nmask);
  for (int k = 0; k < K; ++k) {
    const double d = dist(k);
    if (d < radius) ws.add(wgt(k, d));
  }
  return ws.sum();
}

// acc[j] = the bias field of one row for a tile of steps, from bias(k, j): a point's own row (own >= 0) takes its
// exact bias; otherwise sum_k (w_k / wsum) bias(k, j) over the points within the radius, pairwise for a single step
// (a (n, 1) sum reduces along its only non-trivial axis) and point by point for several (numpy's axis-0 sum).
template <class Dist, class Wgt, class Bias>
__device__ __forceinline__ void idw_row_field(Dist dist, Wgt wgt, Bias bias, int K, double radius, int own, int nmask,
                                              double wsum, int steps, double (&acc)[kStepTile]) {
  if (own >= 0) {
#pragma unroll
    for (int j = 0; j < kStepTile; ++j) acc[j] = bias(own, j);
  } else if (steps == 1) {
    NpSum ps(nmask);
    for (int k = 0; k < K && nmask; ++k) {
      const double d = dist(k);
      if (d < radius) ps.add(rounded((wgt(k, d) / wsum) * bias(k, 0)));
    }
#pragma unroll
    for (int j = 0; j < kStepTile; ++j) acc[j] = 0.0;
    acc[0] = nmask ? ps.sum() : 0.0;
  } else {
#pragma unroll
    for (int j = 0; j < kStepTile; ++j) acc[j] = 0.0;
    for (int k = 0; k < K && nmask; ++k) {
      const double d = dist(k);
      if (!(d < radius)) continue;
      const double w = wgt(k, d) / wsum;
#pragma unroll
      for (int j = 0; j < kStepTile; ++j) acc[j] += rounded(w * bias(k, j));
    }
  }
}

__global__ void __launch_bounds__(kIdwThreads)
idw_apply_kernel(const void* __restrict__ in, int f64, int64_t bs, int64_t gs, int64_t ss, void* out, int64_t obs,
                 int64_t ogs, int64_t oss, int copy, int G, int steps, int C, int t2m,
                 const double* __restrict__ node_lat, const double* __restrict__ node_lon,
                 const int32_t* __restrict__ pt_idx, int K, const double* __restrict__ bias, int idw, double power,
                 double radius, int32_t* __restrict__ ncorr) {
  __shared__ double plat[kMaxPoints], plon[kMaxPoints];
  __shared__ int32_t pidx[kMaxPoints];
  __shared__ double btile[kMaxPoints * kStepTile];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int r0 = blockIdx.x * kIdwThreads, g = r0 + tid;
  for (int k = tid; k < K; k += kIdwThreads) {
    const int gi = pt_idx[k];
    pidx[k] = gi;
    plat[k] = node_lat[gi];
    plon[k] = node_lon[gi];
  }
  // the other channels of the block's rows, coalesced over (row, step, channel)
  if (copy) {
    const int nr = min(kIdwThreads, G - r0);
    const int per_row = steps * C;  // 32-bit index arithmetic: a block's rows hold < 2^31 elements
    for (int e = tid; e < nr * per_row; e += kIdwThreads) {
      const int rs = e / C, c = e - rs * C;
      if (c == t2m) continue;
      const int rr = rs / steps, s = rs - rr * steps;
      const int64_t io = b * bs + (int64_t)(r0 + rr) * gs + s * ss + c;
      const int64_t oo = b * obs + (int64_t)(r0 + rr) * ogs + s * oss + c;
      if (f64) static_cast<double*>(out)[oo] = static_cast<const double*>(in)[io];
      else static_cast<float*>(out)[oo] = static_cast<const float*>(in)[io];
    }
  }
  __syncthreads();

  const bool live = g < G;
  int own = -1;
  int nmask = 0;
  double wsum = 0.0, glat = 0.0, glon = 0.0;
  const auto dist = [&](int k) { return haversine_km(glat, glon, plat[k], plon[k]); };
  const auto wgt = [&](int, double d) { return idw_raw_weight(d, power); };
  const auto tile = [&](int k, int j) { return btile[k * kStepTile + j]; };
  if (live) {
    for (int k = 0; k < K; ++k)
      if (pidx[k] == g) { own = k; break; }
    if (own < 0 && idw) {
      glat = node_lat[g];
      glon = node_lon[g];
      wsum = idw_weight_sum(dist, wgt, K, radius, nmask);
    }
  }
  const bool touched = live && (own >= 0 || idw);
  bool any_big = false, any_nan = false;
  for (int s0 = 0; s0 < steps; s0 += kStepTile) {
    const int cnt = min(kStepTile, steps - s0);
    __syncthreads();
    for (int e = tid; e < K * kStepTile; e += kIdwThreads) {
      const int k = e / kStepTile, j = e - k * kStepTile;
      btile[e] = j < cnt ? bias[((int64_t)b * K + k) * steps + s0 + j] : 0.0;
    }
    __syncthreads();
    if (!touched) continue;
    double acc[kStepTile];
    idw_row_field(dist, wgt, tile, K, radius, own, nmask, wsum, steps, acc);
#pragma unroll
    for (int j = 0; j < kStepTile; ++j) {
      if (j >= cnt) break;
      const double f = acc[j];
      any_nan |= isnan(f);
      any_big |= fabs(f) > 1e-6;
      const int64_t io = b * bs + (int64_t)g * gs + (int64_t)(s0 + j) * ss + t2m;
      const int64_t oo = b * obs + (int64_t)g * ogs + (int64_t)(s0 + j) * oss + t2m;
      const double y = load_val(in, f64, io) + f;
      if (f64) static_cast<double*>(out)[oo] = y;
      else static_cast<float*>(out)[oo] = (float)y;
    }
  }
  if (live && !touched && copy) {
    for (int s = 0; s < steps; ++s) {
      const int64_t io = b * bs + (int64_t)g * gs + (int64_t)s * ss + t2m;
      const int64_t oo = b * obs + (int64_t)g * ogs + (int64_t)s * oss + t2m;
      if (f64) static_cast<double*>(out)[oo] = static_cast<const double*>(in)[io];
      else static_cast<float*>(out)[oo] = static_cast<const float*>(in)[io];
    }
  }
  // n_corrected: IDW counts rows whose max |bias| > 1e-6 (a NaN makes numpy's max NaN); station-only counts points
  if (ncorr && live && (idw ? (any_big && !any_nan) : own >= 0)) atomicAdd(ncorr + b, 1);
}

// ------------------------------------------------------------------------------------------------------------------
// IDW parameter sweep: the squared t2m error of P (power, radius) settings in one launch
// ------------------------------------------------------------------------------------------------------------------
// One block per 64 grid rows of one sample, one row per lane.  All four waves fill dist[k][lane], the row's distance
// to every point, once; wave 0 then walks the settings.  Per distinct power it fills wgt[k][lane] (pow and the
// division once per (row, point), not once per setting and pass), per setting it forms the field with the functions
// idw_apply_kernel uses, reading both back from LDS, and adds the lanes' squared errors in a fixed butterfly order
// into ws[p, s, block].  idw_sweep_final_kernel adds the blocks in a fixed order onto acc.  No floating-point
// atomics anywhere.
//
// A point further north or south than the largest radius is skipped without its haversine: with both latitudes in
// [-90, 90], a >= sin^2(dlat / 2), so d = 2 R asin(sqrt(a)) >= R |dlat| = 111.19 km per degree; 111 km per degree
// leaves a relative margin of 1.7e-3.  Such a point is outside every setting's radius either way.
__global__ void __launch_bounds__(kSweepThreads)
idw_sweep_kernel(const void* __restrict__ in, int f64, int64_t bs, int64_t gs, int64_t ss,
                 const void* __restrict__ truth, int64_t tbs, int64_t tgs, int64_t tss, int G, int steps, int t2m,
                 const double* __restrict__ node_lat, const double* __restrict__ node_lon,
                 const int32_t* __restrict__ pt_idx, int K, const double* __restrict__ bias, int idw,
                 const double* __restrict__ power, const double* __restrict__ radius, int P, void* fields,
                 int32_t* __restrict__ ncorr, double* __restrict__ ws) {
  extern __shared__ double sweep_lds[];
  double* dists = sweep_lds;                    // [K][kSweepRows]
  double* wgts = sweep_lds + K * kSweepRows;    // [K][kSweepRows]
  __shared__ double plat[kMaxPoints], plon[kMaxPoints];
  __shared__ int32_t pidx[kMaxPoints];
  const int tid = threadIdx.x, lane = tid % kSweepRows, q = tid / kSweepRows;
  const int b = blockIdx.y, B = gridDim.y;
  const int64_t nblk = (int64_t)gridDim.x * B, blk = (int64_t)b * gridDim.x + blockIdx.x;
  const int g = blockIdx.x * kSweepRows + lane;
  const bool live = g < G;
  for (int k = tid; k < K; k += kSweepThreads) {
    const int gi = pt_idx[k];
    pidx[k] = gi;
    plat[k] = node_lat ? node_lat[gi] : 0.0;
    plon[k] = node_lon ? node_lon[gi] : 0.0;
  }
  __syncthreads();
  double rmax = 0.0;
  for (int p = 0; p < P; ++p) rmax = fmax(rmax, radius[p]);
  if (idw) {
    const double glat = live ? node_lat[g] : 0.0, glon = live ? node_lon[g] : 0.0;
    const double inf = __builtin_inf();
    for (int k = q; k < K; k += kSweepThreads / kSweepRows) {
      const double pl = plat[k];
      const bool far = fabs(glat) <= 90.0 && fabs(pl) <= 90.0 && rounded(fabs(pl - glat) * 111.0) > rmax;
      dists[k * kSweepRows + lane] = live && !far ? haversine_km(glat, glon, pl, plon[k]) : inf;
    }
  }
  __syncthreads();
  if (q) return;

  int own = -1;
  if (live)
    for (int k = 0; k < K; ++k)
      if (pidx[k] == g) { own = k; break; }
  const bool touched = live && (own >= 0 || idw);
  const auto dist = [&](int k) { return dists[k * kSweepRows + lane]; };
  const auto wgt = [&](int k, double) { return wgts[k * kSweepRows + lane]; };
  const int64_t in0 = b * bs + (int64_t)g * gs + t2m, tr0 = b * tbs + (int64_t)g * tgs;
  double cur_power = 0.0;
  bool have_power = false;
  for (int p = 0; p < P; ++p) {
    const double pw = power[p], rad = radius[p];
    if (idw && !(have_power && pw == cur_power)) {
      for (int k = 0; k < K; ++k) {
        const double d = dists[k * kSweepRows + lane];
        wgts[k * kSweepRows + lane] = d < rmax ? idw_raw_weight(d, pw) : 0.0;
      }
      cur_power = pw;
      have_power = true;
    }
    int nmask = 0;
    double wsum = 0.0;
    if (live && own < 0 && idw) wsum = idw_weight_sum(dist, wgt, K, rad, nmask);
    // a row that no point reaches keeps x: its field is not evaluated
    const bool eval = touched && (own >= 0 || nmask > 0);
    bool any_big = false, any_nan = false;
    for (int s0 = 0; s0 < steps; s0 += kStepTile) {
      const int cnt = min(kStepTile, steps - s0);
      const double* bp = bias + (int64_t)b * K * steps + s0;
      const auto bvals = [&](int k, int j) { return j < cnt ? bp[(int64_t)k * steps + j] : 0.0; };
      double acc[kStepTile];
#pragma unroll
      for (int j = 0; j < kStepTile; ++j) acc[j] = 0.0;
      if (eval) idw_row_field(dist, wgt, bvals, K, rad, own, nmask, wsum, steps, acc);
#pragma unroll
      for (int j = 0; j < kStepTile; ++j) {
        if (j >= cnt) continue;  // uniform; no break, so that the loop unrolls around the wave sum
        const int s = s0 + j;
        double e = 0.0;
        if (live) {
          const double f = acc[j];
          any_nan |= isnan(f);
          any_big |= fabs(f) > 1e-6;
          const int64_t io = in0 + (int64_t)s * ss, to = tr0 + (int64_t)s * tss;
          const int64_t fo = (((int64_t)p * B + b) * G + g) * steps + s;
          // idw_apply_kernel's output: x + field in float64, rounded to the forecast's type; then sqerr_kernel's
          // error: difference and square in that type, each rounded on its own
          if (f64) {
            const double x = static_cast<const double*>(in)[io];
            const double y = touched ? x + f : x;
            if (fields) static_cast<double*>(fields)[fo] = y;
            const double d = y - static_cast<const double*>(truth)[to];
            e = rounded(d * d);
          } else {
            const float x = static_cast<const float*>(in)[io];
            const float y = touched ? (float)((double)x + f) : x;
            if (fields) static_cast<float*>(fields)[fo] = y;
            const float d = y - static_cast<const float*>(truth)[to];
            e = (double)rounded(d * d);
          }
        }
        const double tot = gcl::wave_sum(e);
        if (lane == 0) ws[((int64_t)p * steps + s) * nblk + blk] = tot;
      }
    }
    if (ncorr) {
      const bool counted = live && (idw ? (any_big && !any_nan) : own >= 0);
      const int n = __popcll(__ballot(counted));
      if (lane == 0 && n) atomicAdd(ncorr + (int64_t)p * B + b, n);
    }
  }
}

// acc[p, h0 + s] += the sum of the nblk block partials of (p, s): thread t adds partials t, t + 256, ... in order,
// then the 256 thread sums are added in a fixed tree.
__global__ void __launch_bounds__(kSweepFinalThreads)
idw_sweep_final_kernel(const double* __restrict__ ws, int64_t nblk, int steps, int H, int h0,
                       double* __restrict__ acc) {
  __shared__ double part[kSweepFinalThreads];
  const int ps = blockIdx.x, tid = threadIdx.x;
  const double* w = ws + (int64_t)ps * nblk;
  double s = 0.0;
  for (int64_t i = tid; i < nblk; i += kSweepFinalThreads) s += w[i];
  part[tid] = s;
  __syncthreads();
  for (int o = kSweepFinalThreads / 2; o > 0; o >>= 1) {
    if (tid < o) part[tid] += part[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const int p = ps / steps, st = ps - p * steps;
    acc[(int64_t)p * H + h0 + st] += part[0];
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Table MOS
// ------------------------------------------------------------------------------------------------------------------
__global__ void table_apply_kernel(const void* __restrict__ in, int f64, int64_t bs, int64_t gs, int64_t ss, void* out,
                                   int64_t obs, int64_t ogs, int64_t oss, int copy, int G, int steps, int C, int t2m,
                                   const double* __restrict__ tb, int nvalid, int B) {
  const int64_t per = copy ? (int64_t)steps * C : steps;
  const int64_t total = (int64_t)B * G * per;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t bg = e / per;
    const int64_t w = e - bg * per;
    const int s = copy ? (int)(w / C) : (int)w;
    const int c = copy ? (int)(w - (int64_t)s * C) : t2m;
    const int64_t b = bg / G, g = bg - b * G;
    const int64_t io = b * bs + g * gs + s * ss + c, oo = b * obs + g * ogs + s * oss + c;
    const bool add = c == t2m && s < nvalid;
    if (f64) {
      const double x = static_cast<const double*>(in)[io];
      static_cast<double*>(out)[oo] = add ? x + tb[s] : x;
    } else {
      const float x = static_cast<const float*>(in)[io];
      static_cast<float*>(out)[oo] = add ? x + (float)tb[s] : x;
    }
  }
}

}  // namespace

extern "C" int gcl_mos_forest_eval(const void* nodes, const int32_t* roots, int32_t ntrees, double baseline,
                                   const double* X, int32_t n, double* y, gcl_stream_t stream) {
  GCL_CHECK_ARG(nodes && roots && X && y, "mos_forest_eval: null argument");
  GCL_CHECK_ARG(ntrees > 0 && n >= 0, "mos_forest_eval: bad shape (ntrees=%d, n=%d)", ntrees, n);
  if (n == 0) return GCL_OK;
  hipLaunchKernelGGL(forest_eval_kernel, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream,
                     (const MosNode*)nodes, roots, ntrees, baseline, X, n, y);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_mos_forest_predict(const void* nodes, const int32_t* roots, int32_t ntrees, double baseline,
                                      const void* pred, int32_t pred_f64, int64_t bs, int64_t gs, int64_t ss,
                                      int32_t steps, int32_t c_t2m, int32_t c_u, int32_t c_v, int32_t c_sp,
                                      int32_t c_tp, const int32_t* grid_idx, const int32_t* group_start,
                                      int32_t ngroups, int32_t nst, const double* tfeat, double* bias,
                                      double* feat_out, int32_t* n_corrected, int32_t B, gcl_stream_t stream) {
  GCL_CHECK_ARG(nodes && roots && pred && grid_idx && group_start && tfeat && bias, "mos_forest_predict: null argument");
  GCL_CHECK_ARG(ntrees > 0 && steps > 0 && B > 0 && B <= 65535, "mos_forest_predict: bad shape (ntrees=%d, "
                "steps=%d, B=%d)", ntrees, steps, B);
  GCL_CHECK_ARG(ngroups > 0 && ngroups <= kMaxPoints && nst >= ngroups, "mos_forest_predict: %d groups of %d "
                "stations (at most %d groups)", ngroups, nst, kMaxPoints);
  GCL_CHECK_ARG(c_t2m >= 0, "mos_forest_predict: no t2m channel");
  // stations per pass: the leaf budget, and the pass's features and leaves next to sbias within 64 KiB of LDS (128
  // stations of 44 to 48 trees are within the budget and past 64 KiB)
  const int fit = (64 * 1024 / 8 - kMaxPoints) / (kNumFeat + ntrees);
  const int pass_max = max(1, min(kMaxPoints, min(kLeafBudget / (8 * ntrees), fit)));
  const size_t lds = ((size_t)pass_max * kNumFeat + (size_t)pass_max * ntrees + kMaxPoints) * sizeof(double);
  GCL_CHECK_ARG(lds <= 64 * 1024, "mos_forest_predict: %d trees exceed the LDS leaf table", ntrees);
  const Chans ch{c_t2m, c_u, c_v, c_sp, c_tp};
  hipLaunchKernelGGL(forest_station_kernel, dim3(ngroups, B), dim3(kForestThreads), lds, (hipStream_t)stream,
                     (const MosNode*)nodes, roots, ntrees, baseline, pred, pred_f64, bs, gs, ss, steps, ch, grid_idx,
                     group_start, nst, tfeat, bias, feat_out, n_corrected, pass_max);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_mos_idw_apply(const void* in, int32_t f64, int64_t bs, int64_t gs, int64_t ss, void* out,
                                 int64_t obs, int64_t ogs, int64_t oss, int32_t G, int32_t steps, int32_t C,
                                 int32_t t2m, const double* node_lat, const double* node_lon, const int32_t* pt_idx,
                                 int32_t K, const double* bias, int32_t idw, double power, double radius,
                                 int32_t* n_corrected, int32_t B, gcl_stream_t stream) {
  GCL_CHECK_ARG(in && out && pt_idx && bias, "mos_idw_apply: null argument");
  GCL_CHECK_ARG(!idw || (node_lat && node_lon), "mos_idw_apply: IDW needs the node coordinates");
  GCL_CHECK_ARG(G > 0 && steps > 0 && C > 0 && t2m >= 0 && t2m < C && B > 0 && B <= 65535,
                "mos_idw_apply: bad shape (G=%d, steps=%d, C=%d, t2m=%d, B=%d)", G, steps, C, t2m, B);
  GCL_CHECK_ARG(K > 0 && K <= kMaxPoints, "mos_idw_apply: %d station points (1..%d)", K, kMaxPoints);
  GCL_CHECK_ARG((int64_t)kIdwThreads * steps * C < (1ll << 31), "mos_idw_apply: steps x C = %d x %d too large",
                steps, C);
  const int copy = in != out;
  hipLaunchKernelGGL(idw_apply_kernel, dim3((G + kIdwThreads - 1) / kIdwThreads, B), dim3(kIdwThreads), 0,
                     (hipStream_t)stream, in, f64, bs, gs, ss, out, obs, ogs, oss, copy, G, steps, C, t2m, node_lat,
                     node_lon, pt_idx, K, bias, idw, power, radius, n_corrected);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

static inline int64_t sweep_blocks(int32_t G, int32_t B) { return gcl::cdiv(G, kSweepRows) * (int64_t)B; }

extern "C" size_t gcl_mos_idw_sweep_ws_bytes(int32_t G, int32_t P, int32_t steps, int32_t B) {
  if (G <= 0 || P <= 0 || steps <= 0 || B <= 0) return 0;
  return (size_t)sweep_blocks(G, B) * (size_t)P * (size_t)steps * sizeof(double);
}

extern "C" int gcl_mos_idw_sweep_max_configs(void) { return kSweepMaxConfigs; }

extern "C" int gcl_mos_idw_sweep(const void* in, int32_t f64, int64_t bs, int64_t gs, int64_t ss, const void* truth,
                                 int64_t tbs, int64_t tgs, int64_t tss, int32_t G, int32_t steps, int32_t t2m,
                                 const double* node_lat, const double* node_lon, const int32_t* pt_idx, int32_t K,
                                 const double* bias, int32_t idw, const double* power, const double* radius,
                                 int32_t P, double* acc, int32_t H, int32_t h0, void* fields_out,
                                 int32_t* n_corrected, void* ws, size_t ws_bytes, int32_t B, gcl_stream_t stream) {
  GCL_CHECK_ARG(in && truth && pt_idx && bias && power && radius && acc && ws, "mos_idw_sweep: null argument");
  GCL_CHECK_ARG(!idw || (node_lat && node_lon), "mos_idw_sweep: IDW needs the node coordinates");
  GCL_CHECK_ARG(G > 0 && steps > 0 && t2m >= 0 && B > 0 && B <= 65535,
                "mos_idw_sweep: bad shape (G=%d, steps=%d, t2m=%d, B=%d)", G, steps, t2m, B);
  GCL_CHECK_ARG(K > 0 && K <= kMaxPoints, "mos_idw_sweep: %d station points (1..%d)", K, kMaxPoints);
  GCL_CHECK_ARG(P > 0 && P <= kSweepMaxConfigs, "mos_idw_sweep: %d settings (1..%d per call)", P, kSweepMaxConfigs);
  GCL_CHECK_ARG(H > 0 && h0 >= 0 && (int64_t)h0 + steps <= H, "mos_idw_sweep: steps %d..%d outside the %d columns of "
                "acc", h0, h0 + steps - 1, H);
  GCL_CHECK_ARG((int64_t)P * steps < (1ll << 31), "mos_idw_sweep: P x steps = %d x %d too large", P, steps);
  GCL_CHECK_ARG(ws_bytes >= gcl_mos_idw_sweep_ws_bytes(G, P, steps, B), "mos_idw_sweep: workspace of %zu bytes, %zu "
                "needed", ws_bytes, gcl_mos_idw_sweep_ws_bytes(G, P, steps, B));
  const size_t lds = idw ? 2 * (size_t)K * kSweepRows * sizeof(double) : 0;
  if (lds > 64 * 1024) GCL_ENSURE_DYN_LDS(idw_sweep_kernel, lds);
  hipLaunchKernelGGL(idw_sweep_kernel, dim3((unsigned)gcl::cdiv(G, kSweepRows), B), dim3(kSweepThreads), lds,
                     (hipStream_t)stream, in, f64, bs, gs, ss, truth, tbs, tgs, tss, G, steps, t2m, node_lat, node_lon,
                     pt_idx, K, bias, idw, power, radius, P, fields_out, n_corrected, (double*)ws);
  GCL_CHECK_LAUNCH();
  hipLaunchKernelGGL(idw_sweep_final_kernel, dim3(P * steps), dim3(kSweepFinalThreads), 0, (hipStream_t)stream,
                     (const double*)ws, sweep_blocks(G, B), steps, H, h0, acc);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_mos_table_apply(const void* in, int32_t f64, int64_t bs, int64_t gs, int64_t ss, void* out,
                                   int64_t obs, int64_t ogs, int64_t oss, int32_t G, int32_t steps, int32_t C,
                                   int32_t t2m, const double* step_bias, int32_t nvalid, int32_t B,
                                   gcl_stream_t stream) {
  GCL_CHECK_ARG(in && out && (step_bias || nvalid == 0), "mos_table_apply: null argument");
  GCL_CHECK_ARG(G >= 0 && steps > 0 && C > 0 && t2m >= 0 && t2m < C && B > 0 && nvalid >= 0 && nvalid <= steps,
                "mos_table_apply: bad shape (G=%d, steps=%d, C=%d, t2m=%d, nvalid=%d)", G, steps, C, t2m, nvalid);
  const int copy = in != out;
  const int64_t total = (int64_t)B * G * (copy ? (int64_t)steps * C : steps);
  if (total == 0) return GCL_OK;
  const int64_t nb = (total + 255) / 256;
  hipLaunchKernelGGL(table_apply_kernel, dim3((unsigned)(nb > 8192 ? 8192 : nb)), dim3(256), 0, (hipStream_t)stream,
                     in, f64, bs, gs, ss, out, obs, ogs, oss, copy, G, steps, C, t2m, step_bias, nvalid, B);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}
