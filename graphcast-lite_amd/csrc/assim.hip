// Data assimilation (src/assimilation/): the nudging blend and a matrix-free optimal interpolation (OI).
//
// OI.  Every observation maps to one OI node J_k (its nearest node), so H only selects nodes and the analysis
//   S = sb2 K(J, J) + diag I,   W = S^-1 (y - x_b[J]),   x_a[i] = x_b[i] + sum_k sb2 K(i, J_k) W[k]
// (K(p, q) = exp(-(R theta_pq / L)^2), theta the haversine angle) never needs B.  S depends only on the station set,
// so it is factored once per set: a root-free Cholesky (S = U^T D U, U unit upper) that also eliminates the identity,
// leaving X = U^-T in the lower triangle, so that the solves S^-1 r = X^T D^-1 X r are two triangular products that
// run in parallel over rows instead of sequential substitutions.  Factor and solves are float64; the analysis, the
// hot kernel, evaluates the kernel in float32 from float64 coordinate differences and accumulates in float32.
#include "common.h"

#include <initializer_list>

namespace {

constexpr int kMaxStations = 16384;  // one float64 m x m factor: 2 GiB at the limit

// ---------------------------------------------------------------------------------------------------------------
// Nudging.  Both of the reference's formulas, evaluated exactly as torch CPU does in float32: one rounding per
// operation, never contracted into an FMA: every product passes through gcl::rounded (common.h), so the add sees an
// opaque, already rounded value.
// ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void nudge_kernel(const float* __restrict__ f, int64_t ldf, int64_t bsf,
                                                   const float* __restrict__ o, int64_t ldo, int64_t bso,
                                                   const uint8_t* __restrict__ mask, float c0, float c1, int form,
                                                   float* out, int64_t ldt, int64_t bst, int32_t B, int32_t G,
                                                   int32_t C) {
  const int64_t total = (int64_t)B * G * C;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
    const int c = (int)(t % C);
    const int64_t r = t / C;
    const int g = (int)(r % G);
    const int64_t b = r / G;
    const float fv = f[b * bsf + (int64_t)g * ldf + c];
    const float ov = o[b * bso + (int64_t)g * ldo + c];
    float v = fv;
    if (!__builtin_isnan(ov) && (!mask || mask[c])) {
      if (form == 0)
        v = fv + gcl::rounded(c1 * (ov - fv));  // f + alpha (o - f)               (nudging.py:91-92)
      else
        v = gcl::rounded(c0 * fv) + gcl::rounded(c1 * ov);  // (1 - alpha) f + alpha o  (nudging.py:205)
    }
    out[b * bst + (int64_t)g * ldt + c] = v;
  }
}

// The sequential form with one setting per batch row: row b is nudged with alpha[b] at the stations of network
// net_of_row[b] (station_mask [n_net][G]; net < 0: the row is not nudged).  Observations are read only at stations, so
// the truth can be passed as it is (bso = 0 broadcasts it); in place (out == f) only nudged values are touched.
__global__ __launch_bounds__(256) void nudge_rows_kernel(const float* f, int64_t ldf, int64_t bsf,
                                                        const float* __restrict__ o, int64_t ldo, int64_t bso,
                                                        const uint8_t* __restrict__ station_mask,
                                                        const int32_t* __restrict__ net_of_row,
                                                        const float* __restrict__ alpha,
                                                        const uint8_t* __restrict__ mask, float* out, int64_t ldt,
                                                        int64_t bst, int32_t B, int32_t G, int32_t C) {
  const int64_t total = (int64_t)B * G * C;
  const int64_t stride = (int64_t)gridDim.x * 256;
  const bool in_place = out == f;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += stride) {
    const int c = (int)(t % C);
    const int64_t r = t / C;
    const int g = (int)(r % G);
    const int64_t b = r / G;
    const int net = net_of_row[b];
    const bool at_station = net >= 0 && station_mask[(int64_t)net * G + g] && (!mask || mask[c]);
    if (!at_station && in_place) continue;
    const float fv = f[b * bsf + (int64_t)g * ldf + c];
    float v = fv;
    if (at_station) {
      const float ov = o[b * bso + (int64_t)g * ldo + c];
      if (!__builtin_isnan(ov)) v = fv + gcl::rounded(alpha[b] * (ov - fv));  // nudge_kernel, form 0
    }
    out[b * bst + (int64_t)g * ldt + c] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// OI: station covariance, factor, solves.
// ---------------------------------------------------------------------------------------------------------------
// Haversine angle between two points (radians), float64: 2 asin(sqrt(a)) as in optimal_interpolation.py:49-56.
__device__ __forceinline__ double hav_angle(double la1, double lo1, double la2, double lo2) {
  const double s1 = sin(0.5 * (la1 - la2)), s2 = sin(0.5 * (lo1 - lo2));
  double a = s1 * s1 + cos(la1) * cos(la2) * (s2 * s2);
  a = a < 1.0 ? a : 1.0;
  return 2.0 * asin(sqrt(a));
}

// S[a, b] = sb2 exp(-rl2 theta_ab^2) + (a == b) diag, row-major m x m.
__global__ __launch_bounds__(256) void oi_cov_kernel(const double* __restrict__ lat, const double* __restrict__ lon,
                                                     int32_t m, double sb2, double rl2, double diag,
                                                     double* __restrict__ S) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  const int a = blockIdx.y;
  if (b >= m) return;
  const double th = hav_angle(lat[a], lon[a], lat[b], lon[b]);
  S[(int64_t)a * m + b] = sb2 * exp(-rl2 * th * th) + (a == b ? diag : 0.0);
}

// One pivot j of the root-free elimination, in place on M (m x m, row-major).  Invariant before step j:
//   upper triangle rows >= j hold the partially reduced S (row j is final: pivot row), the diagonal M[j][j] = d_j;
//   strict lower rows hold X = U^-T, built row by row (row j is final).
// For every row i > j, with l = M[j][i] / d_j (= U[j][i]):
//   M[i][k] -= l M[j][k]   k >= i  (trailing update of S; only the upper triangle is kept)
//   M[i][c] -= l M[j][c]   c <  j  (X row update), and M[i][j] = -l (X[j][j] = 1).
// Row j is only read and rows i > j only written, so one launch per pivot needs no other synchronisation; both
// halves read the pivot row and write row i contiguously.
__global__ __launch_bounds__(256) void oi_ldl_step_kernel(double* __restrict__ M, int32_t m, int32_t j) {
  const int i = j + 1 + blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int nx = j + 1;           // columns [0, j]: X part
  const int ns = m - i;           // columns [i, m): S part
  if (t >= nx + ns) return;
  const int64_t rj = (int64_t)j * m, ri = (int64_t)i * m;
  const double l = M[rj + i] / M[rj + j];
  if (t < nx) {
    M[ri + t] = (t == j) ? -l : M[ri + t] - l * M[rj + t];
  } else {
    const int k = i + (t - nx);
    M[ri + k] -= l * M[rj + k];
  }
}

// Mirror the strict lower triangle into the strict upper one (X^T next to X), 32 x 32 tiles through LDS.
__global__ __launch_bounds__(256) void oi_mirror_kernel(double* __restrict__ M, int32_t m) {
  __shared__ double tile[32][33];
  const int bi = blockIdx.y, bc = blockIdx.x;  // tile rows [32 bi, ...), cols [32 bc, ...)
  if (bc > bi) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 8 rows per pass
  for (int r = ty; r < 32; r += 8) {
    const int i = bi * 32 + r, c = bc * 32 + tx;
    tile[r][tx] = (i < m && c < m) ? M[(int64_t)i * m + c] : 0.0;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int c = bc * 32 + r, i = bi * 32 + tx;  // write M[c][i] = M[i][c] for c < i
    if (i < m && c < i) M[(int64_t)c * m + i] = tile[tx][r];
  }
}

// Triangular product over the factor, one wave per row i, kRhs right-hand sides per block column:
//   FWD: out[q][i] = (in[q][i] + sum_{c < i} X[i][c] in[q][c]) / d_i        (z = D^-1 X r)
//   BWD: out[q][i] =  in[q][i] + sum_{k > i} X[k][i] in[q][k]                (W = X^T z; X^T is the upper triangle)
// in / out are [n][m] (station index contiguous).  Each column's sum has a fixed order (lane-strided partial sums,
// then a fixed butterfly), independent of n and of the other columns.
constexpr int kRhs = 8;

template <bool FWD, typename TO>
__global__ __launch_bounds__(256) void oi_tri_kernel(const double* __restrict__ M, int32_t m,
                                                     const double* __restrict__ in, TO* __restrict__ out, int32_t n) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int q0 = blockIdx.y * kRhs;
  if (i >= m) return;
  const int nq = n - q0 < kRhs ? n - q0 : kRhs;
  const int64_t ri = (int64_t)i * m;
  const int c_lo = FWD ? 0 : i + 1, c_hi = FWD ? i : m;
  double acc[kRhs];
#pragma unroll
  for (int q = 0; q < kRhs; ++q) acc[q] = 0.0;
  for (int c = c_lo + lane; c < c_hi; c += 64) {
    const double x = M[ri + c];
#pragma unroll
    for (int q = 0; q < kRhs; ++q)
      if (q < nq) acc[q] = fma(x, in[(int64_t)(q0 + q) * m + c], acc[q]);
  }
#pragma unroll
  for (int q = 0; q < kRhs; ++q) acc[q] = gcl::wave_sum(acc[q]);
  if (lane < nq) {
    double v = 0.0;
#pragma unroll
    for (int q = 0; q < kRhs; ++q)
      if (q == lane) v = acc[q];
    v += in[(int64_t)(q0 + lane) * m + i];
    if (FWD) v /= M[ri + i];
    out[(int64_t)(q0 + lane) * m + i] = (TO)v;
  }
}

// rhs[b * nch + q][k] = obs[b, obs_row[k], chans[q]] - x_b[b, node_row[k], chans[q]]  (float64, exact)
__global__ __launch_bounds__(256) void oi_innov_kernel(const float* __restrict__ obs, int64_t ldo, int64_t bso,
                                                       const float* __restrict__ xb, int64_t ldx, int64_t bsx,
                                                       const int32_t* __restrict__ obs_row,
                                                       const int32_t* __restrict__ node_row,
                                                       const int32_t* __restrict__ chans, int32_t m, int32_t nch,
                                                       int32_t B, double* __restrict__ rhs) {
  const int64_t total = (int64_t)B * nch * m;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int k = (int)(t % m);
    const int64_t col = t / m;
    const int q = (int)(col % nch);
    const int64_t b = col / nch;
    const int c = chans[q];
    rhs[t] = (double)obs[b * bso + (int64_t)obs_row[k] * ldo + c] - (double)xb[b * bsx + (int64_t)node_row[k] * ldx + c];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// OI analysis (the hot kernel).  One thread per OI node, stations staged through LDS in tiles of kTile, NCH columns of
// W (sample-major: b * nch + q) per block column.  Per (node, station) pair: two float64 coordinate differences
// (no cancellation: the sine arguments are exact to float32), then in float32
//   a = sin^2(dlat/2) + cos(lat_i) cos(lat_k) sin^2(dlon/2),  theta = 2 asin(sqrt(a)),  w = sb2 exp(-rl2 theta^2).
// Pairs with |dlat| > theta_cut or a > a_cut have exp(-rl2 theta^2) < exp(-120), i.e. w == 0 in float32, and skip the
// transcendentals; a wave whose lanes all have w == 0 skips the NCH FMAs (adding 0 * W leaves the sum unchanged).
// ---------------------------------------------------------------------------------------------------------------
constexpr int kTile = 128;

// The pair geometry of both analysis kernels: the haversine angle theta of node (la, lo, ci = cos la) and station
// (sla, slo, sc), false when the pair is beyond the cut (theta is then not computed).
__device__ __forceinline__ bool oi_pair_theta(double la, double lo, float ci, double sla, double slo, float sc,
                                              float th_cut, float a_cut, float& th) {
  const float dlat = (float)(la - sla);
  if (!(fabsf(dlat) <= th_cut)) return false;
  const float dlon = (float)(lo - slo);
  const float s1 = sinf(0.5f * dlat), s2 = sinf(0.5f * dlon);
  const float a = s1 * s1 + (ci * sc) * (s2 * s2);
  if (!(a <= a_cut)) return false;
  th = 2.f * asinf(sqrtf(fminf(a, 1.f)));
  return true;
}

template <int NCH>
__global__ __launch_bounds__(256) void oi_analysis_kernel(
    const float* xb, int64_t ldx, int64_t bsx, float* xa, int64_t lda, int64_t bsa, const int32_t* __restrict__ chans,
    int32_t nch, const int32_t* __restrict__ node_row, const double* __restrict__ nlat,
    const double* __restrict__ nlon, const float* __restrict__ ncos, int32_t n_nodes, const double* __restrict__ slat,
    const double* __restrict__ slon, const float* __restrict__ scos, const float* __restrict__ W, int32_t m,
    int32_t ncol, float sb2, float rl2, float th_cut, float a_cut) {
  __shared__ double s_lat[kTile], s_lon[kTile];
  __shared__ float s_cos[kTile];
  __shared__ float s_w[kTile][NCH];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int col0 = blockIdx.y * NCH;
  const int ncl = ncol - col0 < NCH ? ncol - col0 : NCH;
  const bool live = i < n_nodes;
  const double la = live ? nlat[i] : 0.0, lo = live ? nlon[i] : 0.0;
  const float ci = live ? ncos[i] : 0.f;
  float acc[NCH];
#pragma unroll
  for (int q = 0; q < NCH; ++q) acc[q] = 0.f;
  for (int k0 = 0; k0 < m; k0 += kTile) {
    const int nk = m - k0 < kTile ? m - k0 : kTile;
    __syncthreads();
    for (int t = threadIdx.x; t < kTile; t += 256) {
      const bool ok = t < nk;
      s_lat[t] = ok ? slat[k0 + t] : 0.0;
      s_lon[t] = ok ? slon[k0 + t] : 0.0;
      s_cos[t] = ok ? scos[k0 + t] : 0.f;
    }
    for (int t = threadIdx.x; t < kTile * NCH; t += 256) {
      const int q = t / kTile, k = t % kTile;  // consecutive threads: consecutive stations of one W row
      s_w[k][q] = (q < ncl && k < nk) ? W[(int64_t)(col0 + q) * m + k0 + k] : 0.f;
    }
    __syncthreads();
    for (int k = 0; k < nk; ++k) {
      float w = 0.f, th;
      if (live && oi_pair_theta(la, lo, ci, s_lat[k], s_lon[k], s_cos[k], th_cut, a_cut, th))
        w = sb2 * expf(-rl2 * (th * th));
      if (__any(w != 0.f)) {
#pragma unroll
        for (int q = 0; q < NCH; ++q) acc[q] = fmaf(w, s_w[k][q], acc[q]);
      }
    }
  }
  if (!live) return;
  const int64_t g = node_row ? node_row[i] : i;
  for (int q = 0; q < ncl; ++q) {
    const int col = col0 + q;
    const int c = chans[col % nch];
    const int64_t b = col / nch;
    const float v = xb[b * bsx + g * ldx + c];
    xa[b * bsa + g * lda + c] = v + acc[q];
  }
}

template <int NCH>
int launch_analysis(hipStream_t st, int nblk, int ncol, const float* xb, int64_t ldx, int64_t bsx, float* xa,
                    int64_t lda, int64_t bsa, const int32_t* chans, int32_t nch, const int32_t* node_row,
                    const double* nlat, const double* nlon, const float* ncos, int32_t n_nodes, const double* slat,
                    const double* slon, const float* scos, const float* W, int32_t m, float sb2, float rl2,
                    float th_cut, float a_cut) {
  hipLaunchKernelGGL(oi_analysis_kernel<NCH>, dim3(nblk, (unsigned)gcl::cdiv(ncol, NCH)), dim3(256), 0, st, xb, ldx,
                     bsx, xa, lda, bsa, chans, nch, node_row, nlat, nlon, ncos, n_nodes, slat, slon, scos, W, m, ncol,
                     sb2, rl2, th_cut, a_cut);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

// The analysis with one (sb2, rl2) per sample.  A block column is NS consecutive samples x CC of their nch
// channels (the same channel chunk of every sample), so which accumulator belongs to which sample is known at compile
// time.  The pair geometry is computed once for the NS * CC columns; expf once per run of equal rl2 among the NS
// samples (the caller orders the samples so that equal rl2 are adjacent), w = sb2 e once per sample.  (th_cut, a_cut)
// are those of the longest correlation length: inside them a sample of a shorter one gets e == 0 from the underflow
// of expf itself, and a wave whose lanes all have e == 0 for a sample skips that sample's CC FMAs.  The settings of
// the NS samples are block-uniform (scalar registers, scalar branches).
template <int NS, int CC>
__global__ __launch_bounds__(256) void oi_analysis_rows_kernel(
    const float* xb, int64_t ldx, int64_t bsx, float* xa, int64_t lda, int64_t bsa, const int32_t* __restrict__ chans,
    int32_t nch, const int32_t* __restrict__ node_row, const double* __restrict__ nlat,
    const double* __restrict__ nlon, const float* __restrict__ ncos, int32_t n_nodes, const double* __restrict__ slat,
    const double* __restrict__ slon, const float* __restrict__ scos, const float* __restrict__ W, int32_t m,
    int32_t B, int32_t nchunk, const float* __restrict__ sb2_row, const float* __restrict__ rl2_row, float th_cut,
    float a_cut) {
  constexpr int NCOL = NS * CC;
  __shared__ double s_lat[kTile], s_lon[kTile];
  __shared__ float s_cos[kTile];
  __shared__ float s_w[kTile][NCOL];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int b0 = (blockIdx.y / nchunk) * NS;   // first sample
  const int c0 = (blockIdx.y % nchunk) * CC;   // first channel (position in chans)
  const int nb = B - b0 < NS ? B - b0 : NS;
  const int nc = nch - c0 < CC ? nch - c0 : CC;
  const bool live = i < n_nodes;
  const double la = live ? nlat[i] : 0.0, lo = live ? nlon[i] : 0.0;
  const float ci = live ? ncos[i] : 0.f;
  float sb2[NS], rl2[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const int b = b0 + (s < nb ? s : nb - 1);  // padding samples repeat the last one (their W is 0)
    sb2[s] = sb2_row[b];
    rl2[s] = rl2_row[b];
  }
  float acc[NS][CC];
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int c = 0; c < CC; ++c) acc[s][c] = 0.f;
  for (int k0 = 0; k0 < m; k0 += kTile) {
    const int nk = m - k0 < kTile ? m - k0 : kTile;
    __syncthreads();
    for (int t = threadIdx.x; t < kTile; t += 256) {
      const bool ok = t < nk;
      s_lat[t] = ok ? slat[k0 + t] : 0.0;
      s_lon[t] = ok ? slon[k0 + t] : 0.0;
      s_cos[t] = ok ? scos[k0 + t] : 0.f;
    }
    for (int t = threadIdx.x; t < kTile * NCOL; t += 256) {
      const int q = t / kTile, k = t % kTile;  // consecutive threads: consecutive stations of one W row
      const int s = q / CC, c = q % CC;
      s_w[k][q] = (s < nb && c < nc && k < nk) ? W[((int64_t)(b0 + s) * nch + c0 + c) * m + k0 + k] : 0.f;
    }
    __syncthreads();
    for (int k = 0; k < nk; ++k) {
      float th = 0.f;
      const bool near = live && oi_pair_theta(la, lo, ci, s_lat[k], s_lon[k], s_cos[k], th_cut, a_cut, th);
      if (!__any(near)) continue;
      const float th2 = th * th;
      float e = 0.f;
      bool any_e = false;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        if (s == 0 || rl2[s] != rl2[s - 1]) {
          e = near ? expf(-rl2[s] * th2) : 0.f;
          any_e = __any(e != 0.f);
        }
        if (any_e) {
          const float w = sb2[s] * e;
#pragma unroll
          for (int c = 0; c < CC; ++c) acc[s][c] = fmaf(w, s_w[k][s * CC + c], acc[s][c]);
        }
      }
    }
  }
  if (!live) return;
  const int64_t g = node_row ? node_row[i] : i;
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int c = 0; c < CC; ++c)
      if (s < nb && c < nc) {
        const int ch = chans[c0 + c];
        const int64_t b = b0 + s;
        const float v = xb[b * bsx + g * ldx + ch];
        xa[b * bsa + g * lda + ch] = v + acc[s][c];
      }
}

template <int NS, int CC>
int launch_analysis_rows(hipStream_t st, int nblk, const float* xb, int64_t ldx, int64_t bsx, float* xa, int64_t lda,
                         int64_t bsa, const int32_t* chans, int32_t nch, const int32_t* node_row, const double* nlat,
                         const double* nlon, const float* ncos, int32_t n_nodes, const double* slat,
                         const double* slon, const float* scos, const float* W, int32_t m, int32_t B,
                         const float* sb2_row, const float* rl2_row, float th_cut, float a_cut) {
  const int nchunk = (int)gcl::cdiv(nch, CC);
  hipLaunchKernelGGL((oi_analysis_rows_kernel<NS, CC>), dim3(nblk, (unsigned)(gcl::cdiv(B, NS) * nchunk)), dim3(256),
                     0, st, xb, ldx, bsx, xa, lda, bsa, chans, nch, node_row, nlat, nlon, ncos, n_nodes, slat, slon,
                     scos, W, m, B, nchunk, sb2_row, rl2_row, th_cut, a_cut);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

}  // namespace

extern "C" int gcl_oi_max_stations(void) { return kMaxStations; }

extern "C" int gcl_nudge(const float* f, int64_t ldf, int64_t bsf, const float* o, int64_t ldo, int64_t bso,
                         const uint8_t* chan_mask, float c0, float c1, int32_t form, float* out, int64_t ldt,
                         int64_t bst, int32_t B, int32_t G, int32_t C, gcl_stream_t stream) {
  GCL_CHECK_ARG(f && o && out, "nudge: null argument");
  GCL_CHECK_ARG(form == 0 || form == 1, "nudge: form must be 0 (sequential) or 1 (offline), got %d", form);
  GCL_CHECK_ARG(B > 0 && G >= 0 && C > 0 && ldf >= C && ldo >= C && ldt >= C, "nudge: bad shape");
  const int64_t total = (int64_t)B * G * C;
  if (total == 0) return GCL_OK;
  hipLaunchKernelGGL(nudge_kernel, dim3(gcl::grid_for(total, 4096)), dim3(256), 0, (hipStream_t)stream, f, ldf, bsf, o, ldo, bso,
                     chan_mask, c0, c1, form, out, ldt, bst, B, G, C);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_nudge_rows(const float* f, int64_t ldf, int64_t bsf, const float* o, int64_t ldo, int64_t bso,
                              const uint8_t* station_mask, int32_t n_net, const int32_t* net_of_row,
                              const float* alpha, const uint8_t* chan_mask, float* out, int64_t ldt, int64_t bst,
                              int32_t B, int32_t G, int32_t C, gcl_stream_t stream) {
  GCL_CHECK_ARG(f && o && out && station_mask && net_of_row && alpha, "nudge_rows: null argument");
  GCL_CHECK_ARG(B > 0 && G >= 0 && C > 0 && n_net > 0 && ldf >= C && ldo >= C && ldt >= C, "nudge_rows: bad shape");
  const int64_t total = (int64_t)B * G * C;
  if (total == 0) return GCL_OK;
  hipLaunchKernelGGL(nudge_rows_kernel, dim3(gcl::grid_for(total, 4096)), dim3(256), 0, (hipStream_t)stream, f, ldf,
                     bsf, o, ldo, bso, station_mask, net_of_row, alpha, chan_mask, out, ldt, bst, B, G, C);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_oi_station_cov(const double* lat, const double* lon, int32_t m, double sb2, double rl2,
                                  double diag, double* S, gcl_stream_t stream) {
  GCL_CHECK_ARG(lat && lon && S, "oi_station_cov: null argument");
  GCL_CHECK_ARG(m > 0 && m <= kMaxStations, "oi_station_cov: m=%d outside [1, %d]", m, kMaxStations);
  hipLaunchKernelGGL(oi_cov_kernel, dim3((unsigned)gcl::cdiv(m, 256), m), dim3(256), 0, (hipStream_t)stream, lat, lon,
                     m, sb2, rl2, diag, S);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_oi_factor(double* M, int32_t m, gcl_stream_t stream) {
  GCL_CHECK_ARG(M, "oi_factor: null argument");
  GCL_CHECK_ARG(m > 0 && m <= kMaxStations, "oi_factor: m=%d outside [1, %d]", m, kMaxStations);
  const hipStream_t st = (hipStream_t)stream;
  for (int j = 0; j + 1 < m; ++j) {
    const int rows = m - 1 - j;
    // row i has j + 1 X columns and m - i S columns: the widest (i = j + 1) has m
    hipLaunchKernelGGL(oi_ldl_step_kernel, dim3((unsigned)gcl::cdiv(m, 256), rows), dim3(256), 0, st, M, m, j);
    GCL_CHECK_LAUNCH();
  }
  const unsigned nt = (unsigned)gcl::cdiv(m, 32);
  hipLaunchKernelGGL(oi_mirror_kernel, dim3(nt, nt), dim3(256), 0, st, M, m);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_oi_solve(const double* M, int32_t m, const double* rhs, double* tmp, float* W, int32_t n,
                            gcl_stream_t stream) {
  GCL_CHECK_ARG(M && rhs && tmp && W, "oi_solve: null argument");
  GCL_CHECK_ARG(m > 0 && m <= kMaxStations && n > 0, "oi_solve: bad shape (m=%d, n=%d)", m, n);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)gcl::cdiv(m, 4), (unsigned)gcl::cdiv(n, kRhs));
  hipLaunchKernelGGL((oi_tri_kernel<true, double>), grid, dim3(256), 0, st, M, m, rhs, tmp, n);
  GCL_CHECK_LAUNCH();
  hipLaunchKernelGGL((oi_tri_kernel<false, float>), grid, dim3(256), 0, st, M, m, (const double*)tmp, W, n);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_oi_innovation(const float* obs, int64_t ldo, int64_t bso, const float* xb, int64_t ldx,
                                 int64_t bsx, const int32_t* obs_row, const int32_t* node_row, const int32_t* chans,
                                 int32_t m, int32_t nch, int32_t B, double* rhs, gcl_stream_t stream) {
  GCL_CHECK_ARG(obs && xb && obs_row && node_row && chans && rhs, "oi_innovation: null argument");
  GCL_CHECK_ARG(m > 0 && nch > 0 && B > 0, "oi_innovation: bad shape");
  const int64_t total = (int64_t)B * nch * m;
  hipLaunchKernelGGL(oi_innov_kernel, dim3(gcl::grid_for(total, 4096)), dim3(256), 0, (hipStream_t)stream, obs, ldo, bso, xb, ldx,
                     bsx, obs_row, node_row, chans, m, nch, B, rhs);
  GCL_CHECK_LAUNCH();
  return GCL_OK;
}

extern "C" int gcl_oi_analysis(const float* xb, int64_t ldx, int64_t bsx, float* xa, int64_t lda, int64_t bsa,
                               const int32_t* chans, int32_t nch, const int32_t* node_row, const double* nlat,
                               const double* nlon, const float* ncos, int32_t n_nodes, const double* slat,
                               const double* slon, const float* scos, const float* W, int32_t m, float sb2, float rl2,
                               float th_cut, float a_cut, int32_t B, gcl_stream_t stream) {
  GCL_CHECK_ARG(xb && xa && chans && nlat && nlon && ncos && slat && slon && scos && W, "oi_analysis: null argument");
  GCL_CHECK_ARG(n_nodes >= 0 && m > 0 && nch > 0 && B > 0, "oi_analysis: bad shape");
  if (n_nodes == 0) return GCL_OK;
  const hipStream_t st = (hipStream_t)stream;
  const int nblk = (int)gcl::cdiv(n_nodes, 256);
  const int ncol = B * nch;
  if (ncol <= 8)
    return launch_analysis<8>(st, nblk, ncol, xb, ldx, bsx, xa, lda, bsa, chans, nch, node_row, nlat, nlon, ncos,
                              n_nodes, slat, slon, scos, W, m, sb2, rl2, th_cut, a_cut);
  if (ncol <= 16)
    return launch_analysis<16>(st, nblk, ncol, xb, ldx, bsx, xa, lda, bsa, chans, nch, node_row, nlat, nlon, ncos,
                               n_nodes, slat, slon, scos, W, m, sb2, rl2, th_cut, a_cut);
  if (ncol <= 24)
    return launch_analysis<24>(st, nblk, ncol, xb, ldx, bsx, xa, lda, bsa, chans, nch, node_row, nlat, nlon, ncos,
                               n_nodes, slat, slon, scos, W, m, sb2, rl2, th_cut, a_cut);
  return launch_analysis<32>(st, nblk, ncol, xb, ldx, bsx, xa, lda, bsa, chans, nch, node_row, nlat, nlon, ncos,
                             n_nodes, slat, slon, scos, W, m, sb2, rl2, th_cut, a_cut);
}

extern "C" int gcl_oi_analysis_rows(const float* xb, int64_t ldx, int64_t bsx, float* xa, int64_t lda, int64_t bsa,
                                    const int32_t* chans, int32_t nch, const int32_t* node_row, const double* nlat,
                                    const double* nlon, const float* ncos, int32_t n_nodes, const double* slat,
                                    const double* slon, const float* scos, const float* W, int32_t m,
                                    const float* sb2_row, const float* rl2_row, float th_cut, float a_cut, int32_t B,
                                    gcl_stream_t stream) {
  GCL_CHECK_ARG(xb && xa && chans && nlat && nlon && ncos && slat && slon && scos && W && sb2_row && rl2_row,
                "oi_analysis_rows: null argument");
  GCL_CHECK_ARG(n_nodes >= 0 && m > 0 && nch > 0 && B > 0, "oi_analysis_rows: bad shape");
  if (n_nodes == 0) return GCL_OK;
  const hipStream_t st = (hipStream_t)stream;
  const int nblk = (int)gcl::cdiv(n_nodes, 256);
  // samples per block (ascending widths): the fewest sample groups, i.e. evaluations of the pair geometry, then the
  // narrowest block; a padding sample costs FMAs on zeros only
  const auto pick = [B](std::initializer_list<int> widths) {
    int best = 0;
    int64_t best_groups = 0;
    for (int ns : widths) {
      const int64_t groups = gcl::cdiv(B, ns);
      if (best == 0 || groups < best_groups) best = ns, best_groups = groups;
    }
    return best;
  };
#define GCL_ROWS(NS, CC)                                                                                             \
  return launch_analysis_rows<NS, CC>(st, nblk, xb, ldx, bsx, xa, lda, bsa, chans, nch, node_row, nlat, nlon, ncos, \
                                      n_nodes, slat, slon, scos, W, m, B, sb2_row, rl2_row, th_cut, a_cut)
  if (nch <= 4) {
    switch (pick({2, 4, 8})) {
      case 2: GCL_ROWS(2, 4);
      case 4: GCL_ROWS(4, 4);
      default: GCL_ROWS(8, 4);
    }
  }
  switch (pick({1, 2, 4, 6})) {
    case 1: GCL_ROWS(1, 8);
    case 2: GCL_ROWS(2, 8);
    case 4: GCL_ROWS(4, 8);
    default: GCL_ROWS(6, 8);
  }
#undef GCL_ROWS
}
