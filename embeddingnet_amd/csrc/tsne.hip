// Exact t-SNE (van der Maaten & Hinton) in two dimensions: scikit-learn's TSNE(method='exact', n_components=2) arithmetic on
// the device.  Stands in for `TSNE().fit_transform(encodings)` of the reference's utils.py plot_tsne / plot_tsne_interactive.
//
//   affinities  D2[n,n] squared distances (embnet_pairwise_dist_f32(squared = 1)) -> P[n,n], beta[n]
//     per row i a bisection on beta so that H_i = -sum_j p_j|i log p_j|i = log(perplexity), p_j|i ~ exp(-beta D2_ij), j != i:
//     beta = 1, <= 100 steps, stop at |H - log perplexity| <= 1e-5, double / halve while the bracket is open, a zero row sum
//     becomes 1e-8 (sklearn/manifold/_utils.pyx _binary_search_perplexity).  The row minimum of D2 is subtracted before exp (it
//     cancels in p and H; without it a large beta leaves an all-zero row).  One wave per row: rows of <= 4096 columns sit in
//     LDS for the 100 steps, longer ones are streamed (from L2).  exp in fp32, the sums and H in f64.
//     P = (Pc + Pc^T) / S, S = sum of Pc + Pc^T (two stages: per row in its wave, rows in index order by one workgroup), then
//     max(P, 2.220446e-16) off the diagonal, diagonal 0.  (i,j) and (j,i) are formed by one thread from the same two
//     operands: symmetric bit for bit.  P may alias D2.
//   iteration   w_ij = 1/(1 + |y_i - y_j|^2), Z = sum_{i != j} w_ij, g_i = 4 sum_j (a P_ij - w_ij/Z) w_ij (y_i - y_j)
//     launch A (tsne_rows_kernel): a workgroup per block of rows streams P (16 B per lane) against Y tiles in LDS and writes
//       per row sum_j P w (y_i - y_j), sum_j w^2 (y_i - y_j), sum_j w: fp32 per lane, f64 across the wave.
//     launch B (tsne_update_kernel, a component per thread): Z from the n row sums in a fixed order (f64; every workgroup adds
//       them itself, in the same order, so there is no flag and no second launch), g, then scikit-learn's
//       _gradient_descent update with the sign test done on signs (an fp32 product of two small factors underflows to 0):
//       inc = (u < 0 && g > 0) || (u > 0 && g < 0); gains += 0.2 where inc, *= 0.8 elsewhere, floor 0.01;
//       u = momentum u - lr gains g; Y += u.
//   kl          launch A, Z, a second sweep for sum_ij P log(max(P,eps) / max(w/Z,eps)) (f64 accumulation), and a one-workgroup
//     finish that writes the KL, the 2-norm of the gradient and optionally the gradient.
// No atomics at all, every reduction has a fixed order: bitwise reproducible.  No host synchronisation, no allocation.
#include "common.h"
#include "../../include/embnet.h"

namespace embnet {

constexpr int TS_MAX_N = 32768;
constexpr int TS_ROW_LDS = 4096;                         // affinities: floats of one row per wave in LDS (4 waves: 64 KiB)
constexpr int TS_TILE = 1024;                            // launch A: points of Y per LDS tile (8 KiB)
constexpr int TS_ONE = 1024;                             // threads of the one-workgroup kernels
constexpr float TS_EPS = 2.220446e-16f;                  // scikit-learn's MACHINE_EPSILON (float64 epsilon)

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// Sum over the TS_ONE threads of one workgroup in a fixed order (lane tree, then waves in index order); every thread gets it.
__device__ double ts_block_sum(double v) {
  __shared__ double part[TS_ONE / 64];
  v = wave_sum(v);
  __syncthreads();                                       // a previous call's readers are done with part[]
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < TS_ONE / 64; ++w) t += part[w];
  return t;
}

// ---- affinities ----------------------------------------------------------------------------------------------------------
// grid ceil(n / 4) x 256 threads, one wave per row.  Writes Pc (row i of p, the conditional probabilities), beta[i] and the
// f64 sum of the stored row.
template <bool IN_LDS>
__global__ __launch_bounds__(256) void tsne_beta_kernel(const float* d2, int n, float log_perp, float* p, float* beta_out,
                                                        double* rowsum) {
  __shared__ float lrow[IN_LDS ? 4 : 1][IN_LDS ? TS_ROW_LDS : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wave;
  if (i >= n) return;                                    // wave-uniform; no workgroup barrier below
  const float* row = d2 + (long)i * n;
  if (IN_LDS) {
    for (int j = lane; j < n; j += 64) lrow[wave][j] = row[j];
    row = lrow[wave];
  }
  float m = INFINITY;
  for (int j = lane; j < n; j += 64)
    if (j != i) m = fminf(m, row[j]);
  m = wave_min(m);
  float beta = 1.f, beta_min = -INFINITY, beta_max = INFINITY;
  float beta_used = beta;                                // like scikit-learn, the row keeps the last beta that was EVALUATED
  double sum = 1.0;
  for (int step = 0; step < 100; ++step) {
    beta_used = beta;
    double s = 0.0, sd = 0.0;
    for (int j = lane; j < n; j += 64) {
      if (j == i) continue;
      const float dm = row[j] - m;
      const float e = expf(-beta * dm);
      s += (double)e;
      sd += (double)dm * (double)e;
    }
    s = wave_sum(s);                                     // xor butterfly: every lane holds the same bits
    sd = wave_sum(sd);
    if (s == 0.0) s = 1e-8;
    sum = s;
    const double h = log(s) + (double)beta * sd / s;
    const double diff = h - (double)log_perp;
    if (fabs(diff) <= 1e-5) break;
    if (diff > 0.0) {
      beta_min = beta;
      beta = beta_max == INFINITY ? beta * 2.f : (beta + beta_max) * 0.5f;
    } else {
      beta_max = beta;
      beta = beta_min == -INFINITY ? beta * 0.5f : (beta + beta_min) * 0.5f;
    }
  }
  const float inv = (float)(1.0 / sum);
  float* out = p + (long)i * n;
  double rs = 0.0;
  for (int j = lane; j < n; j += 64) {
    const float v = j == i ? 0.f : expf(-beta_used * (row[j] - m)) * inv;
    out[j] = v;
    rs += (double)v;
  }
  rs = wave_sum(rs);
  if (lane == 0) { beta_out[i] = beta_used; rowsum[i] = rs; }
}

// one workgroup: *total = 2 * sum_i rowsum[i] (the sum of Pc + Pc^T), rows in a fixed order
__global__ __launch_bounds__(TS_ONE) void tsne_psum_kernel(const double* rowsum, int n, double* total) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += TS_ONE) s += rowsum[i];
  s = ts_block_sum(s);
  if (threadIdx.x == 0) *total = fmax(2.0 * s, (double)TS_EPS);
}

// grid (T, T), T = ceil(n / 32), 256 threads; the workgroups with bj < bi leave at once, (bi, bj) owns tiles (bi,bj) and (bj,bi)
__device__ __forceinline__ float ts_joint(float a, float b, double total, bool diag) {
  return diag ? 0.f : fmaxf((float)(((double)a + (double)b) / total), TS_EPS);
}
__global__ __launch_bounds__(256) void tsne_symmetrize_kernel(float* p, int n, const double* total) {
  __shared__ float ta[32][33];
  __shared__ float tb[32][33];
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bj < bi) return;
  const int i0 = bi * 32, j0 = bj * 32;
  for (int t = threadIdx.x; t < 1024; t += 256) {
    const int r = t >> 5, c = t & 31;
    ta[r][c] = (i0 + r < n && j0 + c < n) ? p[(long)(i0 + r) * n + j0 + c] : 0.f;
    tb[r][c] = (j0 + r < n && i0 + c < n) ? p[(long)(j0 + r) * n + i0 + c] : 0.f;
  }
  __syncthreads();
  const double s = *total;
  for (int t = threadIdx.x; t < 1024; t += 256) {
    const int r = t >> 5, c = t & 31;
    if (i0 + r < n && j0 + c < n) p[(long)(i0 + r) * n + j0 + c] = ts_joint(ta[r][c], tb[c][r], s, i0 + r == j0 + c);
    if (bi != bj && j0 + r < n && i0 + c < n) p[(long)(j0 + r) * n + i0 + c] = ts_joint(tb[r][c], ta[c][r], s, false);
  }
}

// ---- launch A ------------------------------------------------------------------------------------------------------------
// grid ceil(n / (4 R)) x 256 threads; wave w of workgroup b owns rows (4 b + w) R .. + R - 1.  VEC: n % 4 == 0 and P 16-byte
// aligned, a lane loads 4 consecutive columns; otherwise columns lane + 64 q.
// KL = false: rows[i][0..4] = sum_j P w dx, sum_j P w dy, sum_j w^2 dx, sum_j w^2 dy, sum_{j != i} w   (dx = y_i0 - y_j0)
// KL = true (R = 1): klrow[i] = sum_{j != i} P log(max(P, eps) / max(w / Z, eps)), Z = *zsum
template <int R, bool VEC, bool KL>
__global__ __launch_bounds__(256) void tsne_rows_kernel(const float* __restrict__ p, const float* __restrict__ y, int n,
                                                        double* __restrict__ rows, const double* __restrict__ zsum) {
  __shared__ __attribute__((aligned(16))) float2 ys[TS_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = (blockIdx.x * 4 + wave) * R;
  float yix[R], yiy[R], ax[R], ay[R], rx[R], ry[R], sw[R];
  double kl[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = i0 + r;
    yix[r] = i < n ? y[2 * i] : 0.f;
    yiy[r] = i < n ? y[2 * i + 1] : 0.f;
    ax[r] = ay[r] = rx[r] = ry[r] = sw[r] = 0.f;
    kl[r] = 0.0;
  }
  const float inv_z = KL ? (float)(1.0 / *zsum) : 0.f;
  for (int t0 = 0; t0 < n; t0 += TS_TILE) {
    __syncthreads();
    for (int c = tid; c < TS_TILE; c += 256) {
      const int j = t0 + c;
      ys[c] = j < n ? reinterpret_cast<const float2*>(y)[j] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    for (int s0 = 0; s0 < TS_TILE && t0 + s0 < n; s0 += 256) {
      float pv[R][4];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int i = i0 + r;
        if (VEC) {
          const int j = t0 + s0 + 4 * lane;
          float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
          if (i < n && j < n) v = *reinterpret_cast<const float4*>(p + (long)i * n + j);
          pv[r][0] = v.x; pv[r][1] = v.y; pv[r][2] = v.z; pv[r][3] = v.w;
        } else {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int j = t0 + s0 + lane + 64 * q;
            pv[r][q] = (i < n && j < n) ? p[(long)i * n + j] : 0.f;
          }
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = VEC ? s0 + 4 * lane + q : s0 + lane + 64 * q;
        const int j = t0 + c;
        const float2 yj = ys[c];
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float dx = yix[r] - yj.x, dy = yiy[r] - yj.y;
          const float d = fmaf(dx, dx, dy * dy);
          float w = __builtin_amdgcn_rcpf(1.f + d);
          w = (j < n && j != i0 + r) ? w : 0.f;
          if (KL) {
            const float pj = pv[r][q];
            if (w > 0.f) kl[r] += (double)(pj * logf(fmaxf(pj, TS_EPS) / fmaxf(w * inv_z, TS_EPS)));
          } else {
            const float wdx = w * dx, wdy = w * dy;        // not (w * w) * dx: w^2 leaves the normal range at |y| ~ 1e10
            ax[r] = fmaf(pv[r][q], wdx, ax[r]);
            ay[r] = fmaf(pv[r][q], wdy, ay[r]);
            rx[r] = fmaf(w, wdx, rx[r]);
            ry[r] = fmaf(w, wdy, ry[r]);
            sw[r] += w;
          }
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = i0 + r;
    if (KL) {
      const double k = wave_sum(kl[r]);
      if (lane == 0 && i < n) rows[i] = k;
    } else {
      const double a0 = wave_sum((double)ax[r]), a1 = wave_sum((double)ay[r]);
      const double r0 = wave_sum((double)rx[r]), r1 = wave_sum((double)ry[r]);
      const double s = wave_sum((double)sw[r]);
      if (lane == 0 && i < n) {
        double* o = rows + (long)i * 5;
        o[0] = a0; o[1] = a1; o[2] = r0; o[3] = r1; o[4] = s;
      }
    }
  }
}

__device__ __forceinline__ double ts_zsum(const double* rows, int n) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += TS_ONE) s += rows[(long)i * 5 + 4];
  return ts_block_sum(s);
}

// ---- launch B: ceil(2n / 1024) workgroups ----------------------------------------------------------------------------------
// Every workgroup adds the n row sums of w itself, in the same fixed order (so all hold the same bits of Z; n f64 from L2),
// then updates one component per thread.
__global__ __launch_bounds__(TS_ONE) void tsne_update_kernel(const double* __restrict__ rows, int n, float* __restrict__ y,
                                                             float* __restrict__ update, float* __restrict__ gains,
                                                             float alpha, float momentum, float lr) {
  const double z = ts_zsum(rows, n);
  const int t = blockIdx.x * TS_ONE + threadIdx.x;
  if (t >= 2 * n) return;
  const double* o = rows + (long)(t >> 1) * 5 + (t & 1);
  const float g = (float)(4.0 * ((double)alpha * o[0] - o[2] / z));
  const float u = update[t];
  const bool inc = (u < 0.f && g > 0.f) || (u > 0.f && g < 0.f);
  const float gain = fmaxf(inc ? gains[t] + 0.2f : gains[t] * 0.8f, 0.01f);
  const float un = momentum * u - lr * (gain * g);
  gains[t] = gain;
  update[t] = un;
  y[t] += un;
}

__global__ __launch_bounds__(TS_ONE) void tsne_zsum_kernel(const double* rows, int n, double* zsum) {
  const double z = ts_zsum(rows, n);
  if (threadIdx.x == 0) *zsum = z;
}

__global__ __launch_bounds__(TS_ONE) void tsne_kl_finish_kernel(const double* __restrict__ rows, const double* __restrict__ klrow,
                                                                int n, const double* __restrict__ zsum, float* kl,
                                                                float* grad_norm, float* grad) {
  const double z = *zsum;
  double g2 = 0.0, k = 0.0;
  for (int t = threadIdx.x; t < 2 * n; t += TS_ONE) {
    const double* o = rows + (long)(t >> 1) * 5 + (t & 1);
    const double g = 4.0 * (o[0] - o[2] / z);
    if (grad) grad[t] = (float)g;
    g2 += g * g;
  }
  for (int i = threadIdx.x; i < n; i += TS_ONE) k += klrow[i];
  g2 = ts_block_sum(g2);
  k = ts_block_sum(k);
  if (threadIdx.x == 0) { *kl = (float)k; *grad_norm = (float)sqrt(g2); }
}

static size_t ts_align64(size_t b) { return (b + 63) / 64 * 64; }

// workspace: [64 B: f64 Z, f64 S][n x 5 f64 row sums][n f64 per-row KL / row sums of Pc]
struct TsneWs { double* zsum; double* psum; double* rows; double* klrow; };
static TsneWs ts_carve(void* ws, int n) {
  char* b = (char*)ws;
  return {(double*)b, (double*)b + 1, (double*)(b + 64), (double*)(b + 64 + ts_align64((size_t)n * 40))};
}

static bool ts_vec_ok(const float* p, int n) { return n % 4 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// launch A for the gradient sums: 4 rows per wave once there are enough rows to fill the chip with them
static void ts_launch_rows(const float* p, const float* y, int n, double* rows, hipStream_t s) {
  EMBNET_TRACE("embnet::tsne_rows_kernel", TRACE_BYTES, 4.0 * n * n + 56.0 * n, s);
  const bool vec = ts_vec_ok(p, n);
  if (n >= 4096) {
    if (vec) tsne_rows_kernel<4, true, false><<<cdiv(n, 16), 256, 0, s>>>(p, y, n, rows, nullptr);
    else tsne_rows_kernel<4, false, false><<<cdiv(n, 16), 256, 0, s>>>(p, y, n, rows, nullptr);
  } else {
    if (vec) tsne_rows_kernel<1, true, false><<<cdiv(n, 4), 256, 0, s>>>(p, y, n, rows, nullptr);
    else tsne_rows_kernel<1, false, false><<<cdiv(n, 4), 256, 0, s>>>(p, y, n, rows, nullptr);
  }
}

}  // namespace embnet

using namespace embnet;

extern "C" size_t embnet_tsne_workspace_bytes(int n) {
  if (n < 2 || n > TS_MAX_N) return 0;
  return 64 + ts_align64((size_t)n * 40) + ts_align64((size_t)n * 8);
}

#define TS_CHECK_WS(what, ws, ws_bytes, n)                                                                              \
  do {                                                                                                                  \
    EMBNET_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 15) == 0, what ": workspace must be 16-byte aligned");          \
    if ((ws_bytes) < embnet_tsne_workspace_bytes(n))                                                                    \
      return fail(EMBNET_EWORKSPACE, what ": workspace %zu < %zu bytes", (size_t)(ws_bytes), embnet_tsne_workspace_bytes(n)); \
  } while (0)

extern "C" int embnet_tsne_affinities(const float* d2, int n, float perplexity, float* p, float* beta, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  EMBNET_CHECK_ARG(d2 && p && beta && workspace, "tsne_affinities: null pointer");
  EMBNET_CHECK_ARG(n >= 2 && n <= TS_MAX_N, "tsne_affinities: n=%d outside [2, %d]", n, TS_MAX_N);
  EMBNET_CHECK_ARG(perplexity >= 1.f && perplexity < (float)n, "tsne_affinities: perplexity=%g outside [1, n=%d)",
                   (double)perplexity, n);
  TS_CHECK_WS("tsne_affinities", workspace, workspace_bytes, n);
  const TsneWs w = ts_carve(workspace, n);
  hipStream_t s = (hipStream_t)stream;
  const float log_perp = (float)log((double)perplexity);
  {
    EMBNET_TRACE("embnet::tsne_beta_kernel", TRACE_BYTES, 8.0 * n * n, stream);
    if (n <= TS_ROW_LDS) tsne_beta_kernel<true><<<cdiv(n, 4), 256, 0, s>>>(d2, n, log_perp, p, beta, w.klrow);
    else tsne_beta_kernel<false><<<cdiv(n, 4), 256, 0, s>>>(d2, n, log_perp, p, beta, w.klrow);
  }
  {
    EMBNET_TRACE("embnet::tsne_psum_kernel", TRACE_BYTES, 8.0 * n, stream);
    tsne_psum_kernel<<<1, TS_ONE, 0, s>>>(w.klrow, n, w.psum);
  }
  {
    EMBNET_TRACE("embnet::tsne_symmetrize_kernel", TRACE_BYTES, 8.0 * n * n, stream);
    const int t = cdiv(n, 32);
    tsne_symmetrize_kernel<<<dim3(t, t), 256, 0, s>>>(p, n, w.psum);
  }
  return check_launch("tsne_affinities");
}

extern "C" int embnet_tsne_iterate(const float* p, int n, float* y, float* update, float* gains, float exaggeration,
                                   float momentum, float lr, int n_iter, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  EMBNET_CHECK_ARG(p && y && update && gains && workspace, "tsne_iterate: null pointer");
  EMBNET_CHECK_ARG(n >= 2 && n <= TS_MAX_N, "tsne_iterate: n=%d outside [2, %d]", n, TS_MAX_N);
  EMBNET_CHECK_ARG(n_iter >= 0, "tsne_iterate: n_iter=%d < 0", n_iter);
  TS_CHECK_WS("tsne_iterate", workspace, workspace_bytes, n);
  const TsneWs w = ts_carve(workspace, n);
  hipStream_t s = (hipStream_t)stream;
  for (int it = 0; it < n_iter; ++it) {
    ts_launch_rows(p, y, n, w.rows, s);
    EMBNET_TRACE("embnet::tsne_update_kernel", TRACE_BYTES, 64.0 * n, stream);   // + 8 n of row sums per workgroup, from L2
    tsne_update_kernel<<<cdiv(2L * n, TS_ONE), TS_ONE, 0, s>>>(w.rows, n, y, update, gains, exaggeration, momentum, lr);
  }
  return check_launch("tsne_iterate");
}

extern "C" int embnet_tsne_kl(const float* p, int n, const float* y, float* kl, float* grad_norm, float* grad,
                              void* workspace, size_t workspace_bytes, void* stream) {
  EMBNET_CHECK_ARG(p && y && kl && grad_norm && workspace, "tsne_kl: null pointer");
  EMBNET_CHECK_ARG(n >= 2 && n <= TS_MAX_N, "tsne_kl: n=%d outside [2, %d]", n, TS_MAX_N);
  TS_CHECK_WS("tsne_kl", workspace, workspace_bytes, n);
  const TsneWs w = ts_carve(workspace, n);
  hipStream_t s = (hipStream_t)stream;
  ts_launch_rows(p, y, n, w.rows, s);
  {
    EMBNET_TRACE("embnet::tsne_zsum_kernel", TRACE_BYTES, 8.0 * n, stream);
    tsne_zsum_kernel<<<1, TS_ONE, 0, s>>>(w.rows, n, w.zsum);
  }
  {
    EMBNET_TRACE("embnet::tsne_kl_rows_kernel", TRACE_BYTES, 4.0 * n * n + 16.0 * n, stream);
    if (ts_vec_ok(p, n)) tsne_rows_kernel<1, true, true><<<cdiv(n, 4), 256, 0, s>>>(p, y, n, w.klrow, w.zsum);
    else tsne_rows_kernel<1, false, true><<<cdiv(n, 4), 256, 0, s>>>(p, y, n, w.klrow, w.zsum);
  }
  {
    EMBNET_TRACE("embnet::tsne_kl_finish_kernel", TRACE_BYTES, 56.0 * n, stream);
    tsne_kl_finish_kernel<<<1, TS_ONE, 0, s>>>(w.rows, w.klrow, n, w.zsum, kl, grad_norm, grad);
  }
  return check_launch("tsne_kl");
}
