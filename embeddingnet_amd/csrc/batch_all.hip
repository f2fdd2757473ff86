// Batch-all triplet loss (Moindrot; Hermans et al. name it next to batch-hard): every valid triplet of a class-contiguous
// P x K batch takes part, the loss is the mean over the triplets that violate the margin.  Build-defined: the reference
// cites both batch strategies (README [2], [4]) and implements neither.
//
//   X [N, E] fp32, N = P*K, rows c*K .. c*K+K-1 are class c.  d(i,j) = sum_c (x_ic - x_jc)^2 (the squared-L2 quantity of
//   triplet_gather_fwd).  Valid (a,p,n): p in a's class, p != a, n in another class; T = N (K-1) (N-K) of them.
//   b = (d(a,p) - d(a,n)) + margin; a triplet is ACTIVE iff b > 0 (strict: the selection rules' `active` flags use b >= 0).
//   A = #active;  loss = sum_active b / max(A, 1);  frac_active = A / T.
//   W[a,p] = #{n : (a,p,n) active},  W[a,n] = -#{p : (a,p,n) active},  0 elsewhere (small integers, exact in fp32).
//   backward, A held constant:  demb_i = (2 g / max(A,1)) * sum_j M_ij (x_i - x_j),  M = W + W^T
//                                      = (2 g / max(A,1)) * (s_i x_i - (M X)_i),   s_i = sum_j M_ij.
//
// Forward, per-class path (N <= 512, K <= 16, K (E + N) floats in 64 KiB of LDS: C1, C2, C5 and the shipped configs), ONE
// launch: a workgroup per class holds its K rows and their K x N distance rows (difference form) in LDS, one wave per anchor
// sweeps (K-1) positives x (N-K) negatives and writes the anchor's row of W (rows belong to their anchor: no atomics), the
// workgroup writes a per-class partial (f64 sum of b, count), and the last workgroup to arrive (agent-scope ticket, the
// hand-off of fused_loss.hip) reduces the partials in class order.
// Forward, distance-matrix path (everything else up to N = 4096, E = 4096): the per-class block would re-read all N rows per
// class (N^2 E / K bytes from L2), so the squared distances come from embnet_pairwise_dist_f32(squared = 1) into the
// workspace (the Gram form: its rounding differs from the difference form) and a sweep kernel takes one anchor row per wave,
// with the same partial / ticket / fixed-order reduction over anchors.
// Backward, one launch: Y = M X on the f64 matrix instructions (v_mfma_f64_16x16x4_f64) with the epilogue
// demb = (2g/A)(s x - Y).  Not the f32 ones: an f32 chain over j rounds relative to sum_j |M_ij| |x_j|, while the gradient is
// a sum of differences (x_i - x_j) whose size can be far below that (same-class rows are close); M is integer and x fp32, so
// every f64 product is exact and the result carries one fp32 rounding relative to sum_j |M_ij| |x_i - x_j|.
// Nothing is atomic in floating point, every reduction has a fixed order: bitwise reproducible.  No host synchronisation, no
// allocation: capturable in a graph.
#include "common.h"
#include "../../include/embnet.h"

namespace embnet {

constexpr int BA_MAX_N = 4096;
constexpr int BA_MAX_E = 4096;
constexpr int BA_CLASS_MAX_N = 512;
constexpr int BA_CLASS_MAX_K = 16;
constexpr int BA_LDS_FLOATS = 16 * 1024;                 // 64 KiB: K*(E + N) floats
constexpr int BA_CLASS_THREADS = 1024;                   // 16 waves: one per anchor, and the distance phase's L2 round trips
constexpr int BA_SWEEP_THREADS = 256;                    // 4 anchors per workgroup, a 16 KiB distance row each

__device__ __forceinline__ float ba_b(float dap, float dan, float margin) {   // one rounding order everywhere
  return __fadd_rn(__fsub_rn(dap, dan), margin);
}

// One wave, one anchor (local index ai of class [lo, lo+k)), its squared-distance row drow[n] (LDS).  Writes the anchor's
// row of W and returns the wave's f64 sum of active b (fixed order) and its active count.
__device__ void ba_sweep_anchor(const float* drow, int n, int k, int lo, int ai, float margin, float* wrow, int lane,
                                double& sum_out, int& cnt_out) {
  double s = 0.0;
  int c = 0;
  for (int col = lane; col < n; col += 64) {             // negatives: W[a,n] = -#{p : active}
    if (col >= lo && col < lo + k) continue;
    const float dan = drow[col];
    int cn = 0;
    for (int j = 0; j < k; ++j) {
      if (j == ai) continue;
      const float b = ba_b(drow[lo + j], dan, margin);
      if (b > 0.f) { ++cn; s += (double)b; }
    }
    wrow[col] = -(float)cn;
    c += cn;
  }
  for (int j = 0; j < k; ++j) {                          // positives: W[a,p] = #{n : active}; W[a,a] = 0
    int cp = 0;
    if (j != ai) {
      const float dap = drow[lo + j];
      for (int col = lane; col < n; col += 64)
        if ((col < lo || col >= lo + k) && ba_b(dap, drow[col], margin) > 0.f) ++cp;
    }
    cp = wave_sum(cp);
    if (lane == 0) wrow[lo + j] = (float)cp;
  }
  sum_out = wave_sum(s);
  cnt_out = wave_sum(c);                                 // <= (K-1)(N-K) < 2^23
}

struct BatchAllParams {
  const float* emb; int n, p, k, e; float margin;
  float* w; int32_t* n_active; float* frac; float* mean;
  int* ticket; double* part_sum; long long* part_cnt;    // workspace: arrival counter (zero between launches), partials
  const float* dist;                                     // distance-matrix path: squared distances [n][n]
  long long t_total;
};

// Arrival ticket (fused_loss.hip's hand-off): every storing wave drains, barrier, one lane releases at agent scope and takes
// the ticket; the last arriver acquires, re-arms the counter and reduces the `slots` partials in index order.
template <int THREADS>
__device__ void ba_finish(const BatchAllParams& q, int slots) {
  __shared__ int s_last;
  __shared__ double ws_sum[THREADS / 64];
  __shared__ long long ws_cnt[THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int t = atomicAdd(q.ticket, 1);
    s_last = t == (int)gridDim.x - 1;
    if (s_last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      *q.ticket = 0;                                     // re-arm the counter for the next launch
    }
  }
  __syncthreads();
  if (!s_last) return;
  double s = 0.0;
  long long c = 0;
  for (int i = tid; i < slots; i += THREADS) {
    s += __hip_atomic_load(&q.part_sum[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    c += __hip_atomic_load(&q.part_cnt[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  s = wave_sum(s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if (lane == 0) { ws_sum[wave] = s; ws_cnt[wave] = c; }
  __syncthreads();
  if (tid == 0) {
    double ts = 0.0;
    long long tc = 0;
    for (int w = 0; w < THREADS / 64; ++w) { ts += ws_sum[w]; tc += ws_cnt[w]; }
    *q.n_active = (int32_t)tc;
    *q.frac = (float)((double)tc / (double)q.t_total);
    *q.mean = (float)(ts / (double)(tc > 0 ? tc : 1));
  }
}

// ---- forward, per-class path: grid = P workgroups ----------------------------------------------------------------------
__global__ __launch_bounds__(BA_CLASS_THREADS) void batch_all_class_fwd_kernel(BatchAllParams q) {
  __shared__ __attribute__((aligned(16))) float lds[BA_LDS_FLOATS];
  __shared__ double wsum[BA_CLASS_MAX_K];
  __shared__ int wcnt[BA_CLASS_MAX_K];
  const int n = q.n, k = q.k, e = q.e, c = blockIdx.x, lo = c * k;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = BA_CLASS_THREADS / 64;
  float* A = lds;                                        // [k][e] the class's rows
  float* D = lds + k * e;                                // [k][n] squared distances anchor -> row, difference form
  for (int i = tid; i < k * e; i += BA_CLASS_THREADS) A[i] = q.emb[(long)lo * e + i];
  __syncthreads();
  // row r of the block against the K anchors: the row is read once, eight loads in flight per lane (fused_loss.hip's loop)
  for (int r = wave; r < n; r += NW) {
    const float* y = q.emb + (long)r * e;
    float acc[BA_CLASS_MAX_K];
#pragma unroll
    for (int a = 0; a < BA_CLASS_MAX_K; ++a) acc[a] = 0.f;
    for (int c0 = 0; c0 < e; c0 += 512) {
      float yv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { const int cc = c0 + lane + 64 * j; yv[j] = cc < e ? y[cc] : 0.f; }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int cc = c0 + lane + 64 * j;
        if (cc < e) {
#pragma unroll
          for (int a = 0; a < BA_CLASS_MAX_K; ++a)
            if (a < k) { const float d = A[a * e + cc] - yv[j]; acc[a] = fmaf(d, d, acc[a]); }
        }
      }
    }
#pragma unroll
    for (int a = 0; a < BA_CLASS_MAX_K; ++a) {
      if (a < k) {
        const float g = wave_sum(acc[a]);
        if (lane == 0) D[a * n + r] = g;
      }
    }
  }
  __syncthreads();
  if (wave < k) {
    double s; int cnt;
    ba_sweep_anchor(D + wave * n, n, k, lo, wave, q.margin, q.w + (long)(lo + wave) * n, lane, s, cnt);
    if (lane == 0) { wsum[wave] = s; wcnt[wave] = cnt; }
  }
  __syncthreads();
  if (tid == 0) {                                        // the class's partial, anchors in order
    double s = 0.0;
    long long cnt = 0;
    for (int a = 0; a < k; ++a) { s += wsum[a]; cnt += wcnt[a]; }
    q.part_sum[c] = s;
    q.part_cnt[c] = cnt;
  }
  ba_finish<BA_CLASS_THREADS>(q, q.p);
}

// ---- forward, distance-matrix path: grid = ceil(N / 4), one anchor per wave ----------------------------------------------
__global__ __launch_bounds__(BA_SWEEP_THREADS) void batch_all_sweep_kernel(BatchAllParams q) {
  __shared__ __attribute__((aligned(16))) float rows[BA_SWEEP_THREADS / 64][BA_MAX_N];
  const int n = q.n, k = q.k, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int a = blockIdx.x * (BA_SWEEP_THREADS / 64) + wave;
  float* drow = rows[wave];
  if (a < n) {                                           // wave-uniform
    const float* src = q.dist + (long)a * n;
    for (int col = lane; col < n; col += 64) drow[col] = src[col];
  }
  __syncthreads();
  if (a < n) {
    const int lo = (a / k) * k;
    double s; int cnt;
    ba_sweep_anchor(drow, n, k, lo, a - lo, q.margin, q.w + (long)a * n, lane, s, cnt);
    if (lane == 0) { q.part_sum[a] = s; q.part_cnt[a] = cnt; }
  }
  ba_finish<BA_SWEEP_THREADS>(q, n);
}

// ---- backward: demb = (2g / max(A,1)) (s x - M X), M = W + W^T ----------------------------------------------------------
// grid (ceil(N/32), ceil(E/32)), 4 waves, each a 16 x 16 tile of the 32 x 32 block; j in chunks of 32 through LDS.
// v_mfma_f64_16x16x4_f64: A[i = l&15][k = l>>4], B[k = l>>4][col = l&15], D[row = (l>>4) + 4r][col = l&15] (the f64 map).
using f64x4 = __attribute__((ext_vector_type(4))) double;

__global__ __launch_bounds__(256) void batch_all_bwd_kernel(const float* __restrict__ emb, int n, int e,
                                                           const float* __restrict__ w, const int32_t* __restrict__ n_active,
                                                           const float* __restrict__ upstream, float* __restrict__ demb) {
  __shared__ float wa[32][33];                           // W[i0 + ii][j0 + jj]
  __shared__ float wb[32][33];                           // W[j0 + jj][i0 + ii], stored [jj][ii]
  __shared__ float xs[32][33];                           // X[j0 + jj][e0 + ee]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = blockIdx.x * 32, e0 = blockIdx.y * 32;
  const int ro = 16 * (wave >> 1), co = 16 * (wave & 1);
  const int lr = lane & 15, lk = lane >> 4;
  f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  double srow = 0.0;                                     // sum of this lane's M[ro + lr][k] operands
  for (int j0 = 0; j0 < n; j0 += 32) {
    for (int t = tid; t < 1024; t += 256) {
      const int r = t >> 5, cc = t & 31;
      const int i = i0 + r, j = j0 + cc, jr = j0 + r, ic = i0 + cc, ec = e0 + cc;
      wa[r][cc] = (i < n && j < n) ? w[(long)i * n + j] : 0.f;
      wb[r][cc] = (jr < n && ic < n) ? w[(long)jr * n + ic] : 0.f;
      xs[r][cc] = (jr < n && ec < e) ? emb[(long)jr * e + ec] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const int kx = 4 * kk + lk;
      const double av = (double)wa[ro + lr][kx] + (double)wb[kx][ro + lr];
      const double bv = (double)xs[kx][co + lr];
      srow += av;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
    __syncthreads();
  }
  srow += __shfl_xor(srow, 16, 64);                      // the four k-lanes of row lr: s_i, exact (integers)
  srow += __shfl_xor(srow, 32, 64);
  const int cnt = *n_active;
  const double g = upstream ? (double)*upstream : 1.0;
  const double scale = 2.0 * g / (double)(cnt > 0 ? cnt : 1);
  const int col = e0 + co + lr;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int rl = lk + 4 * r;
    const double s = __shfl(srow, rl, 64);               // lane rl holds s of row rl
    const int row = i0 + ro + rl;
    if (row < n && col < e) {
      const double x = (double)emb[(long)row * e + col];
      demb[(long)row * e + col] = (float)(scale * (s * x - acc[r]));
    }
  }
}

static bool ba_class_path_fits(int p, int k, int e) {
  const long n = (long)p * k;
  return k <= BA_CLASS_MAX_K && n <= BA_CLASS_MAX_N && (long)k * (e + n) <= BA_LDS_FLOATS;
}

static size_t ba_align16(size_t b) { return (b + 15) / 16 * 16; }

static bool ba_range_ok(int p, int k, int e) {
  if (p < 2 || k < 2 || e < 1 || e > BA_MAX_E) return false;
  const long long n = (long long)p * k;
  return n <= BA_MAX_N && n * (k - 1) * (n - k) <= 0x7fffffffLL;
}

}  // namespace embnet

using namespace embnet;

// workspace: [16 B ticket][n f64 partial sums][n int64 partial counts][n*n f32 distances][pairwise workspace]
// (sized for both forward paths, so a caller may force either)
extern "C" size_t embnet_batch_all_workspace_bytes(int p, int k, int e) {
  if (!ba_range_ok(p, k, e)) return 0;
  const int n = p * k;
  return 16 + ba_align16((size_t)n * 8) * 2 + ba_align16((size_t)n * n * 4) + ba_align16(embnet_pairwise_workspace_bytes(n, e));
}

extern "C" int embnet_batch_all_path(int p, int k, int e) {
  if (!ba_range_ok(p, k, e)) return 0;
  return ba_class_path_fits(p, k, e) ? EMBNET_BATCH_ALL_PER_CLASS : EMBNET_BATCH_ALL_DISTANCE_MATRIX;
}

extern "C" int embnet_batch_all_loss_fwd(const float* emb, int p, int k, int e, float margin, int path, float* pair_w,
                                         int32_t* n_active, float* frac_active, float* mean_loss, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  EMBNET_CHECK_ARG(emb && pair_w && n_active && frac_active && mean_loss && workspace, "batch_all_loss_fwd: null pointer");
  EMBNET_CHECK_ARG(p >= 2 && k >= 2, "batch_all_loss_fwd: need p >= 2 classes and k >= 2 samples (p=%d k=%d)", p, k);
  EMBNET_CHECK_ARG((long long)p * k <= BA_MAX_N, "batch_all_loss_fwd: n = p*k = %lld > %d", (long long)p * k, BA_MAX_N);
  EMBNET_CHECK_ARG(e >= 1 && e <= BA_MAX_E, "batch_all_loss_fwd: e=%d outside [1, %d]", e, BA_MAX_E);
  EMBNET_CHECK_ARG(ba_range_ok(p, k, e), "batch_all_loss_fwd: p=%d k=%d has more than 2^31-1 triplets", p, k);
  EMBNET_CHECK_ARG(path >= 0 && path <= EMBNET_BATCH_ALL_DISTANCE_MATRIX, "batch_all_loss_fwd: unknown path %d", path);
  EMBNET_CHECK_ARG(path != EMBNET_BATCH_ALL_PER_CLASS || ba_class_path_fits(p, k, e),
                   "batch_all_loss_fwd: p=%d k=%d e=%d does not fit the per-class path", p, k, e);
  EMBNET_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "batch_all_loss_fwd: workspace must be 16-byte aligned");
  if (workspace_bytes < embnet_batch_all_workspace_bytes(p, k, e))
    return fail(EMBNET_EWORKSPACE, "batch_all_loss_fwd: workspace %zu < %zu bytes", workspace_bytes,
                embnet_batch_all_workspace_bytes(p, k, e));
  const int n = p * k;
  if (path == 0) path = embnet_batch_all_path(p, k, e);
  char* ws = (char*)workspace;
  double* part_sum = (double*)(ws + 16);
  long long* part_cnt = (long long*)(ws + 16 + ba_align16((size_t)n * 8));
  float* dist = (float*)(ws + 16 + 2 * ba_align16((size_t)n * 8));
  char* pw = (char*)dist + ba_align16((size_t)n * n * 4);
  BatchAllParams q{emb, n, p, k, e, margin, pair_w, n_active, frac_active, mean_loss, (int*)ws, part_sum, part_cnt, dist,
                   (long long)n * (k - 1) * (n - k)};
  hipStream_t s = (hipStream_t)stream;
  if (path == EMBNET_BATCH_ALL_PER_CLASS) {
    EMBNET_TRACE("embnet::batch_all_class_fwd_kernel", TRACE_BYTES, 4.0 * n * e * (p + 1.0) + 4.0 * n * n, stream);
    batch_all_class_fwd_kernel<<<p, BA_CLASS_THREADS, 0, s>>>(q);
    return check_launch("batch_all_loss_fwd");
  }
  const int rc = embnet_pairwise_dist_f32(emb, n, e, dist, 1, pw, ba_align16(embnet_pairwise_workspace_bytes(n, e)), stream);
  if (rc != EMBNET_OK) return rc;
  EMBNET_TRACE("embnet::batch_all_sweep_kernel", TRACE_BYTES, 8.0 * n * n, stream);
  batch_all_sweep_kernel<<<cdiv(n, BA_SWEEP_THREADS / 64), BA_SWEEP_THREADS, 0, s>>>(q);
  return check_launch("batch_all_loss_fwd");
}

extern "C" int embnet_batch_all_loss_bwd(const float* emb, int n, int e, const float* pair_w, const int32_t* n_active,
                                         const float* upstream, float* demb, void* stream) {
  EMBNET_CHECK_ARG(emb && pair_w && n_active && demb, "batch_all_loss_bwd: null pointer");
  EMBNET_CHECK_ARG(n >= 4 && n <= BA_MAX_N, "batch_all_loss_bwd: n=%d outside [4, %d]", n, BA_MAX_N);
  EMBNET_CHECK_ARG(e >= 1 && e <= BA_MAX_E, "batch_all_loss_bwd: e=%d outside [1, %d]", e, BA_MAX_E);
  EMBNET_TRACE_FLOP("embnet::batch_all_bwd_kernel", 2.0 * n * n * e, 4.0 * (2.0 * n * n + 2.0 * n * e), stream);
  batch_all_bwd_kernel<<<dim3(cdiv(n, 32), cdiv(e, 32)), 256, 0, (hipStream_t)stream>>>(emb, n, e, pair_w, n_active,
                                                                                           upstream, demb);
  return check_launch("batch_all_loss_bwd");
}
