// Multi-similarity loss (Wang et al., CVPR 2019; the pair-based baseline of "A Metric Learning Reality Check") over a
// class-contiguous P x K batch.  Build-defined: the reference has no pair-based loss.  Semantics: include/embnet.h.
//
//   X [N, E] fp32, N = P*K, rows c*K .. c*K+K-1 are class c.  S_ij = sum_c x_ic x_jc (cosine similarity of unit rows; unit rows
//   are not required).  Anchor i: positives P_i = the other rows of its class, negatives N_i = the rows of other classes.
//   Mining, one rounding form: n kept iff fl(S_in + eps) > min_p S_ip;  p kept iff fl(max_n S_in + eps) > S_ip.  fl is
//   monotone, so an anchor keeps a positive AND a negative (it is ACTIVE) or nothing.
//   t+_p = -alpha (S_ip - base), t-_n = beta (S_in - base);  m = max(0, max t) per side;
//   l_i = (m+ + log(e^{-m+} + sum_p e^{t+_p - m+})) / alpha + (m- + log(e^{-m-} + sum_n e^{t-_n - m-})) / beta   (0 if inactive)
//   loss = (1/N) sum_i l_i;   G[i,p] = -e^{t+_p - m+} / (e^{-m+} + sum),  G[i,n] = +e^{t-_n - m-} / (e^{-m-} + sum), 0 elsewhere.
//   backward, kept sets held constant:  demb_i = (g / N) sum_j (G_ij + G_ji) x_j.
//   counts = {kept positives, kept negatives, active anchors, kept positives + kept negatives}, exact.
//
// Forward, per-class path (N <= 512, K <= 16, K (E + N) floats in 64 KiB of LDS: batch_all.hip's fit rule), ONE launch: a
// workgroup per class holds its K rows and their K x N similarity rows in LDS (per-lane fmaf chain over the columns + wave sum),
// one wave per anchor mines, sums and writes the anchor's row of G (rows belong to their anchor: no atomics), the workgroup writes
// a per-class partial and the last workgroup to arrive (agent-scope ticket, the hand-off of fused_loss.hip) reduces the partials
// in class order.
// Forward, similarity-matrix path (everything else up to N = E = 4096): S = X X^T through embnet_dense_dgrad_f32 (the exact-fp32
// matrix-instruction GEMM, a k-ordered chain per element) into the workspace, then a sweep kernel takes one anchor row per wave
// from an LDS copy of its row of S; per-anchor partials, the same ticket and fixed-order reduction.
// Backward, one launch: Y = (G + G^T) X on the f64 matrix instructions (v_mfma_f64_16x16x4_f64), demb = (g/N) Y.  G + G^T is formed
// in f64 while staging; the result carries one fp32 rounding of an f64 sum, because the L2-normalisation backward that follows
// projects out the radial part and what remains can be far below sum_j |M_ij| |x_j|.
// Nothing is atomic in floating point, every reduction has a fixed order: bitwise reproducible.  No host synchronisation, no
// allocation: capturable in a graph.
#include <math.h>
#include "common.h"
#include "../../include/embnet.h"

namespace embnet {

constexpr int MS_MAX_N = 4096;
constexpr int MS_MAX_E = 4096;
constexpr int MS_CLASS_MAX_N = 512;
constexpr int MS_CLASS_MAX_K = 16;
constexpr int MS_LDS_FLOATS = 16 * 1024;                 // 64 KiB: K*(E + N) floats
constexpr int MS_CLASS_THREADS = 1024;                   // 16 waves: one per anchor, and the similarity phase's L2 round trips
constexpr int MS_SWEEP_THREADS = 256;                    // 4 anchors per workgroup, a 16 KiB similarity row each

__device__ __forceinline__ float ms_wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
// one rounding order everywhere: t = fl(c * fl(s - base)), c = -alpha or +beta; monotone in s
__device__ __forceinline__ float ms_t(float c, float s, float base) { return __fmul_rn(c, __fsub_rn(s, base)); }

struct MsAnchorOut { float loss; int npos, nneg; };

// One wave, one anchor (local index ai of class [lo, lo+k)), its similarity row srow[n] (LDS).  Writes all n entries of the
// anchor's row of G and returns (the same in every lane) the anchor's loss and its kept counts.
__device__ MsAnchorOut ms_anchor(const float* srow, int n, int k, int lo, int ai, float alpha, float beta, float base,
                                 float eps, float* grow, int lane) {
  float mn = INFINITY, mx = -INFINITY;
  for (int j = lane; j < k; j += 64)
    if (j != ai) mn = fminf(mn, srow[lo + j]);
  for (int col = lane; col < n; col += 64)
    if (col < lo || col >= lo + k) mx = fmaxf(mx, srow[col]);
  mn = ms_wave_min(mn);                                  // min over the positives
  mx = wave_max(mx);                                     // max over the negatives
  const float mxe = __fadd_rn(mx, eps);
  if (!(mxe > mn)) {                                     // inactive (wave-uniform): nothing kept on either side
    for (int col = lane; col < n; col += 64) grow[col] = 0.f;
    return MsAnchorOut{0.f, 0, 0};
  }
  // t is monotone in s, so the largest exponent of each side belongs to the hardest kept pair, which is kept whenever any is
  const float mp = fmaxf(0.f, ms_t(-alpha, mn, base));
  const float mg = fmaxf(0.f, ms_t(beta, mx, base));
  float sp = 0.f, sn = 0.f;
  int cp = 0, cn = 0;
  for (int j = lane; j < k; j += 64) {                   // lane-strided, column order
    const float s = srow[lo + j];
    if (j != ai && mxe > s) { sp += expf(__fsub_rn(ms_t(-alpha, s, base), mp)); ++cp; }
  }
  for (int col = lane; col < n; col += 64) {
    if (col >= lo && col < lo + k) continue;
    const float s = srow[col];
    if (__fadd_rn(s, eps) > mn) { sn += expf(__fsub_rn(ms_t(beta, s, base), mg)); ++cn; }
  }
  const float dp = __fadd_rn(expf(-mp), wave_sum(sp));   // e^{-m} + sum e^{t - m}
  const float dn = __fadd_rn(expf(-mg), wave_sum(sn));
  for (int col = lane; col < n; col += 64) {
    const float s = srow[col];
    float g = 0.f;
    if (col >= lo && col < lo + k) {
      if (col - lo != ai && mxe > s) g = -__fdiv_rn(expf(__fsub_rn(ms_t(-alpha, s, base), mp)), dp);
    } else if (__fadd_rn(s, eps) > mn) {
      g = __fdiv_rn(expf(__fsub_rn(ms_t(beta, s, base), mg)), dn);
    }
    grow[col] = g;
  }
  const float lp = __fdiv_rn(__fadd_rn(mp, logf(dp)), alpha);
  const float ln = __fdiv_rn(__fadd_rn(mg, logf(dn)), beta);
  return MsAnchorOut{__fadd_rn(lp, ln), wave_sum(cp), wave_sum(cn)};
}

struct MsParams {
  const float* emb; int n, p, k, e; float alpha, beta, base, eps;
  float* g; int32_t* counts; float* mean;
  int* ticket; double* part_loss; int4* part_cnt;        // workspace: arrival counter (zero between launches), partials
  const float* sim;                                      // similarity-matrix path: S [n][n]
};

// Arrival ticket (fused_loss.hip's hand-off): every storing wave drains, barrier, one lane releases at agent scope and takes
// the ticket; the last arriver acquires, re-arms the counter and reduces the `slots` partials in index order.
template <int THREADS>
__device__ void ms_finish(const MsParams& q, int slots) {
  __shared__ int s_last;
  __shared__ double ws_loss[THREADS / 64];
  __shared__ int ws_cnt[THREADS / 64][3];
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
  int c0 = 0, c1 = 0, c2 = 0;
  const int* pc = (const int*)q.part_cnt;
  for (int i = tid; i < slots; i += THREADS) {
    s += __hip_atomic_load(&q.part_loss[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    c0 += __hip_atomic_load(&pc[4 * i + 0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    c1 += __hip_atomic_load(&pc[4 * i + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    c2 += __hip_atomic_load(&pc[4 * i + 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  s = wave_sum(s);
  c0 = wave_sum(c0); c1 = wave_sum(c1); c2 = wave_sum(c2);
  if (lane == 0) { ws_loss[wave] = s; ws_cnt[wave][0] = c0; ws_cnt[wave][1] = c1; ws_cnt[wave][2] = c2; }
  __syncthreads();
  if (tid == 0) {
    double ts = 0.0;
    int t0 = 0, t1 = 0, t2 = 0;
    for (int w = 0; w < THREADS / 64; ++w) { ts += ws_loss[w]; t0 += ws_cnt[w][0]; t1 += ws_cnt[w][1]; t2 += ws_cnt[w][2]; }
    q.counts[0] = t0;                                    // <= N (K-1)
    q.counts[1] = t1;                                    // <= N (N-K) < 2^24
    q.counts[2] = t2;
    q.counts[3] = t0 + t1;
    *q.mean = (float)(ts / (double)q.n);
  }
}

// ---- forward, per-class path: grid = P workgroups ----------------------------------------------------------------------
__global__ __launch_bounds__(MS_CLASS_THREADS) void ms_class_fwd_kernel(MsParams q) {
  __shared__ __attribute__((aligned(16))) float lds[MS_LDS_FLOATS];
  __shared__ float wloss[MS_CLASS_MAX_K];
  __shared__ int wcnt[MS_CLASS_MAX_K][2];
  const int n = q.n, k = q.k, e = q.e, c = blockIdx.x, lo = c * k;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = MS_CLASS_THREADS / 64;
  float* A = lds;                                        // [k][e] the class's rows
  float* S = lds + k * e;                                // [k][n] similarities anchor -> row
  for (int i = tid; i < k * e; i += MS_CLASS_THREADS) A[i] = q.emb[(long)lo * e + i];
  __syncthreads();
  // row r of the block against the K anchors: the row is read once, eight loads in flight per lane (batch_all.hip's loop)
  for (int r = wave; r < n; r += NW) {
    const float* y = q.emb + (long)r * e;
    float acc[MS_CLASS_MAX_K];
#pragma unroll
    for (int a = 0; a < MS_CLASS_MAX_K; ++a) acc[a] = 0.f;
    for (int c0 = 0; c0 < e; c0 += 512) {
      float yv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { const int cc = c0 + lane + 64 * j; yv[j] = cc < e ? y[cc] : 0.f; }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int cc = c0 + lane + 64 * j;
        if (cc < e) {
#pragma unroll
          for (int a = 0; a < MS_CLASS_MAX_K; ++a)
            if (a < k) acc[a] = fmaf(A[a * e + cc], yv[j], acc[a]);
        }
      }
    }
#pragma unroll
    for (int a = 0; a < MS_CLASS_MAX_K; ++a) {
      if (a < k) {
        const float g = wave_sum(acc[a]);
        if (lane == 0) S[a * n + r] = g;
      }
    }
  }
  __syncthreads();
  if (wave < k) {
    const MsAnchorOut o = ms_anchor(S + wave * n, n, k, lo, wave, q.alpha, q.beta, q.base, q.eps,
                                    q.g + (long)(lo + wave) * n, lane);
    if (lane == 0) { wloss[wave] = o.loss; wcnt[wave][0] = o.npos; wcnt[wave][1] = o.nneg; }
  }
  __syncthreads();
  if (tid == 0) {                                        // the class's partial, anchors in order
    double s = 0.0;
    int cp = 0, cn = 0, ca = 0;
    for (int a = 0; a < k; ++a) { s += (double)wloss[a]; cp += wcnt[a][0]; cn += wcnt[a][1]; ca += wcnt[a][1] > 0; }
    q.part_loss[c] = s;
    q.part_cnt[c] = make_int4(cp, cn, ca, 0);
  }
  ms_finish<MS_CLASS_THREADS>(q, q.p);
}

// ---- forward, similarity-matrix path: grid = ceil(N / 4), one anchor per wave ------------------------------------------
__global__ __launch_bounds__(MS_SWEEP_THREADS) void ms_sweep_kernel(MsParams q) {
  __shared__ __attribute__((aligned(16))) float rows[MS_SWEEP_THREADS / 64][MS_MAX_N];
  const int n = q.n, k = q.k, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int a = blockIdx.x * (MS_SWEEP_THREADS / 64) + wave;
  float* srow = rows[wave];
  if (a < n) {                                           // wave-uniform
    const float* src = q.sim + (long)a * n;
    for (int col = lane; col < n; col += 64) srow[col] = src[col];
  }
  __syncthreads();
  if (a < n) {
    const int lo = (a / k) * k;
    const MsAnchorOut o = ms_anchor(srow, n, k, lo, a - lo, q.alpha, q.beta, q.base, q.eps, q.g + (long)a * n, lane);
    if (lane == 0) { q.part_loss[a] = (double)o.loss; q.part_cnt[a] = make_int4(o.npos, o.nneg, o.nneg > 0, 0); }
  }
  ms_finish<MS_SWEEP_THREADS>(q, n);
}

// ---- backward: demb = (g / N) (G + G^T) X ------------------------------------------------------------------------------
// grid (ceil(N/32), ceil(E/32)), 4 waves, each a 16 x 16 tile of the 32 x 32 block; j in chunks of 32 through LDS.
// v_mfma_f64_16x16x4_f64: A[i = l&15][k = l>>4], B[k = l>>4][col = l&15], D[row = (l>>4) + 4r][col = l&15] (the f64 map).
using f64x4 = __attribute__((ext_vector_type(4))) double;

__global__ __launch_bounds__(256) void ms_bwd_kernel(const float* __restrict__ emb, int n, int e, const float* __restrict__ gw,
                                                     const float* __restrict__ upstream, float* __restrict__ demb) {
  __shared__ float wa[32][33];                           // G[i0 + ii][j0 + jj]
  __shared__ float wb[32][33];                           // G[j0 + jj][i0 + ii], stored [jj][ii]
  __shared__ float xs[32][33];                           // X[j0 + jj][e0 + ee]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = blockIdx.x * 32, e0 = blockIdx.y * 32;
  const int ro = 16 * (wave >> 1), co = 16 * (wave & 1);
  const int lr = lane & 15, lk = lane >> 4;
  f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int j0 = 0; j0 < n; j0 += 32) {
    for (int t = tid; t < 1024; t += 256) {
      const int r = t >> 5, cc = t & 31;
      const int i = i0 + r, j = j0 + cc, jr = j0 + r, ic = i0 + cc, ec = e0 + cc;
      wa[r][cc] = (i < n && j < n) ? gw[(long)i * n + j] : 0.f;
      wb[r][cc] = (jr < n && ic < n) ? gw[(long)jr * n + ic] : 0.f;
      xs[r][cc] = (jr < n && ec < e) ? emb[(long)jr * e + ec] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const int kx = 4 * kk + lk;
      const double av = (double)wa[ro + lr][kx] + (double)wb[kx][ro + lr];
      const double bv = (double)xs[kx][co + lr];
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
    __syncthreads();
  }
  const double scale = (upstream ? (double)*upstream : 1.0) / (double)n;
  const int col = e0 + co + lr;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = i0 + ro + lk + 4 * r;
    if (row < n && col < e) demb[(long)row * e + col] = (float)(scale * acc[r]);
  }
}

static bool ms_class_path_fits(int p, int k, int e) {
  const long n = (long)p * k;
  return k <= MS_CLASS_MAX_K && n <= MS_CLASS_MAX_N && (long)k * (e + n) <= MS_LDS_FLOATS;
}

static size_t ms_align16(size_t b) { return (b + 15) / 16 * 16; }

static bool ms_range_ok(int p, int k, int e) {
  return p >= 2 && k >= 2 && e >= 1 && e <= MS_MAX_E && (long long)p * k <= MS_MAX_N;
}

}  // namespace embnet

using namespace embnet;

// workspace: [16 B ticket][n f64 partial losses][n int4 partial counts][n*n f32 similarities]
// (sized for both forward paths, so a caller may force either)
extern "C" size_t embnet_ms_loss_workspace_bytes(int p, int k, int e) {
  if (!ms_range_ok(p, k, e)) return 0;
  const size_t n = (size_t)p * k;
  return 16 + ms_align16(n * 8) + n * 16 + ms_align16(n * n * 4);
}

extern "C" int embnet_ms_loss_path(int p, int k, int e) {
  if (!ms_range_ok(p, k, e)) return 0;
  return ms_class_path_fits(p, k, e) ? EMBNET_MS_PER_CLASS : EMBNET_MS_SIMILARITY_MATRIX;
}

extern "C" int embnet_ms_loss_fwd(const float* emb, int p, int k, int e, float alpha, float beta, float base, float epsilon,
                                  int path, float* pair_g, int32_t* counts, float* mean_loss, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  EMBNET_CHECK_ARG(emb && pair_g && counts && mean_loss && workspace, "ms_loss_fwd: null pointer");
  EMBNET_CHECK_ARG(p >= 2 && k >= 2, "ms_loss_fwd: need p >= 2 classes and k >= 2 samples (p=%d k=%d)", p, k);
  EMBNET_CHECK_ARG((long long)p * k <= MS_MAX_N, "ms_loss_fwd: n = p*k = %lld > %d", (long long)p * k, MS_MAX_N);
  EMBNET_CHECK_ARG(e >= 1 && e <= MS_MAX_E, "ms_loss_fwd: e=%d outside [1, %d]", e, MS_MAX_E);
  EMBNET_CHECK_ARG(isfinite(alpha) && alpha > 0.f, "ms_loss_fwd: alpha=%g must be finite and positive", (double)alpha);
  EMBNET_CHECK_ARG(isfinite(beta) && beta > 0.f, "ms_loss_fwd: beta=%g must be finite and positive", (double)beta);
  EMBNET_CHECK_ARG(isfinite(base), "ms_loss_fwd: base=%g must be finite", (double)base);
  EMBNET_CHECK_ARG(isfinite(epsilon) && epsilon >= 0.f, "ms_loss_fwd: epsilon=%g must be finite and non-negative",
                   (double)epsilon);
  EMBNET_CHECK_ARG(path >= 0 && path <= EMBNET_MS_SIMILARITY_MATRIX, "ms_loss_fwd: unknown path %d", path);
  EMBNET_CHECK_ARG(path != EMBNET_MS_PER_CLASS || ms_class_path_fits(p, k, e),
                   "ms_loss_fwd: p=%d k=%d e=%d does not fit the per-class path", p, k, e);
  EMBNET_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "ms_loss_fwd: workspace must be 16-byte aligned");
  if (workspace_bytes < embnet_ms_loss_workspace_bytes(p, k, e))
    return fail(EMBNET_EWORKSPACE, "ms_loss_fwd: workspace %zu < %zu bytes", workspace_bytes,
                embnet_ms_loss_workspace_bytes(p, k, e));
  const int n = p * k;
  if (path == 0) path = embnet_ms_loss_path(p, k, e);
  char* ws = (char*)workspace;
  double* part_loss = (double*)(ws + 16);
  int4* part_cnt = (int4*)(ws + 16 + ms_align16((size_t)n * 8));
  float* sim = (float*)((char*)part_cnt + (size_t)n * 16);
  MsParams q{emb, n, p, k, e, alpha, beta, base, epsilon, pair_g, counts, mean_loss, (int*)ws, part_loss, part_cnt, sim};
  hipStream_t s = (hipStream_t)stream;
  if (path == EMBNET_MS_PER_CLASS) {
    EMBNET_TRACE_FLOP("embnet::ms_class_fwd_kernel", 2.0 * n * n * e, 4.0 * n * e * (p + 1.0) + 4.0 * n * n, stream);
    ms_class_fwd_kernel<<<p, MS_CLASS_THREADS, 0, s>>>(q);
    return check_launch("ms_loss_fwd");
  }
  const int rc = embnet_dense_dgrad_f32(emb, emb, sim, n, n, e, stream);      // S = X X^T
  if (rc != EMBNET_OK) return rc;
  EMBNET_TRACE("embnet::ms_sweep_kernel", TRACE_BYTES, 8.0 * n * n, stream);
  ms_sweep_kernel<<<cdiv(n, MS_SWEEP_THREADS / 64), MS_SWEEP_THREADS, 0, s>>>(q);
  return check_launch("ms_loss_fwd");
}

extern "C" int embnet_ms_loss_bwd(const float* emb, int n, int e, const float* pair_g, const float* upstream, float* demb,
                                  void* stream) {
  EMBNET_CHECK_ARG(emb && pair_g && demb, "ms_loss_bwd: null pointer");
  EMBNET_CHECK_ARG(n >= 4 && n <= MS_MAX_N, "ms_loss_bwd: n=%d outside [4, %d]", n, MS_MAX_N);
  EMBNET_CHECK_ARG(e >= 1 && e <= MS_MAX_E, "ms_loss_bwd: e=%d outside [1, %d]", e, MS_MAX_E);
  EMBNET_TRACE_FLOP("embnet::ms_bwd_kernel", 2.0 * n * n * e, 4.0 * (2.0 * n * n + 2.0 * n * e), stream);
  ms_bwd_kernel<<<dim3(cdiv(n, 32), cdiv(e, 32)), 256, 0, (hipStream_t)stream>>>(emb, n, e, pair_g, upstream, demb);
  return check_launch("ms_loss_bwd");
}
