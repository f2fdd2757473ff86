// The forward skeleton the pair-based losses over a class-contiguous P x K batch share (multi_similarity.hip, supcon.hip): what
// differs between them is what ONE WAVE does with ONE ANCHOR's row of similarities, the Body.
//
//   X [N, E] fp32, N = P*K, rows c*K .. c*K+K-1 are class c;  S = X X^T.
//   per-class path (N <= 512, K <= 16, K (E + N) floats in 64 KiB of LDS: batch_all.hip's fit rule), ONE launch: a workgroup per
//   class holds its K rows and their K x N similarity rows in LDS (per-lane fmaf chain over the columns + wave sum), one wave per
//   anchor runs the Body, the workgroup writes a per-class partial and the last workgroup to arrive (agent-scope ticket, the
//   hand-off of fused_loss.hip) reduces the partials in class order.
//   similarity-matrix path (everything else up to N = E = 4096): S through embnet_dense_dgrad_f32 (the exact-fp32 matrix-instruction
//   GEMM, a k-ordered chain per element) into the workspace, then a sweep takes one anchor row per wave from an LDS copy of its row
//   of S; per-anchor partials, the same ticket and fixed-order reduction.
//
// A Body is a struct with
//   struct Args { ... };                                       the loss's parameters, passed by value with the launch
//   static __device__ PairAnchorOut anchor(const float* srow, int n, int k, int lo, int ai, const Args& a, float* grow, int lane);
//       one wave, anchor ai of class [lo, lo + k), its similarity row srow[n] (LDS): writes all n entries of the anchor's row of
//       the pair weights and returns, the same in every lane, the anchor's loss and two counters;
//   static __device__ int third(const PairAnchorOut& o);       a third per-anchor counter derived from the two
//   static __device__ void write_counts(int32_t* counts, int n, int k, int c0, int c1, int c2);     the block's totals -> counts[]
// The kernels themselves stay in the loss's own file (their names are what a profile shows); they call pair_class_fwd /
// pair_sweep_fwd.  Nothing is atomic in floating point, every reduction has a fixed order; no host synchronisation, no allocation.
#pragma once
#include "common.h"

namespace embnet {

constexpr int PAIR_MAX_N = 4096;
constexpr int PAIR_MAX_E = 4096;
constexpr int PAIR_CLASS_MAX_N = 512;
constexpr int PAIR_CLASS_MAX_K = 16;
constexpr int PAIR_LDS_FLOATS = 16 * 1024;               // 64 KiB: K*(E + N) floats
constexpr int PAIR_CLASS_THREADS = 1024;                 // 16 waves: one per anchor, and the similarity phase's L2 round trips
constexpr int PAIR_SWEEP_THREADS = 256;                  // 4 anchors per workgroup, a 16 KiB similarity row each

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

struct PairAnchorOut { float loss; int c0, c1; };

template <class Body>
struct PairParams {
  const float* emb; int n, p, k, e; typename Body::Args a;
  float* g; int32_t* counts; float* mean;
  int* ticket; double* part_loss; int4* part_cnt;        // workspace: arrival counter (zero between launches), partials
  const float* sim;                                      // similarity-matrix path: S [n][n]
};

// Arrival ticket (fused_loss.hip's hand-off): every storing wave drains, barrier, one lane releases at agent scope and takes
// the ticket; the last arriver acquires, re-arms the counter and reduces the `slots` partials in index order.
template <class Body, int THREADS>
__device__ __forceinline__ void pair_finish(const PairParams<Body>& q, int slots) {
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
    Body::write_counts(q.counts, q.n, q.k, t0, t1, t2);
    *q.mean = (float)(ts / (double)q.n);
  }
}

// ---- forward, per-class path: grid = P workgroups of PAIR_CLASS_THREADS ------------------------------------------------
template <class Body>
__device__ __forceinline__ void pair_class_fwd(const PairParams<Body>& q) {
  __shared__ __attribute__((aligned(16))) float lds[PAIR_LDS_FLOATS];
  __shared__ float wloss[PAIR_CLASS_MAX_K];
  __shared__ int wcnt[PAIR_CLASS_MAX_K][2];
  const int n = q.n, k = q.k, e = q.e, c = blockIdx.x, lo = c * k;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = PAIR_CLASS_THREADS / 64;
  float* A = lds;                                        // [k][e] the class's rows
  float* S = lds + k * e;                                // [k][n] similarities anchor -> row
  for (int i = tid; i < k * e; i += PAIR_CLASS_THREADS) A[i] = q.emb[(long)lo * e + i];
  __syncthreads();
  // row r of the block against the K anchors: the row is read once, eight loads in flight per lane (batch_all.hip's loop)
  for (int r = wave; r < n; r += NW) {
    const float* y = q.emb + (long)r * e;
    float acc[PAIR_CLASS_MAX_K];
#pragma unroll
    for (int a = 0; a < PAIR_CLASS_MAX_K; ++a) acc[a] = 0.f;
    for (int c0 = 0; c0 < e; c0 += 512) {
      float yv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { const int cc = c0 + lane + 64 * j; yv[j] = cc < e ? y[cc] : 0.f; }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int cc = c0 + lane + 64 * j;
        if (cc < e) {
#pragma unroll
          for (int a = 0; a < PAIR_CLASS_MAX_K; ++a)
            if (a < k) acc[a] = fmaf(A[a * e + cc], yv[j], acc[a]);
        }
      }
    }
#pragma unroll
    for (int a = 0; a < PAIR_CLASS_MAX_K; ++a) {
      if (a < k) {
        const float g = wave_sum(acc[a]);
        if (lane == 0) S[a * n + r] = g;
      }
    }
  }
  __syncthreads();
  if (wave < k) {
    const PairAnchorOut o = Body::anchor(S + wave * n, n, k, lo, wave, q.a, q.g + (long)(lo + wave) * n, lane);
    if (lane == 0) { wloss[wave] = o.loss; wcnt[wave][0] = o.c0; wcnt[wave][1] = o.c1; }
  }
  __syncthreads();
  if (tid == 0) {                                        // the class's partial, anchors in order
    double s = 0.0;
    int c0 = 0, c1 = 0, c2 = 0;
    for (int a = 0; a < k; ++a) {
      s += (double)wloss[a]; c0 += wcnt[a][0]; c1 += wcnt[a][1];
      c2 += Body::third(PairAnchorOut{wloss[a], wcnt[a][0], wcnt[a][1]});
    }
    q.part_loss[c] = s;
    q.part_cnt[c] = make_int4(c0, c1, c2, 0);
  }
  pair_finish<Body, PAIR_CLASS_THREADS>(q, q.p);
}

// ---- forward, similarity-matrix path: grid = ceil(N / 4) workgroups of PAIR_SWEEP_THREADS, one anchor per wave -----------
template <class Body>
__device__ __forceinline__ void pair_sweep_fwd(const PairParams<Body>& q) {
  __shared__ __attribute__((aligned(16))) float rows[PAIR_SWEEP_THREADS / 64][PAIR_MAX_N];
  const int n = q.n, k = q.k, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int a = blockIdx.x * (PAIR_SWEEP_THREADS / 64) + wave;
  float* srow = rows[wave];
  if (a < n) {                                           // wave-uniform
    const float* src = q.sim + (long)a * n;
    for (int col = lane; col < n; col += 64) srow[col] = src[col];
  }
  __syncthreads();
  if (a < n) {
    const int lo = (a / k) * k;
    const PairAnchorOut o = Body::anchor(srow, n, k, lo, a - lo, q.a, q.g + (long)a * n, lane);
    if (lane == 0) { q.part_loss[a] = (double)o.loss; q.part_cnt[a] = make_int4(o.c0, o.c1, Body::third(o), 0); }
  }
  pair_finish<Body, PAIR_SWEEP_THREADS>(q, n);
}

// ---- host side: range, fit rule, workspace layout ------------------------------------------------------------------------
inline bool pair_class_path_fits(int p, int k, int e) {
  const long n = (long)p * k;
  return k <= PAIR_CLASS_MAX_K && n <= PAIR_CLASS_MAX_N && (long)k * (e + n) <= PAIR_LDS_FLOATS;
}

inline size_t pair_align16(size_t b) { return (b + 15) / 16 * 16; }

inline bool pair_range_ok(int p, int k, int e) {
  return p >= 2 && k >= 2 && e >= 1 && e <= PAIR_MAX_E && (long long)p * k <= PAIR_MAX_N;
}

// workspace: [16 B ticket][n f64 partial losses][n int4 partial counts][n*n f32 similarities]
// (sized for both forward paths, so a caller may force either); 0 outside the range
inline size_t pair_workspace_bytes(int p, int k, int e) {
  if (!pair_range_ok(p, k, e)) return 0;
  const size_t n = (size_t)p * k;
  return 16 + pair_align16(n * 8) + n * 16 + pair_align16(n * n * 4);
}

struct PairWorkspace { int* ticket; double* part_loss; int4* part_cnt; float* sim; };

inline PairWorkspace pair_workspace(void* workspace, int n) {
  char* ws = (char*)workspace;
  int4* part_cnt = (int4*)(ws + 16 + pair_align16((size_t)n * 8));
  return PairWorkspace{(int*)ws, (double*)(ws + 16), part_cnt, (float*)((char*)part_cnt + (size_t)n * 16)};
}

// The argument checks the two losses share, in multi_similarity's words.  `what` is the entry point's name without `embnet_`.
inline int pair_check_common(const char* what, const void* emb, const void* pair_g, const void* counts, const void* mean_loss,
                             const void* workspace, int p, int k, int e) {
  EMBNET_CHECK_ARG(emb && pair_g && counts && mean_loss && workspace, "%s: null pointer", what);
  EMBNET_CHECK_ARG(p >= 2 && k >= 2, "%s: need p >= 2 classes and k >= 2 samples (p=%d k=%d)", what, p, k);
  EMBNET_CHECK_ARG((long long)p * k <= PAIR_MAX_N, "%s: n = p*k = %lld > %d", what, (long long)p * k, PAIR_MAX_N);
  EMBNET_CHECK_ARG(e >= 1 && e <= PAIR_MAX_E, "%s: e=%d outside [1, %d]", what, e, PAIR_MAX_E);
  return EMBNET_OK;
}

inline int pair_check_path_and_workspace(const char* what, int p, int k, int e, int path, const void* workspace,
                                         size_t workspace_bytes) {
  EMBNET_CHECK_ARG(path >= 0 && path <= 2, "%s: unknown path %d", what, path);
  EMBNET_CHECK_ARG(path != 1 || pair_class_path_fits(p, k, e), "%s: p=%d k=%d e=%d does not fit the per-class path", what, p, k,
                   e);
  EMBNET_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "%s: workspace must be 16-byte aligned", what);
  if (workspace_bytes < pair_workspace_bytes(p, k, e))
    return fail(EMBNET_EWORKSPACE, "%s: workspace %zu < %zu bytes", what, workspace_bytes, pair_workspace_bytes(p, k, e));
  return EMBNET_OK;
}

}  // namespace embnet
