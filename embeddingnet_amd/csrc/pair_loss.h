// The skeleton the losses over a class-contiguous P x K batch share (batch_all.hip, multi_similarity.hip, supcon.hip, ap_loss.hip,
// circle_loss.hip): what
// differs between them is what ONE WAVE does with ONE ANCHOR's row of the pair matrix, the Body.
//
//   X [N, E] fp32, N = P*K, rows c*K .. c*K+K-1 are class c;  the pair matrix S is X X^T (similarities) or the squared distances.
//   per-class path (N <= 512, K <= 16, K (E + N) floats in 64 KiB of LDS), ONE launch: a workgroup per class holds its K rows and
//   their K x N rows of S in LDS (per-lane chain of Body::term over the columns + wave sum), one wave per anchor runs the Body,
//   the workgroup writes a per-class partial and the last workgroup to arrive (agent-scope ticket, the hand-off of
//   fused_loss.hip) reduces the partials in class order.
//   matrix path (everything else up to N = E = 4096): S through Body::matrix (a library GEMM) into the workspace, then a sweep
//   takes one anchor row per wave from an LDS copy of its row of S; per-anchor partials, the same ticket and fixed-order reduction.
//   backward, one launch: Y = (M + M^T) X on the f64 matrix instructions, M the pair weights the forward wrote; an Epilogue turns
//   Y into demb.
//
// A Body is a struct with
//   struct Args { ... };                                       the loss's parameters, passed by value with the launch
//   using Sum = float or double;                               the type of an anchor's loss (widened to f64 exactly from there on)
//   static constexpr int CLASS_TRACE_UNIT;                     how the per-class kernel's trace entry counts its work
//   static __device__ float term(float a, float y, float acc); per-class path: one column's step of S's chain
//   static int matrix(const float* emb, int n, int e, float* s, void* extra, void* stream);    matrix path, host: S [n][n]
//   static size_t matrix_extra_bytes(int n, int e);            workspace bytes `matrix` needs behind S
//   static __device__ PairAnchorOut<Sum> anchor(const float* srow, int n, int k, int lo, int ai, const Args& a, float* grow, int lane);
//       one wave, anchor ai of class [lo, lo + k), its row srow[n] of S (LDS): writes all n entries of the anchor's row of the
//       pair weights and returns, the same in every lane, the anchor's loss and two counters;
//   static __device__ int third(const PairAnchorOut<Sum>& o);  a third per-anchor counter derived from the two
//   static __device__ void finish(const PairParams<Body>& q, double total, int c0, int c1, int c2);     the batch's f64 loss
//       total and counter totals -> every output (counts, mean, whatever else Args points to); one thread
// The counters are int: a Body states why its totals fit.  PairDotBody has term / matrix for S = X X^T.
// The kernels themselves stay in the loss's own file (their names are what a profile shows); they call pair_class_fwd /
// pair_sweep_fwd / pair_bwd, and pair_launch launches them.  Nothing is atomic in floating point, every reduction has a fixed
// order; no host synchronisation, no allocation.
//
// Four pieces here know nothing of P x K: the arrival ticket (common.h's last_workgroup_to_arrive), reduce_partials (the last
// workgroup's fixed-order totals), anchor_dots (rows of B against a few anchors in LDS) and mm_f64_tile (the 32 x 32 f64
// matrix-instruction product).  rect_loss.h builds the rectangle losses' skeleton (a batch against proxies, centres or the memory
// bank) on the same four.  The P x K skeleton proper is the Body, PairParams,
// pair_class_fwd / pair_sweep_fwd / pair_finish / pair_bwd, the fit rule, the workspace layout, the checks and pair_launch.
#pragma once
#include <math.h>
#include "common.h"
#include "../../include/embnet.h"

namespace embnet {

constexpr int PAIR_MAX_N = 4096;
constexpr int PAIR_MAX_E = 4096;
constexpr int PAIR_CLASS_MAX_N = 512;
constexpr int PAIR_CLASS_MAX_K = 16;
constexpr int PAIR_LDS_FLOATS = 16 * 1024;               // 64 KiB: K*(E + N) floats
constexpr int PAIR_CLASS_THREADS = 1024;                 // 16 waves: one per anchor, and the pair-matrix phase's L2 round trips
constexpr int PAIR_SWEEP_THREADS = 256;                  // 4 anchors per workgroup, a 16 KiB row of S each
enum { PAIR_PER_CLASS = 1, PAIR_MATRIX = 2 };            // the value of every loss's two path constants (include/embnet.h)

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// Multi-similarity's per-pair pieces, stated once for multi_similarity.hip (pair sets by P x K contiguity) and xbm.hip (pair sets by
// two label vectors).  One rounding order everywhere: t = fl(c * fl(s - base)), c = -alpha or +beta; monotone in s.
__device__ __forceinline__ float ms_t(float c, float s, float base) { return __fmul_rn(c, __fsub_rn(s, base)); }
// a kept pair's term of the stable side: e^{t - m}
__device__ __forceinline__ float ms_term(float c, float s, float base, float m) { return expf(__fsub_rn(ms_t(c, s, base), m)); }
// a side's loss from its maximum m and its denominator d = e^{-m} + sum e^{t - m} >= 1: (m + log d) / c
__device__ __forceinline__ float ms_side(float m, float d, float c) { return __fdiv_rn(__fadd_rn(m, logf(d)), c); }

// Circle loss's per-pair pieces and its row, stated once for circle_loss.hip (pair sets by P x K contiguity, the row in LDS) and
// xbm.hip (pair sets by two label vectors, the row in global memory).  One rounding order everywhere (include/embnet.h):
//   alpha+ = max(fl(O+ - s), 0),  a+ = fl(-gamma fl(alpha+ fl(s - D+)));   alpha- = max(fl(s - O-), 0),  a- = fl(gamma fl(alpha- fl(s - D-)))
struct CircleArgs { float gamma, op, on, dp, dn; };      // gamma, O+ = fl(1 + m), O- = -m, D+ = fl(1 - m), D- = m
__device__ __forceinline__ float circle_alpha(int role, float s, const CircleArgs& a) {
  return fmaxf(role > 0 ? __fsub_rn(a.op, s) : __fsub_rn(s, a.on), 0.f);
}
__device__ __forceinline__ float circle_logit(int role, float alpha, float s, const CircleArgs& a) {
  return role > 0 ? __fmul_rn(-a.gamma, __fmul_rn(alpha, __fsub_rn(s, a.dp))) : __fmul_rn(a.gamma, __fmul_rn(alpha, __fsub_rn(s, a.dn)));
}

struct CircleRowOut { float loss; int viol, cp, cn, active; };   // cp / cn: the side's pairs with alpha > 0

// One wave, one anchor's row srow[cols] of S; role(col) = +1 a positive, -1 a negative, 0 neither.  Three lane-strided passes in
// column order: the sides' largest logits and the extreme similarities; the sums e^{a - M} (>= 1: the largest logit gives e^0) and
// the counters; all `cols` entries of the row of G.  An empty side (min over no positive = +inf, max over no negative = -inf)
// leaves a zero row and no loss.  The same result in every lane.
template <class Role>
__device__ __forceinline__ CircleRowOut circle_row(const float* __restrict__ srow, int cols, const Role& role, const CircleArgs& a,
                                                   float* __restrict__ grow, int lane) {
  float mn = INFINITY, mx = -INFINITY, Mp = -INFINITY, Mn = -INFINITY;
  for (int col = lane; col < cols; col += 64) {
    const int r = role(col);
    if (r == 0) continue;
    const float s = srow[col];
    const float t = circle_logit(r, circle_alpha(r, s, a), s, a);
    if (r > 0) { mn = fminf(mn, s); Mp = fmaxf(Mp, t); }
    else { mx = fmaxf(mx, s); Mn = fmaxf(Mn, t); }
  }
  mn = wave_min(mn);                                     // min over the positives (+inf: none)
  mx = wave_max(mx);                                     // max over the negatives (-inf: none)
  if (mn == INFINITY || mx == -INFINITY) {               // an empty side (wave-uniform)
    for (int col = lane; col < cols; col += 64) grow[col] = 0.f;
    return CircleRowOut{0.f, 0, 0, 0, 0};
  }
  Mp = wave_max(Mp);
  Mn = wave_max(Mn);
  float sp = 0.f, sn = 0.f;
  int cp = 0, cn = 0;
  for (int col = lane; col < cols; col += 64) {
    const int r = role(col);
    if (r == 0) continue;
    const float s = srow[col];
    const float al = circle_alpha(r, s, a);
    const float t = circle_logit(r, al, s, a);
    if (r > 0) { sp += expf(__fsub_rn(t, Mp)); cp += al > 0.f; }
    else { sn += expf(__fsub_rn(t, Mn)); cn += al > 0.f; }
  }
  const float dp = wave_sum(sp), dn = wave_sum(sn);      // >= 1 each
  const float z = __fadd_rn(__fadd_rn(Mp, logf(dp)), __fadd_rn(Mn, logf(dn)));
  const float t1 = expf(-fabsf(z));                      // softplus and sigmoid from e^{-|z|} <= 1
  const float d1 = __fadd_rn(1.f, t1);
  const float sg = __fmul_rn(__fdiv_rn(z >= 0.f ? 1.f : t1, d1), a.gamma);      // sigma gamma
  const float wp = __fdiv_rn(sg, dp), wn = __fdiv_rn(sg, dn);
  for (int col = lane; col < cols; col += 64) {
    const int r = role(col);
    float g = 0.f;
    if (r != 0) {
      const float s = srow[col];
      const float al = circle_alpha(r, s, a);
      const float t = circle_logit(r, al, s, a);
      g = r > 0 ? -__fmul_rn(wp, __fmul_rn(al, expf(__fsub_rn(t, Mp)))) : __fmul_rn(wn, __fmul_rn(al, expf(__fsub_rn(t, Mn))));
    }
    grow[col] = g;
  }
  return CircleRowOut{__fadd_rn(fmaxf(z, 0.f), logf(d1)), mx >= mn, wave_sum(cp), wave_sum(cn), 1};
}

// The parameters on the host: m in [0, 1] and gamma > 0, both finite -> the five constants, each one fp32 operation.
inline int circle_args(const char* what, float m, float gamma, CircleArgs& a) {
  EMBNET_CHECK_ARG(isfinite(m) && m >= 0.f && m <= 1.f, "%s: m=%g must be finite and in [0, 1]", what, (double)m);
  EMBNET_CHECK_ARG(isfinite(gamma) && gamma > 0.f, "%s: gamma=%g must be finite and positive", what, (double)gamma);
  a = CircleArgs{gamma, 1.f + m, -m, 1.f - m, m};
  return EMBNET_OK;
}

template <class Sum>
struct PairAnchorOut { Sum loss; int c0, c1; };

template <class Body>
struct PairParams {
  const float* emb; int n, p, k, e; typename Body::Args a;
  float* g; int32_t* counts; float* mean;
  int* ticket; double* part_loss; int4* part_cnt;        // workspace: arrival counter (zero between launches), partials
  const float* sim;                                      // matrix path: S [n][n]
};

// S = X X^T: the per-class chain is a dot product, the matrix comes from the exact-fp32 matrix-instruction GEMM (a k-ordered
// chain per element).
struct PairDotBody {
  static constexpr int CLASS_TRACE_UNIT = TRACE_FLOP;
  static __device__ float term(float a, float y, float acc) { return fmaf(a, y, acc); }
  static int matrix(const float* emb, int n, int e, float* s, void*, void* stream) {
    return embnet_dense_dgrad_f32(emb, emb, s, n, n, e, stream);
  }
  static size_t matrix_extra_bytes(int, int) { return 0; }
};

// Totals of `slots` per-anchor partials (NS f64 sums, a stride of NS doubles; NC counters out of an int4) for the last
// workgroup, all THREADS threads calling: thread-strided relaxed agent-scope loads, wave butterflies, then thread 0 adds the
// waves in order.  The totals are thread 0's: true there, false elsewhere.
template <int THREADS, int NS, int NC>
__device__ __forceinline__ bool reduce_partials(const double* part_loss, const int4* part_cnt, int slots, double (&ts)[NS],
                                                int (&tc)[NC]) {
  __shared__ double ws_loss[THREADS / 64][NS];
  __shared__ int ws_cnt[THREADS / 64][NC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int* pc = (const int*)part_cnt;
#pragma unroll
  for (int j = 0; j < NS; ++j) ts[j] = 0.0;
#pragma unroll
  for (int j = 0; j < NC; ++j) tc[j] = 0;
  for (int i = tid; i < slots; i += THREADS) {
#pragma unroll
    for (int j = 0; j < NS; ++j) ts[j] += __hip_atomic_load(&part_loss[NS * i + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
    for (int j = 0; j < NC; ++j) tc[j] += __hip_atomic_load(&pc[4 * i + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
#pragma unroll
  for (int j = 0; j < NS; ++j) ts[j] = wave_sum(ts[j]);   // the butterflies first, one store block behind them: they interleave
#pragma unroll
  for (int j = 0; j < NC; ++j) tc[j] = wave_sum(tc[j]);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < NS; ++j) ws_loss[wave][j] = ts[j];
#pragma unroll
    for (int j = 0; j < NC; ++j) ws_cnt[wave][j] = tc[j];
  }
  __syncthreads();
  if (tid != 0) return false;
#pragma unroll
  for (int j = 0; j < NS; ++j) ts[j] = 0.0;
#pragma unroll
  for (int j = 0; j < NC; ++j) tc[j] = 0;
  for (int w = 0; w < THREADS / 64; ++w) {
#pragma unroll
    for (int j = 0; j < NS; ++j) ts[j] += ws_loss[w][j];
#pragma unroll
    for (int j = 0; j < NC; ++j) tc[j] += ws_cnt[w][j];
  }
  return true;
}

// The last workgroup to arrive reduces the `slots` partials in index order and hands the totals to the Body.
template <class Body, int THREADS>
__device__ __forceinline__ void pair_finish(const PairParams<Body>& q, int slots) {
  if (!last_workgroup_to_arrive(q.ticket)) return;
  double ts[1];
  int tc[3];
  if (reduce_partials<THREADS>(q.part_loss, q.part_cnt, slots, ts, tc)) Body::finish(q, ts[0], tc[0], tc[1], tc[2]);
}

// Rows r = wave, wave + NW, ... of B [nb][e] against the first na <= MAX_A of the anchors A [MAX_A][e] held in LDS, all NW waves
// calling: S[a * nb + r] = the lane-strided chain of Term::term over the columns + wave sum.  A row is read once, eight loads in
// flight per lane (fused_loss.hip's loop).
template <int MAX_A, int NW, class Term>
__device__ __forceinline__ void anchor_dots(const float* A, int na, const float* B, int nb, int e, float* S) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int r = wave; r < nb; r += NW) {
    const float* y = B + (long)r * e;
    float acc[MAX_A];
#pragma unroll
    for (int a = 0; a < MAX_A; ++a) acc[a] = 0.f;
    for (int c0 = 0; c0 < e; c0 += 512) {
      float yv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { const int cc = c0 + lane + 64 * j; yv[j] = cc < e ? y[cc] : 0.f; }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int cc = c0 + lane + 64 * j;
        if (cc < e) {
#pragma unroll
          for (int a = 0; a < MAX_A; ++a)
            if (a < na) acc[a] = Term::term(A[a * e + cc], yv[j], acc[a]);
        }
      }
    }
#pragma unroll
    for (int a = 0; a < MAX_A; ++a) {
      if (a < na) {
        const float g = wave_sum(acc[a]);
        if (lane == 0) (S + r)[a * nb] = g;              // S + r first: keeps MAX_A row pointers out of the scalar registers
      }
    }
  }
}

// ---- forward, per-class path: grid = P workgroups of PAIR_CLASS_THREADS ------------------------------------------------
template <class Body>
__device__ __forceinline__ void pair_class_fwd(const PairParams<Body>& q) {
  using Sum = typename Body::Sum;
  __shared__ __attribute__((aligned(16))) float lds[PAIR_LDS_FLOATS];
  __shared__ Sum wloss[PAIR_CLASS_MAX_K];
  __shared__ int wcnt[PAIR_CLASS_MAX_K][2];
  const int n = q.n, k = q.k, e = q.e, c = blockIdx.x, lo = c * k;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = PAIR_CLASS_THREADS / 64;
  float* A = lds;                                        // [k][e] the class's rows
  float* S = lds + k * e;                                // [k][n] pair matrix, anchor -> row
  for (int i = tid; i < k * e; i += PAIR_CLASS_THREADS) A[i] = q.emb[(long)lo * e + i];
  __syncthreads();
  anchor_dots<PAIR_CLASS_MAX_K, NW, Body>(A, k, q.emb, n, e, S);
  __syncthreads();
  if (wave < k) {
    const PairAnchorOut<Sum> o = Body::anchor(S + wave * n, n, k, lo, wave, q.a, q.g + (long)(lo + wave) * n, lane);
    if (lane == 0) { wloss[wave] = o.loss; wcnt[wave][0] = o.c0; wcnt[wave][1] = o.c1; }
  }
  __syncthreads();
  if (tid == 0) {                                        // the class's partial, anchors in order
    double s = 0.0;
    int c0 = 0, c1 = 0, c2 = 0;
    for (int a = 0; a < k; ++a) {
      s += (double)wloss[a]; c0 += wcnt[a][0]; c1 += wcnt[a][1];
      c2 += Body::third(PairAnchorOut<Sum>{wloss[a], wcnt[a][0], wcnt[a][1]});
    }
    q.part_loss[c] = s;
    q.part_cnt[c] = make_int4(c0, c1, c2, 0);
  }
  pair_finish<Body, PAIR_CLASS_THREADS>(q, q.p);
}

// ---- forward, matrix path: grid = ceil(N / 4) workgroups of PAIR_SWEEP_THREADS, one anchor per wave -----------------------
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
    const PairAnchorOut<typename Body::Sum> o = Body::anchor(srow, n, k, lo, a - lo, q.a, q.g + (long)a * n, lane);
    if (lane == 0) { q.part_loss[a] = (double)o.loss; q.part_cnt[a] = make_int4(o.c0, o.c1, Body::third(o), 0); }
  }
  pair_finish<Body, PAIR_SWEEP_THREADS>(q, n);
}

// ---- the f64 tile product: Out[i][col] = sum_{j in [jb, je)} M(i, j) B[j][col], i < R, col < e ------------------------------
// grid (ceil(R/32), ceil(e/32)), 256 threads: 4 waves, each a 16 x 16 tile of the 32 x 32 block; j in chunks of 32 through LDS
// (jb is a multiple of 32 and je of 32 or J: j < J guards the tail).
// v_mfma_f64_16x16x4_f64: A[i = l&15][k = l>>4], B[k = l>>4][col = l&15], D[row = (l>>4) + 4r][col = l&15] (the f64 map).
// Not the f32 instructions: an f32 chain over j rounds relative to sum_j |M_ij| |b_j|, and what the caller keeps of the result
// can be far below that.
// The left operand M comes from a matrix G of floats: MM_DIRECT G[i][j] (G is [R][J]); MM_TRANS G[j][i] (G is [J][R]); MM_SYM
// G[i][j] + G[j][i] (R = J), formed in f64 while the operand is read; SCALE: times qv[j], an exact f64 product.
// An Out says how a result leaves:
//   static constexpr bool ROW_SUM;                             whether put() wants s_i = sum_j M(i, j)
//   __device__ double begin() const;                           read once per thread, after the products
//   __device__ void put(double begun, long at, double y, double s) const;     element at = i * e + col from the f64 sum y and s_i
using f64x4 = __attribute__((ext_vector_type(4))) double;
enum { MM_DIRECT, MM_TRANS, MM_SYM };

template <int LEFT, bool SCALE, class Out>
__device__ __forceinline__ void mm_f64_tile(const float* __restrict__ G, const float* __restrict__ qv, const float* __restrict__ B,
                                            int R, int J, int e, int jb, int je, const Out& out) {
  // (an array no instantiated branch below touches gets no LDS: 12 672 B with wb, 8 576 B with qs, 8 448 B with neither)
  __shared__ float wa[32][33];                           // M's first term, [ii][jj]
  __shared__ float wb[32][33];                           // MM_SYM: G[j0 + jj][i0 + ii], stored [jj][ii]
  __shared__ float xs[32][33];                           // B[j0 + jj][e0 + ee]
  __shared__ float qs[32];                               // SCALE: qv[j0 + jj]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = blockIdx.x * 32, e0 = blockIdx.y * 32;
  const int ro = 16 * (wave >> 1), co = 16 * (wave & 1);
  const int lr = lane & 15, lk = lane >> 4;
  f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  double srow = 0.0;                                     // ROW_SUM: sum of this lane's M(ro + lr, k) operands
  for (int j0 = jb; j0 < je; j0 += 32) {
    for (int t = tid; t < 1024; t += 256) {
      const int r = t >> 5, cc = t & 31;
      const int i = i0 + r, j = j0 + cc, jr = j0 + r, ic = i0 + cc, ec = e0 + cc;
      if constexpr (LEFT == MM_TRANS) wa[cc][r] = (ic < R && jr < J) ? G[(long)jr * R + ic] : 0.f;
      else wa[r][cc] = (i < R && j < J) ? G[(long)i * J + j] : 0.f;
      if constexpr (LEFT == MM_SYM) wb[r][cc] = (jr < J && ic < R) ? G[(long)jr * R + ic] : 0.f;
      xs[r][cc] = (jr < J && ec < e) ? B[(long)jr * e + ec] : 0.f;
    }
    if constexpr (SCALE) {
      if (tid < 32) qs[tid] = j0 + tid < J ? qv[j0 + tid] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) {
      const int kx = 4 * kk + lk;
      double av = (double)wa[ro + lr][kx];
      if constexpr (LEFT == MM_SYM) av += (double)wb[kx][ro + lr];
      if constexpr (SCALE) av *= (double)qs[kx];
      const double bv = (double)xs[kx][co + lr];
      if constexpr (Out::ROW_SUM) srow += av;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
    }
    __syncthreads();
  }
  if constexpr (Out::ROW_SUM) {
    srow += __shfl_xor(srow, 16, 64);                    // the four k-lanes of row lr: s_i
    srow += __shfl_xor(srow, 32, 64);
  }
  const double begun = out.begin();
  const int col = e0 + co + lr;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int rl = lk + 4 * r;
    double s = 0.0;
    if constexpr (Out::ROW_SUM) s = __shfl(srow, rl, 64);                // lane rl holds s of row rl
    const int row = i0 + ro + rl;
    if (row < R && col < e) out.put(begun, (long)row * e + col, acc[r], s);
  }
}

// ---- backward: Y = (M + M^T) X, demb = Epilogue(Y), M the pair weights [n][n] ----------------------------------------------
// The result carries one fp32 rounding of an f64 sum.  An Epilogue is built by the kernel from its arguments and has
//   static constexpr bool ROW_SUM;                             whether value() wants s_i = sum_j (M + M^T)_ij
//   __device__ double scale(int n) const;                      read once per thread, after the products
//   __device__ double value(double scale, double y, double s, const float* x) const;     demb[i][c] from Y_ic, s_i, &X[i][c]
template <class Epilogue>
struct PairBwdOut {
  static constexpr bool ROW_SUM = Epilogue::ROW_SUM;
  const Epilogue& ep; const float* emb; int n; float* demb;
  __device__ double begin() const { return ep.scale(n); }
  __device__ void put(double scale, long at, double y, double s) const { demb[at] = (float)ep.value(scale, y, s, emb + at); }
};

template <class Epilogue>
__device__ __forceinline__ void pair_bwd(const float* __restrict__ emb, int n, int e, const float* __restrict__ w,
                                         const Epilogue& ep, float* __restrict__ demb) {
  mm_f64_tile<MM_SYM, false>(w, nullptr, emb, n, n, e, 0, n, PairBwdOut<Epilogue>{ep, emb, n, demb});
}

// ---- host side: range, fit rule, workspace layout, argument checks, launches ----------------------------------------------
inline bool pair_class_path_fits(int p, int k, int e) {
  const long n = (long)p * k;
  return k <= PAIR_CLASS_MAX_K && n <= PAIR_CLASS_MAX_N && (long)k * (e + n) <= PAIR_LDS_FLOATS;
}

inline size_t pair_align16(size_t b) { return (b + 15) / 16 * 16; }

inline bool pair_range_ok(int p, int k, int e) {
  return p >= 2 && k >= 2 && e >= 1 && e <= PAIR_MAX_E && (long long)p * k <= PAIR_MAX_N;
}

inline int pair_path(int p, int k, int e) {              // the path `auto` takes; 0 outside the range
  if (!pair_range_ok(p, k, e)) return 0;
  return pair_class_path_fits(p, k, e) ? PAIR_PER_CLASS : PAIR_MATRIX;
}

// workspace: [16 B ticket][n f64 partial losses][n int4 partial counts][n*n f32 pair matrix][Body::matrix's own workspace]
// (sized for both forward paths, so a caller may force either); 0 outside the range
template <class Body>
inline size_t pair_workspace_bytes(int p, int k, int e) {
  if (!pair_range_ok(p, k, e)) return 0;
  const size_t n = (size_t)p * k;
  return 16 + pair_align16(n * 8) + n * 16 + pair_align16(n * n * 4) + pair_align16(Body::matrix_extra_bytes((int)n, e));
}

// The argument checks the losses share.  `what` is the entry point's name without `embnet_`, `pointers` whether all are set,
// `need` the loss's own workspace size.
inline int pair_check_common(const char* what, bool pointers, int p, int k, int e) {
  EMBNET_CHECK_ARG(pointers, "%s: null pointer", what);
  EMBNET_CHECK_ARG(p >= 2 && k >= 2, "%s: need p >= 2 classes and k >= 2 samples (p=%d k=%d)", what, p, k);
  EMBNET_CHECK_ARG((long long)p * k <= PAIR_MAX_N, "%s: n = p*k = %lld > %d", what, (long long)p * k, PAIR_MAX_N);
  EMBNET_CHECK_ARG(e >= 1 && e <= PAIR_MAX_E, "%s: e=%d outside [1, %d]", what, e, PAIR_MAX_E);
  return EMBNET_OK;
}

inline int pair_check_path_and_workspace(const char* what, int p, int k, int e, int path, const void* workspace,
                                         size_t workspace_bytes, size_t need) {
  EMBNET_CHECK_ARG(path >= 0 && path <= PAIR_MATRIX, "%s: unknown path %d", what, path);
  EMBNET_CHECK_ARG(path != PAIR_PER_CLASS || pair_class_path_fits(p, k, e), "%s: p=%d k=%d e=%d does not fit the per-class path",
                   what, p, k, e);
  return check_workspace(what, workspace, workspace_bytes, need);
}

inline int pair_check_bwd(const char* what, bool pointers, int n, int e) {
  EMBNET_CHECK_ARG(pointers, "%s: null pointer", what);
  EMBNET_CHECK_ARG(n >= 4 && n <= PAIR_MAX_N, "%s: n=%d outside [4, %d]", what, n, PAIR_MAX_N);
  EMBNET_CHECK_ARG(e >= 1 && e <= PAIR_MAX_E, "%s: e=%d outside [1, %d]", what, e, PAIR_MAX_E);
  return EMBNET_OK;
}

// A loss's two forward kernels (its own __global__ wrappers) under the names its trace entries carry.
template <class Body>
struct PairKernels {
  void (*class_fwd)(PairParams<Body>); const char* class_name;
  void (*sweep)(PairParams<Body>); const char* sweep_name;
};

// The forward on checked arguments: the per-class kernel, or Body::matrix and then the sweep.
template <class Body>
inline int pair_launch(const char* what, const PairKernels<Body>& kn, const float* emb, int p, int k, int e,
                       const typename Body::Args& a, int path, float* pair_g, int32_t* counts, float* mean_loss, void* workspace,
                       void* stream) {
  const int n = p * k;
  char* ws = (char*)workspace;
  int4* part_cnt = (int4*)(ws + 16 + pair_align16((size_t)n * 8));
  float* sim = (float*)((char*)part_cnt + (size_t)n * 16);
  PairParams<Body> q{emb, n, p, k, e, a, pair_g, counts, mean_loss, (int*)ws, (double*)(ws + 16), part_cnt, sim};
  hipStream_t s = (hipStream_t)stream;
  if (path == 0) path = pair_path(p, k, e);
  if (path == PAIR_PER_CLASS) {
    const double bytes = 4.0 * n * e * (p + 1.0) + 4.0 * n * n;
    TraceScope trace(kn.class_name, Body::CLASS_TRACE_UNIT, Body::CLASS_TRACE_UNIT == TRACE_FLOP ? 2.0 * n * n * e : bytes, stream,
                     bytes);
    kn.class_fwd<<<p, PAIR_CLASS_THREADS, 0, s>>>(q);
    return check_launch(what);
  }
  const int rc = Body::matrix(emb, n, e, sim, (char*)sim + pair_align16((size_t)n * n * 4), stream);
  if (rc != EMBNET_OK) return rc;
  EMBNET_TRACE(kn.sweep_name, TRACE_BYTES, 8.0 * n * n, stream);
  kn.sweep<<<cdiv(n, PAIR_SWEEP_THREADS / 64), PAIR_SWEEP_THREADS, 0, s>>>(q);
  return check_launch(what);
}

}  // namespace embnet
