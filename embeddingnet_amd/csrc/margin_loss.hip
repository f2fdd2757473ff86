// Distance-weighted sampling and the margin loss (Wu, Manmatha, Smola, Kraehenbuehl, ICCV 2017, "Sampling Matters in Deep
// Embedding Learning") over a class-contiguous P x K batch.  Build-defined: the reference has no such loss.  Semantics, rounding
// form and summation order: include/embnet.h.
//
//   X [N, E] fp32, N = P*K, rows c*K .. c*K+K-1 are class c.  d2(i,j) = sum_c (x_ic - x_jc)^2 (batch_all.hip's pair matrix, both
//   paths), D = sqrt(d2).  Anchor i draws ONE negative for each of its K-1 positives, with replacement, from the other-class columns
//   with D < c_hi, weighted by the inverse of the density of pairwise distances on the unit sphere S^(E-1):
//     lw = (2 - E) log D~ - ((E - 3) / 2) log(1 - D~^2 / 4),  D~ = max(D, c_lo);   w = e^{lw - max lw}  (the largest weight is 1)
//   and pays two hinges around the boundary beta:  l+ = [D_ip - beta + alpha]+,  l- = [beta - D_in + alpha]+.
//   loss = (sum l+ + sum l-) / max(A, 1),  A = the number of positive hinges (a draw counts each time it is drawn).
//   W[i,p] = [l+ > 0] / D_ip,  W[i,n] = -#{active draws of i that picked n} / D_in,  0 elsewhere and wherever D = 0.
//   backward, A held constant:  demb_i = (g / max(A,1)) sum_j (W_ij + W_ji) (x_i - x_j) = (g / max(A,1)) (s_i x_i - (M X)_i).
//
// One wave per anchor on pair_loss.h's skeleton, its row of d2 in LDS, no LDS of its own.  The weights are recomputed wherever they
// are needed (three passes of logf / expf over the row: the maximum, the total, the draws) and nothing is parked.  The sampler walks
// the row in chunks of 64 columns: a wave inclusive scan of the chunk's weights in f64 plus a running carry gives every column its
// prefix sum, and the wave's draws (lane l holds draw 64 b + l) are compared against the chunk one after the other, so a chunk is
// scanned once for 64 draws.  The picks leave through `triplets`; the last pass counts them per column from there (behind a
// workgroup-scope fence: the rows were written by other lanes of the same wave).  Nothing is atomic in floating point, every
// reduction has a fixed order: the same seed gives the same bits.  No host synchronisation, no allocation: capturable in a graph.
#include <math.h>
#include "common.h"
#include "pair_loss.h"
#include "../../include/embnet.h"

namespace embnet {

static_assert(EMBNET_MARGIN_PER_CLASS == PAIR_PER_CLASS && EMBNET_MARGIN_DISTANCE_MATRIX == PAIR_MATRIX, "path constants");

struct MarginArgs {
  float beta, alpha, c_lo, c_hi, a1, a2;                 // a1 = 2 - E, a2 = (E - 3) / 2: exact in fp32 up to E = 4096
  uint64_t seed; const uint64_t* seed_dev;
  int32_t* triplets; float* sample_w;
  const float* norms;                                    // matrix path: |x_j|^2 as embnet_pairwise_dist_f32 left them; else NULL
};

// one rounding form everywhere (include/embnet.h)
__device__ __forceinline__ float margin_log_weight(float d, const MarginArgs& a) {
  const float dt = fmaxf(d, a.c_lo);
  const float t = __fsub_rn(1.f, __fmul_rn(0.25f, __fmul_rn(dt, dt)));
  return __fsub_rn(__fmul_rn(a.a1, logf(dt)), __fmul_rn(a.a2, logf(t)));
}
__device__ __forceinline__ float margin_hinge_pos(float d, const MarginArgs& a) {
  return fmaxf(__fadd_rn(__fsub_rn(d, a.beta), a.alpha), 0.f);
}
__device__ __forceinline__ float margin_hinge_neg(float d, const MarginArgs& a) {
  return fmaxf(__fadd_rn(__fsub_rn(a.beta, d), a.alpha), 0.f);
}

// A wave's inclusive scan in lane order: steps 1, 2, 4, .. 32, lane l adds the value l - step lanes below it.
__device__ __forceinline__ double wave_inclusive_scan(double v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double up = __shfl_up(v, o, 64);
    if (lane >= o) v += up;
  }
  return v;
}
__device__ __forceinline__ int wave_max_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// The anchor's view of its row: distances, and the sampling weights once the largest log-weight is known.
struct MarginRow {
  const float* d2; const float* norms; int lo, hi; bool anchor_bad; float big;
  // D = sqrt(max(d2, 0)) with a NaN kept.  The Gram form's clamp turns the NaN of a non-finite row into 0, so on the matrix path a
  // column (or an anchor) whose squared norm is not finite has D = NaN, as the difference form gives it.
  __device__ float dist(int col) const {
    float v = d2[col];
    if (norms && (anchor_bad || !(norms[col] < INFINITY))) v = NAN;
    return sqrtf(v < 0.f ? 0.f : v);
  }
  __device__ float weight(int col, const MarginArgs& a) const {        // 0 on own-class and ineligible columns
    if (col >= lo && col < hi) return 0.f;
    const float d = dist(col);
    return d < a.c_hi ? expf(__fsub_rn(margin_log_weight(d, a), big)) : 0.f;
  }
};

// Counts: c+ <= N (K-1) and c- <= N (K-1), N (K-1) <= 4096 * 2047 < 2^23, so both, their sum A and every partial fit an int.
struct MarginBody {
  using Args = MarginArgs;
  using Sum = double;
  static constexpr int CLASS_TRACE_UNIT = TRACE_BYTES;

  static __device__ float term(float a, float y, float acc) { const float d = a - y; return fmaf(d, d, acc); }   // difference form
  static int matrix(const float* emb, int n, int e, float* dist, void* extra, void* stream) {
    return embnet_pairwise_dist_f32(emb, n, e, dist, 1, extra, pair_align16(embnet_pairwise_workspace_bytes(n, e)), stream);
  }
  static size_t matrix_extra_bytes(int n, int e) { return embnet_pairwise_workspace_bytes(n, e); }

  static __device__ PairAnchorOut<double> anchor(const float* drow, int n, int k, int lo, int ai, const Args& a, float* wrow,
                                                 int lane) {
    const int hi = lo + k, self = lo + ai, km1 = k - 1;
    MarginRow row{drow, a.norms, lo, hi, a.norms && !(a.norms[self] < INFINITY), 0.f};
    float big = -INFINITY;                                 // pass 1: the largest log-weight over the eligible columns
    for (int col = lane; col < n; col += 64) {
      if (col >= lo && col < hi) continue;
      const float d = row.dist(col);
      if (d < a.c_hi) big = fmaxf(big, margin_log_weight(d, a));
    }
    row.big = big = wave_max(big);
    const bool any = big > -INFINITY;                      // wave-uniform; false: a fall-back anchor, every weight is 0
    float* sw = a.sample_w ? a.sample_w + (long)self * n : nullptr;
    double total = 0.0;                                    // pass 2: the total, in the sampler's own order; sample_w
    int lastpos = -1;
    for (int c0 = 0; c0 < n; c0 += 64) {
      const int col = c0 + lane;
      const float w = col < n ? row.weight(col, a) : 0.f;
      if (sw && col < n) sw[col] = w;
      if (w > 0.f) lastpos = col;
      total += __shfl(wave_inclusive_scan((double)w, lane), 63, 64);
    }
    lastpos = wave_max_int(lastpos);
    const uint64_t seed = a.seed_dev ? *a.seed_dev : a.seed;
    int32_t* trip = a.triplets + (long)self * km1 * 3;
    double s = 0.0;
    int cp = 0, cn = 0;
    for (int j0 = 0; j0 < km1; j0 += 64) {                 // 64 draws at a time, draw j0 + l in lane l
      const int j = j0 + lane, live = min(64, km1 - j0);
      const uint64_t bits = ((uint64_t)rng_u32(seed, (uint64_t)self, 2ull * j) << 32) | rng_u32(seed, (uint64_t)self, 2ull * j + 1);
      const double u = (double)(bits >> 11) * 0x1p-53;
      int pick = -1;
      if (any) {                                           // pass 3: the prefix sums against the block's targets
        const double target = u * total;
        double carry = 0.0;
        for (int c0 = 0; c0 < n; c0 += 64) {
          const int col = c0 + lane;
          const float w = col < n ? row.weight(col, a) : 0.f;
          const double incl = wave_inclusive_scan((double)w, lane);
          const double prefix = carry + incl;
          carry += __shfl(incl, 63, 64);
          for (int jj = 0; jj < live; ++jj) {
            const double tj = __shfl(target, jj, 64);      // by every lane, outside the condition: a && would mask the source lane
            const unsigned long long over = __ballot(w > 0.f && prefix > tj);
            if (lane == jj && pick < 0 && over) pick = c0 + __ffsll((long long)over) - 1;
          }
        }
        if (pick < 0) pick = lastpos;                      // rounding left no prefix above u * total: the last positive weight
      } else {
        const int idx = (int)(u * (double)(n - k));        // the idx-th other-class column
        pick = idx < lo ? idx : idx + k;
      }
      pick = min(max(pick, 0), n - 1);
      if (j < km1) {
        const int pcol = lo + (j < ai ? j : j + 1);
        const float lp = margin_hinge_pos(row.dist(pcol), a), ln = margin_hinge_neg(row.dist(pick), a);
        s += (double)lp;
        s += (double)ln;
        cp += lp > 0.f;
        cn += ln > 0.f;
        trip[3 * j] = self; trip[3 * j + 1] = pcol; trip[3 * j + 2] = pick;
      }
    }
    __threadfence_block();                                 // the picks, written lane by lane, are read back by every lane
    for (int col = lane; col < n; col += 64) {             // pass 4: the anchor's row of W
      float wv = 0.f;
      if (col != self) {
        const float d = row.dist(col);
        if (col >= lo && col < hi) {
          if (margin_hinge_pos(d, a) > 0.f && d > 0.f) wv = __fdiv_rn(1.f, d);
        } else {
          int c = 0;
          for (int j = 0; j < km1; ++j) c += trip[3 * j + 2] == col;
          if (c > 0 && margin_hinge_neg(d, a) > 0.f && d > 0.f) wv = -__fdiv_rn((float)c, d);
        }
      }
      wrow[col] = wv;
    }
    const double sum = wave_sum(s);
    return PairAnchorOut<double>{sum, wave_sum(cp), wave_sum(cn)};
  }
  static __device__ int third(const PairAnchorOut<double>& o) { return o.c0 + o.c1; }
  static __device__ void finish(const PairParams<MarginBody>& q, double total, int cp, int cn, int active) {
    q.counts[0] = cp;
    q.counts[1] = cn;
    q.counts[2] = active;
    *q.mean = (float)(total / (double)(active > 0 ? active : 1));
  }
};
using MarginParams = PairParams<MarginBody>;

__global__ __launch_bounds__(PAIR_CLASS_THREADS) void margin_class_fwd_kernel(MarginParams q) { pair_class_fwd<MarginBody>(q); }
__global__ __launch_bounds__(PAIR_SWEEP_THREADS) void margin_sweep_kernel(MarginParams q) { pair_sweep_fwd<MarginBody>(q); }

// ---- backward: demb = (g / max(A,1)) (s x - M X), M = W + W^T; every f64 product of an fp32 weight and an fp32 x is exact ----
struct MarginEpilogue {
  static constexpr bool ROW_SUM = true;
  const int32_t* counts; const float* upstream;
  __device__ double scale(int) const {
    const int cnt = counts[2];
    const double g = upstream ? (double)*upstream : 1.0;
    return g / (double)(cnt > 0 ? cnt : 1);
  }
  __device__ double value(double scale, double y, double s, const float* x) const { return scale * (s * (double)*x - y); }
};

__global__ __launch_bounds__(256) void margin_bwd_kernel(const float* __restrict__ emb, int n, int e, const float* __restrict__ w,
                                                        const int32_t* __restrict__ counts, const float* __restrict__ upstream,
                                                        float* __restrict__ demb) {
  pair_bwd(emb, n, e, w, MarginEpilogue{counts, upstream}, demb);
}

}  // namespace embnet

using namespace embnet;

// workspace: pair_loss.h's layout, the squared distances as the pair matrix, embnet_pairwise_dist_f32's workspace behind them
extern "C" size_t embnet_margin_loss_workspace_bytes(int p, int k, int e) { return pair_workspace_bytes<MarginBody>(p, k, e); }

extern "C" int embnet_margin_loss_path(int p, int k, int e) { return pair_path(p, k, e); }

extern "C" int embnet_margin_loss_fwd(const float* emb, int p, int k, int e, float beta, float alpha, float cutoff,
                                      float nonzero_loss_cutoff, uint64_t seed, const uint64_t* seed_dev, int path, float* pair_w,
                                      int32_t* counts, int32_t* triplets, float* sample_w, float* mean_loss, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  int rc = pair_check_common("margin_loss_fwd", emb && pair_w && counts && triplets && mean_loss && workspace, p, k, e);
  if (rc != EMBNET_OK) return rc;
  EMBNET_CHECK_ARG(isfinite(beta), "margin_loss_fwd: beta=%g must be finite", (double)beta);
  EMBNET_CHECK_ARG(isfinite(alpha) && alpha >= 0.f, "margin_loss_fwd: alpha=%g must be finite and >= 0", (double)alpha);
  EMBNET_CHECK_ARG(isfinite(cutoff) && isfinite(nonzero_loss_cutoff) && 0.f < cutoff && cutoff < nonzero_loss_cutoff &&
                       nonzero_loss_cutoff < 2.f,
                   "margin_loss_fwd: need 0 < cutoff < nonzero_loss_cutoff < 2 (cutoff=%g nonzero_loss_cutoff=%g)", (double)cutoff,
                   (double)nonzero_loss_cutoff);
  rc = pair_check_path_and_workspace("margin_loss_fwd", p, k, e, path, workspace, workspace_bytes,
                                     embnet_margin_loss_workspace_bytes(p, k, e));
  if (rc != EMBNET_OK) return rc;
  const size_t n = (size_t)p * k;
  const bool per_class = (path == 0 ? pair_path(p, k, e) : path) == PAIR_PER_CLASS;
  // pair_launch's layout: the pair matrix behind the partials, embnet_pairwise_dist_f32's workspace (the row norms first) behind it
  const float* norms = (const float*)((char*)workspace + 16 + pair_align16(n * 8) + n * 16 + pair_align16(n * n * 4));
  static const PairKernels<MarginBody> kernels{margin_class_fwd_kernel, "embnet::margin_class_fwd_kernel", margin_sweep_kernel,
                                               "embnet::margin_sweep_kernel"};
  const MarginArgs a{beta, alpha, cutoff, nonzero_loss_cutoff, (float)(2 - e), 0.5f * (float)(e - 3), seed, seed_dev, triplets, sample_w,
                     per_class ? nullptr : norms};
  return pair_launch<MarginBody>("margin_loss_fwd", kernels, emb, p, k, e, a, path, pair_w, counts, mean_loss, workspace, stream);
}

extern "C" int embnet_margin_loss_bwd(const float* emb, int n, int e, const float* pair_w, const int32_t* counts,
                                      const float* upstream, float* demb, void* stream) {
  const int rc = pair_check_bwd("margin_loss_bwd", emb && pair_w && counts && demb, n, e);
  if (rc != EMBNET_OK) return rc;
  EMBNET_TRACE_FLOP("embnet::margin_bwd_kernel", 2.0 * n * n * e, 4.0 * (2.0 * n * n + 2.0 * n * e), stream);
  margin_bwd_kernel<<<dim3(cdiv(n, 32), cdiv(e, 32)), 256, 0, (hipStream_t)stream>>>(emb, n, e, pair_w, counts, upstream, demb);
  return check_launch("margin_loss_bwd");
}
