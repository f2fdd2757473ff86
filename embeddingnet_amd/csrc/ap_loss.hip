// FastAP and Smooth-AP: the ranking family of losses (smooth surrogates of average precision over each anchor's ranked list) over a
// class-contiguous P x K batch.  Build-defined: the reference has no pair-based loss.  Semantics: include/embnet.h.
//
//   X [N, E] fp32, N = P*K, rows c*K .. c*K+K-1 are class c.  S = X X^T.  Anchor i: positives P_i = the other rows of its class,
//   negatives N_i = the rows of other classes.
//   FastAP (Cakir et al., CVPR 2019), bins = L in [2, 64]: the distances d = 2 - 2 S of the anchor's pairs are soft-binned into
//     histograms h+ / h- over the L + 1 centres l * 4 / L with the triangular pulse; ONE rounding form: inv = L / 4 (exact),
//     u = fl(fl(2 - 2 S) inv), l0 = floor(u), f = u - l0 (exact): fl(1 - f) goes to bin l0 and f to bin l0 + 1, a bin outside 0 .. L
//     is dropped.  Hp, Hn: the running sums of h+, h- from bin 0 up, H = fl(Hp + Hn);
//     F = sum_{l: H_l > 0} h+_l Hp_l / H_l,  l_i = 1 - F / (K-1);
//     b_l = h+_l Hp_l / H_l^2, c_l = h+_l Hn_l / H_l^2 (= a_l - b_l of the header, formed without the subtraction),
//     A-_m = -sum_{l >= m} b_l,  A+_m = Hp_m / H_m + sum_{l >= m} c_l,  G_ij = (2 inv / (K-1)) (A_{l0+1} - A_{l0}).
//   Smooth-AP (Brown et al., ECCV 2020), temperature tau, r = fl(1 / tau) taken once on the host: per positive p and column
//     j not in {i, p}: z = fl(fl(S_ij - S_ip) r), t = e^{-|z|}, s = sigma(z) = 1 / (1 + t) or t / (1 + t), s' = r t / (1 + t)^2;
//     R_p = 1 + sum over the other positives of s, Nn_p = the sum of s over the negatives, Q_p = R_p + Nn_p, U_p / Tn_p the same
//     two sums of s';  l_i = 1 - (1/(K-1)) sum_p R_p / Q_p;
//     G_ij = (1/(K-1)) [ sum_{p != j} s'_pj (j in P_i ? -Nn_p / Q_p^2 : R_p / Q_p^2) + [j in P_i] (U_j Nn_j - R_j Tn_j) / Q_j^2 ]
//     (the header's R/Q^2 - 1/Q and U/Q - R T/Q^2 with Q = R + Nn, T = U + Tn put in: nothing of the size of 1 cancels).
//   loss = (1/N) sum_i l_i;  backward demb_i = (g / N) sum_j (G_ij + G_ji) x_j: embnet_ms_loss_bwd's contract, and its kernel.
//   counts = {positive pairs N (K-1), violating anchors: max_n S_in >= min_p S_ip on the fp32 S}, exact.
//
// The forward is pair_loss.h's skeleton (per-class path, similarity-matrix path, ticket, fixed-order reduction, launch) around the
// two per-anchor bodies below.  Nothing is atomic in floating point, every sum has a fixed order: bitwise reproducible.  No host
// synchronisation, no allocation: capturable in a graph.
#include <math.h>
#include "common.h"
#include "pair_loss.h"
#include "../../include/embnet.h"

namespace embnet {

static_assert(EMBNET_AP_PER_CLASS == PAIR_PER_CLASS && EMBNET_AP_SIMILARITY_MATRIX == PAIR_MATRIX, "path constants");

constexpr int FAST_AP_MAX_BINS = 64;
constexpr int SMOOTH_AP_MAX_K = 65;                      // K - 1 positives, one per lane

// SupCon's counter: whether the hardest negative is at least as similar as the hardest positive.  The same in every lane.
__device__ __forceinline__ int ap_violating(const float* srow, int n, int k, int lo, int ai, int lane) {
  float mn = INFINITY, mx = -INFINITY;
  for (int j = lane; j < k; j += 64)
    if (j != ai) mn = fminf(mn, srow[lo + j]);
  for (int col = lane; col < n; col += 64)
    if (col < lo || col >= lo + k) mx = fmaxf(mx, srow[col]);
  return wave_max(mx) >= wave_min(mn);
}

// v of lane `src`, a wave-uniform index, in every lane
__device__ __forceinline__ float lane_value(float v, int src) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src));
}

template <class Body>
__device__ __forceinline__ void ap_finish(const PairParams<Body>& q, double total, int c0) {
  q.counts[0] = q.n * (q.k - 1);                         // <= 4096 * 2047 < 2^23
  q.counts[1] = c0;
  *q.mean = (float)(total / (double)q.n);
}

// ---- FastAP ---------------------------------------------------------------------------------------------------------------------
// Lane l owns the bins l and l + 64 (the second is bin 64 in lane 0 when L = 64, nothing otherwise).  Histogram: EVERY lane walks
// all N columns in column order (their positions computed 64 at a time, one per lane, and read from the lanes) and keeps what falls
// into its bins: a chain of N terms per bin, no reduction across lanes.  Running sums and suffix sums: serial over the bins, the
// bin's value broadcast from its lane, so every lane forms the same chain and the bin's lane keeps it.  The last pass looks A up
// by a lane-indexed shuffle.
struct FastApBody : PairDotBody {
  struct Args { float inv; int bins; };                  // L / 4, L
  using Sum = float;

  static __device__ __forceinline__ float position(float s, float inv, float& f) {      // -> l0; f = u - l0
    const float u = __fmul_rn(__fsub_rn(2.f, __fmul_rn(2.f, s)), inv);
    const float l0 = floorf(u);
    f = __fsub_rn(u, l0);
    return l0;
  }

  static __device__ PairAnchorOut<float> anchor(const float* srow, int n, int k, int lo, int ai, const Args& a, float* grow, int lane) {
    const float inv = a.inv;
    const int L = a.bins, self = lo + ai;
    const float kf = (float)(k - 1);
    const int viol = ap_violating(srow, n, k, lo, ai, lane);
    const float bin0 = (float)lane, bin1 = (float)(lane + 64);
    float hp0 = 0.f, hp1 = 0.f, hn0 = 0.f, hn1 = 0.f;
    const bool wide = L == 64;                           // bin 64 exists
    for (int c = 0; c < n; c += 64) {                    // wave-uniform: 64 columns' positions at a time, one per lane ...
      float fl;
      const float l0l = position(srow[c + lane < n ? c + lane : 0], inv, fl);
      const int m = min(64, n - c);
      for (int j = 0; j < m; ++j) {                      // ... then every lane takes every column, in column order
        const int col = c + j;
        if (col == self) continue;
        const float l0 = lane_value(l0l, j), f = lane_value(fl, j), l1 = l0 + 1.f;
        const float g = __fsub_rn(1.f, f);
        const float w0 = l0 == bin0 ? g : (l1 == bin0 ? f : 0.f);
        const bool pos = col >= lo && col < lo + k;
        if (pos) hp0 += w0; else hn0 += w0;
        if (wide) {
          const float w1 = l0 == bin1 ? g : (l1 == bin1 ? f : 0.f);
          if (pos) hp1 += w1; else hn1 += w1;
        }
      }
    }
    if (lane > L) hp0 = hn0 = 0.f;                       // a bin above L is dropped
    if (lane + 64 > L) hp1 = hn1 = 0.f;
    float Hp0 = 0.f, Hp1 = 0.f, Hn0 = 0.f, Hn1 = 0.f;
    {
      float cp = 0.f, cn = 0.f;
      for (int m = 0; m <= L; ++m) {                     // running sums from bin 0 up
        const int src = m & 63;
        cp += __shfl(m < 64 ? hp0 : hp1, src, 64);
        cn += __shfl(m < 64 ? hn0 : hn1, src, 64);
        if (lane == src) {
          if (m < 64) { Hp0 = cp; Hn0 = cn; } else { Hp1 = cp; Hn1 = cn; }
        }
      }
    }
    // per bin: rp = Hp / H, b = (h+ / H) rp, c = (h+ / H)(Hn / H), the bin's term of F = h+ rp; all 0 where H = 0 (every bin
    // below the smallest distance) and in the bins nobody owns
    float rp0, b0, c0, f0, rp1, b1, c1, f1;
    {
      const float H0 = __fadd_rn(Hp0, Hn0), H1 = __fadd_rn(Hp1, Hn1);
      const bool ok0 = H0 > 0.f, ok1 = H1 > 0.f;
      const float d0 = ok0 ? H0 : 1.f, d1 = ok1 ? H1 : 1.f;
      const float a0 = ok0 ? __fdiv_rn(hp0, d0) : 0.f, a1 = ok1 ? __fdiv_rn(hp1, d1) : 0.f;
      rp0 = ok0 ? __fdiv_rn(Hp0, d0) : 0.f;
      rp1 = ok1 ? __fdiv_rn(Hp1, d1) : 0.f;
      b0 = __fmul_rn(a0, rp0);
      b1 = __fmul_rn(a1, rp1);
      c0 = __fmul_rn(a0, ok0 ? __fdiv_rn(Hn0, d0) : 0.f);
      c1 = __fmul_rn(a1, ok1 ? __fdiv_rn(Hn1, d1) : 0.f);
      f0 = __fmul_rn(hp0, rp0);
      f1 = __fmul_rn(hp1, rp1);
    }
    float Ap0 = 0.f, Ap1 = 0.f, An0 = 0.f, An1 = 0.f;
    {
      float sb = 0.f, sc = 0.f;
      for (int m = L; m >= 0; --m) {                     // suffix sums from bin L down
        const int src = m & 63;
        sb += __shfl(m < 64 ? b0 : b1, src, 64);
        sc += __shfl(m < 64 ? c0 : c1, src, 64);
        if (lane == src) {
          if (m < 64) { An0 = -sb; Ap0 = __fadd_rn(rp0, sc); } else { An1 = -sb; Ap1 = __fadd_rn(rp1, sc); }
        }
      }
    }
    const float F = wave_sum(__fadd_rn(f0, f1));
    const float Ap64 = __shfl(Ap1, 0, 64), An64 = __shfl(An1, 0, 64);
    const float coef = __fdiv_rn(__fmul_rn(2.f, inv), kf);
    for (int c = 0; c < n; c += 64) {                    // wave-uniform trip count: every lane takes part in the shuffles
      const int col = c + lane;
      const bool in = col < n;
      float f;
      const float l0 = position(srow[in ? col : 0], inv, f);
      const int i0 = (int)fminf(fmaxf(l0, -2.f), 66.f), i1 = i0 + 1;     // beyond [-1, L]: both look-ups give 0
      const bool pos = col >= lo && col < lo + k;
      const float p0 = __shfl(Ap0, i0 & 63, 64), n0 = __shfl(An0, i0 & 63, 64);
      const float p1 = __shfl(Ap0, i1 & 63, 64), n1 = __shfl(An0, i1 & 63, 64);
      float v0 = i0 == 64 ? (pos ? Ap64 : An64) : (pos ? p0 : n0);
      float v1 = i1 == 64 ? (pos ? Ap64 : An64) : (pos ? p1 : n1);
      if (i0 < 0 || i0 > L) v0 = 0.f;
      if (i1 < 0 || i1 > L) v1 = 0.f;
      if (in) grow[col] = col == self ? 0.f : __fmul_rn(coef, __fsub_rn(v1, v0));
    }
    return PairAnchorOut<float>{__fsub_rn(1.f, __fdiv_rn(F, kf)), viol, 0};
  }
  static __device__ int third(const PairAnchorOut<float>&) { return 0; }
  static __device__ void finish(const PairParams<FastApBody>& q, double total, int c0, int, int) { ap_finish(q, total, c0); }
};

// ---- Smooth-AP ------------------------------------------------------------------------------------------------------------------
// The K - 1 <= 64 positives sit one per lane: lane l is class member l + (l >= ai).  A lane-strided pass over the row per positive
// gives its four sums (wave sums; the positive's lane keeps them), then a lane-strided pass over the columns, each column a chain
// over the positives with their weights broadcast from their lanes.
struct SmoothApBody : PairDotBody {
  struct Args { float r; };                              // fl(1 / tau)
  using Sum = float;

  // sigma(z) and sigma'(z) / tau of z = fl(fl(s - sp) r), without the subtraction 1 - sigma
  static __device__ __forceinline__ void sigmoid(float s, float sp, float r, float& sg, float& dsg) {
    const float z = __fmul_rn(__fsub_rn(s, sp), r);
    const float t = expf(-fabsf(z));
    const float iv = __fdiv_rn(1.f, __fadd_rn(1.f, t));
    const float w = __fmul_rn(t, iv);
    sg = z >= 0.f ? iv : w;
    dsg = __fmul_rn(__fmul_rn(r, w), iv);
  }

  static __device__ PairAnchorOut<float> anchor(const float* srow, int n, int k, int lo, int ai, const Args& a, float* grow, int lane) {
    const float r = a.r;
    const int np = k - 1, self = lo + ai;
    const float kf = (float)np;
    const int viol = ap_violating(srow, n, k, lo, ai, lane);
    float R = 1.f, Nn = 0.f, U = 0.f, Tn = 0.f;          // lane p's sums; the lanes past the positives keep Q = 1 and weights 0
    for (int lp = 0; lp < np; ++lp) {
      const int jp = lo + lp + (lp >= ai);
      const float sp = srow[jp];
      float aR = 0.f, aN = 0.f, aU = 0.f, aT = 0.f;
      for (int col = lane; col < n; col += 64) {         // lane-strided, column order
        if (col == self || col == jp) continue;
        float sg, dsg;
        sigmoid(srow[col], sp, r, sg, dsg);
        if (col >= lo && col < lo + k) { aR += sg; aU += dsg; } else { aN += sg; aT += dsg; }
      }
      aR = wave_sum(aR);
      aN = wave_sum(aN);
      aU = wave_sum(aU);
      aT = wave_sum(aT);
      if (lane == lp) { R = __fadd_rn(1.f, aR); Nn = aN; U = aU; Tn = aT; }
    }
    const bool mine = lane < np;
    const float iq = __fdiv_rn(1.f, __fadd_rn(R, Nn));   // Q >= 1
    const float rq = mine ? __fmul_rn(R, iq) : 0.f;      // R / Q
    const float wneg = __fmul_rn(rq, iq);                // R / Q^2: a negative column's weight of s'_p
    const float wpos = -__fmul_rn(__fmul_rn(Nn, iq), iq);                // R / Q^2 - 1 / Q = -Nn / Q^2: a positive column's
    const float own = mine ? __fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(U, Nn), __fmul_rn(R, Tn)), iq), iq) : 0.f;
    const float ap = wave_sum(rq);
    for (int c = 0; c < n; c += 64) {                    // wave-uniform trip count: every lane takes part in the shuffles
      const int col = c + lane;
      const bool in = col < n;
      const float sc = srow[in ? col : 0];
      const bool pos = col >= lo && col < lo + k && col != self;
      float acc = 0.f;
      for (int lp = 0; lp < np; ++lp) {
        const int jp = lo + lp + (lp >= ai);
        const float sp = srow[jp];
        const float wn = __shfl(wneg, lp, 64), wp = __shfl(wpos, lp, 64);
        float sg, dsg;
        sigmoid(sc, sp, r, sg, dsg);
        if (col != jp) acc = fmaf(dsg, pos ? wp : wn, acc);
      }
      const int member = col - lo;                       // a positive column's lane: member - (member > ai)
      const float mine_own = __shfl(own, pos ? member - (member > ai) : 0, 64);
      if (pos) acc = __fadd_rn(acc, mine_own);
      if (in) grow[col] = col == self ? 0.f : __fdiv_rn(acc, kf);
    }
    return PairAnchorOut<float>{__fsub_rn(1.f, __fdiv_rn(ap, kf)), viol, 0};
  }
  static __device__ int third(const PairAnchorOut<float>&) { return 0; }
  static __device__ void finish(const PairParams<SmoothApBody>& q, double total, int c0, int, int) { ap_finish(q, total, c0); }
};

__global__ __launch_bounds__(PAIR_CLASS_THREADS) void fast_ap_class_fwd_kernel(PairParams<FastApBody> q) { pair_class_fwd<FastApBody>(q); }
__global__ __launch_bounds__(PAIR_SWEEP_THREADS) void fast_ap_sweep_kernel(PairParams<FastApBody> q) { pair_sweep_fwd<FastApBody>(q); }
__global__ __launch_bounds__(PAIR_CLASS_THREADS) void smooth_ap_class_fwd_kernel(PairParams<SmoothApBody> q) {
  pair_class_fwd<SmoothApBody>(q);
}
__global__ __launch_bounds__(PAIR_SWEEP_THREADS) void smooth_ap_sweep_kernel(PairParams<SmoothApBody> q) { pair_sweep_fwd<SmoothApBody>(q); }

static const PairKernels<FastApBody> fast_ap_kernels{fast_ap_class_fwd_kernel, "embnet::fast_ap_class_fwd_kernel",
                                                     fast_ap_sweep_kernel, "embnet::fast_ap_sweep_kernel"};
static const PairKernels<SmoothApBody> smooth_ap_kernels{smooth_ap_class_fwd_kernel, "embnet::smooth_ap_class_fwd_kernel",
                                                         smooth_ap_sweep_kernel, "embnet::smooth_ap_sweep_kernel"};

}  // namespace embnet

using namespace embnet;

extern "C" size_t embnet_fast_ap_loss_workspace_bytes(int p, int k, int e) { return pair_workspace_bytes<FastApBody>(p, k, e); }

extern "C" int embnet_fast_ap_loss_path(int p, int k, int e) { return pair_path(p, k, e); }

extern "C" int embnet_fast_ap_loss_fwd(const float* emb, int p, int k, int e, int bins, int path, float* pair_g, int32_t* counts,
                                       float* mean_loss, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = pair_check_common("fast_ap_loss_fwd", emb && pair_g && counts && mean_loss && workspace, p, k, e);
  if (rc != EMBNET_OK) return rc;
  EMBNET_CHECK_ARG(bins >= 2 && bins <= FAST_AP_MAX_BINS, "fast_ap_loss_fwd: bins=%d outside [2, %d]", bins, FAST_AP_MAX_BINS);
  rc = pair_check_path_and_workspace("fast_ap_loss_fwd", p, k, e, path, workspace, workspace_bytes,
                                     embnet_fast_ap_loss_workspace_bytes(p, k, e));
  if (rc != EMBNET_OK) return rc;
  return pair_launch<FastApBody>("fast_ap_loss_fwd", fast_ap_kernels, emb, p, k, e, {0.25f * (float)bins, bins}, path, pair_g, counts,
                                 mean_loss, workspace, stream);
}

extern "C" size_t embnet_smooth_ap_loss_workspace_bytes(int p, int k, int e) { return pair_workspace_bytes<SmoothApBody>(p, k, e); }

extern "C" int embnet_smooth_ap_loss_path(int p, int k, int e) { return pair_path(p, k, e); }

extern "C" int embnet_smooth_ap_loss_fwd(const float* emb, int p, int k, int e, float temperature, int path, float* pair_g,
                                         int32_t* counts, float* mean_loss, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = pair_check_common("smooth_ap_loss_fwd", emb && pair_g && counts && mean_loss && workspace, p, k, e);
  if (rc != EMBNET_OK) return rc;
  EMBNET_CHECK_ARG(k <= SMOOTH_AP_MAX_K, "smooth_ap_loss_fwd: k=%d > %d: the k - 1 positives of an anchor take one lane each", k,
                   SMOOTH_AP_MAX_K);
  EMBNET_CHECK_ARG(isfinite(temperature) && temperature > 0.f, "smooth_ap_loss_fwd: temperature=%g must be finite and positive",
                   (double)temperature);
  const float r = 1.f / temperature;                     // one correctly rounded division
  EMBNET_CHECK_ARG(isnormal(r), "smooth_ap_loss_fwd: temperature=%g: 1/temperature is not a normal fp32 number", (double)temperature);
  rc = pair_check_path_and_workspace("smooth_ap_loss_fwd", p, k, e, path, workspace, workspace_bytes,
                                     embnet_smooth_ap_loss_workspace_bytes(p, k, e));
  if (rc != EMBNET_OK) return rc;
  return pair_launch<SmoothApBody>("smooth_ap_loss_fwd", smooth_ap_kernels, emb, p, k, e, {r}, path, pair_g, counts, mean_loss,
                                   workspace, stream);
}
