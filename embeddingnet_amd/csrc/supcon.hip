// SupCon / NT-Xent: the softmax (InfoNCE) family of contrastive losses over a class-contiguous P x K batch.  Build-defined: the
// reference has no pair-based loss.  Semantics: include/embnet.h.
//
//   X [N, E] fp32, N = P*K, rows c*K .. c*K+K-1 are class c.  S = X X^T.  Anchor i: positives P_i = the other rows of its class,
//   negatives N_i = the rows of other classes.  Logit, ONE rounding form: t_ij = fl(S_ij * r), r = fl(1 / tau) taken once on the
//   host; r > 0 and fl is monotone, so the largest t of a set belongs to its largest S and is that S's own t, bit for bit.
//   denominator `all` (SupCon, Khosla et al. 2020, L_out):   M = max_{a != i} t_a,  d = sum_{a != i} e^{t_a - M}  (>= 1),
//     l_i = log d + (1/(K-1)) sum_p (M - t_p)                          (every term non-negative: nothing cancels)
//     G_ij = r (e^{t_j - M} / d - [j in P_i] / (K-1)),  G_ii = 0.
//   denominator `negatives` (NT-Xent as pytorch-metric-learning has it):   Mn = max_n t_n,  En = sum_n e^{t_n - Mn}  (>= 1),
//     per positive p, the maximum PER PAIR:  m_p = max(t_p, Mn),  a_p = e^{t_p - m_p},  b_p = e^{Mn - m_p},  D_p = a_p + b_p En (>= 1)
//     l_i = (1/(K-1)) sum_p ((m_p - t_p) + log D_p),   Q = sum_p b_p / D_p,
//     G_ip = (r/(K-1)) (a_p / D_p - 1),   G_in = (r/(K-1)) e^{t_n - Mn} Q,   G_ii = 0.
//     (one maximum per anchor would not do: a positive far below another positive, the negatives far below both, has
//     e^{t_p - max} and every e^{t_n - max} underflow, and its logarithm would be taken of 0.)
//   loss = (1/N) sum_i l_i;  backward demb_i = (g / N) sum_j (G_ij + G_ji) x_j: embnet_ms_loss_bwd's contract, and its kernel.
//   counts = {positive pairs N (K-1), violating anchors: max_n S_in >= min_p S_ip on the fp32 S}, exact.
//
// The forward is pair_loss.h's skeleton (per-class path, similarity-matrix path, ticket, fixed-order reduction, launch) around the
// per-anchor body below: a wave minimum over the positives and maxima over both sides, lane-strided expf sums, for `negatives` a
// lane-strided loop over the <= K-1 positives (K reaches 2048 on the matrix path), and the anchor's row of G.
// Nothing is atomic in floating point, every reduction has a fixed order: bitwise reproducible.  No host synchronisation, no
// allocation: capturable in a graph.
#include <math.h>
#include "common.h"
#include "pair_loss.h"
#include "../../include/embnet.h"

namespace embnet {

static_assert(EMBNET_SUPCON_PER_CLASS == PAIR_PER_CLASS && EMBNET_SUPCON_SIMILARITY_MATRIX == PAIR_MATRIX, "path constants");

template <int DENOM>
struct SupconBody : PairDotBody {
  struct Args { float r; };                              // fl(1 / tau)
  using Sum = float;

  static __device__ PairAnchorOut<float> anchor(const float* srow, int n, int k, int lo, int ai, const Args& a, float* grow, int lane) {
    const float r = a.r;
    const float kf = (float)(k - 1);
    const float ck = __fdiv_rn(1.f, kf);
    float mn = INFINITY, px = -INFINITY, mx = -INFINITY;
    for (int j = lane; j < k; j += 64)
      if (j != ai) { const float s = srow[lo + j]; mn = fminf(mn, s); px = fmaxf(px, s); }
    for (int col = lane; col < n; col += 64)
      if (col < lo || col >= lo + k) mx = fmaxf(mx, srow[col]);
    mn = wave_min(mn);                                   // min / max over the positives
    px = wave_max(px);
    mx = wave_max(mx);                                   // max over the negatives
    const int viol = mx >= mn;
    if (DENOM == EMBNET_SUPCON_ALL) {
      const float M = __fmul_rn(fmaxf(px, mx), r);
      float se = 0.f, sh = 0.f;
      for (int col = lane; col < n; col += 64)           // lane-strided, column order
        if (col != lo + ai) se += expf(__fsub_rn(__fmul_rn(srow[col], r), M));
      for (int j = lane; j < k; j += 64)
        if (j != ai) sh += __fsub_rn(M, __fmul_rn(srow[lo + j], r));
      const float d = wave_sum(se);                      // >= 1: the largest logit gives e^0
      for (int col = lane; col < n; col += 64) {
        float g = 0.f;
        if (col != lo + ai) {
          const float w = __fdiv_rn(expf(__fsub_rn(__fmul_rn(srow[col], r), M)), d);
          g = __fmul_rn(r, (col >= lo && col < lo + k) ? __fsub_rn(w, ck) : w);
        }
        grow[col] = g;
      }
      return PairAnchorOut<float>{__fadd_rn(logf(d), __fdiv_rn(wave_sum(sh), kf)), viol, 0};
    } else {
      const float Mn = __fmul_rn(mx, r);
      float se = 0.f;
      for (int col = lane; col < n; col += 64)
        if (col < lo || col >= lo + k) se += expf(__fsub_rn(__fmul_rn(srow[col], r), Mn));
      const float En = wave_sum(se);                     // >= 1
      float sl = 0.f, sq = 0.f;
      for (int j = lane; j < k; j += 64) {
        if (j == ai) continue;
        const float tp = __fmul_rn(srow[lo + j], r);
        const float m = fmaxf(tp, Mn);
        const float b = expf(__fsub_rn(Mn, m));
        const float D = __fadd_rn(expf(__fsub_rn(tp, m)), __fmul_rn(b, En));         // >= 1: one of the two is e^0 (x En >= 1)
        sl += __fadd_rn(__fsub_rn(m, tp), logf(D));
        sq += __fdiv_rn(b, D);
      }
      const float Q = wave_sum(sq);
      const float rck = __fmul_rn(r, ck);
      for (int col = lane; col < n; col += 64) {
        float g = 0.f;
        const float t = __fmul_rn(srow[col], r);
        if (col < lo || col >= lo + k) {
          g = __fmul_rn(rck, __fmul_rn(expf(__fsub_rn(t, Mn)), Q));
        } else if (col != lo + ai) {
          const float m = fmaxf(t, Mn);
          const float D = __fadd_rn(expf(__fsub_rn(t, m)), __fmul_rn(expf(__fsub_rn(Mn, m)), En));
          g = __fmul_rn(rck, __fsub_rn(__fdiv_rn(expf(__fsub_rn(t, m)), D), 1.f));
        }
        grow[col] = g;
      }
      return PairAnchorOut<float>{__fdiv_rn(wave_sum(sl), kf), viol, 0};
    }
  }
  static __device__ int third(const PairAnchorOut<float>&) { return 0; }
  static __device__ void finish(const PairParams<SupconBody>& q, double total, int c0, int, int) {
    q.counts[0] = q.n * (q.k - 1);                       // <= 4096 * 2047 < 2^23
    q.counts[1] = c0;
    *q.mean = (float)(total / (double)q.n);
  }
};
using SupconAll = SupconBody<EMBNET_SUPCON_ALL>;
using SupconNeg = SupconBody<EMBNET_SUPCON_NEGATIVES>;

template <class Body>
__global__ __launch_bounds__(PAIR_CLASS_THREADS) void supcon_class_fwd_kernel(PairParams<Body> q) { pair_class_fwd<Body>(q); }
template <class Body>
__global__ __launch_bounds__(PAIR_SWEEP_THREADS) void supcon_sweep_kernel(PairParams<Body> q) { pair_sweep_fwd<Body>(q); }

template <class Body>
static const PairKernels<Body> supcon_kernels{supcon_class_fwd_kernel<Body>, "embnet::supcon_class_fwd_kernel",
                                              supcon_sweep_kernel<Body>, "embnet::supcon_sweep_kernel"};

}  // namespace embnet

using namespace embnet;

extern "C" size_t embnet_supcon_loss_workspace_bytes(int p, int k, int e) { return pair_workspace_bytes<SupconAll>(p, k, e); }

extern "C" int embnet_supcon_loss_path(int p, int k, int e) { return pair_path(p, k, e); }

extern "C" int embnet_supcon_loss_fwd(const float* emb, int p, int k, int e, float temperature, int denominator, int path,
                                      float* pair_g, int32_t* counts, float* mean_loss, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  int rc = pair_check_common("supcon_loss_fwd", emb && pair_g && counts && mean_loss && workspace, p, k, e);
  if (rc != EMBNET_OK) return rc;
  EMBNET_CHECK_ARG(isfinite(temperature) && temperature > 0.f, "supcon_loss_fwd: temperature=%g must be finite and positive",
                   (double)temperature);
  const float r = 1.f / temperature;                     // one correctly rounded division
  EMBNET_CHECK_ARG(isnormal(r), "supcon_loss_fwd: temperature=%g: 1/temperature is not a normal fp32 number", (double)temperature);
  EMBNET_CHECK_ARG(denominator == EMBNET_SUPCON_ALL || denominator == EMBNET_SUPCON_NEGATIVES,
                   "supcon_loss_fwd: unknown denominator %d", denominator);
  rc = pair_check_path_and_workspace("supcon_loss_fwd", p, k, e, path, workspace, workspace_bytes,
                                     embnet_supcon_loss_workspace_bytes(p, k, e));
  if (rc != EMBNET_OK) return rc;
  if (denominator == EMBNET_SUPCON_ALL)
    return pair_launch<SupconAll>("supcon_loss_fwd", supcon_kernels<SupconAll>, emb, p, k, e, {r}, path, pair_g, counts, mean_loss,
                                  workspace, stream);
  return pair_launch<SupconNeg>("supcon_loss_fwd", supcon_kernels<SupconNeg>, emb, p, k, e, {r}, path, pair_g, counts, mean_loss,
                                workspace, stream);
}
