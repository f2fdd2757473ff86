// Circle loss (Sun et al., CVPR 2020) over a class-contiguous P x K batch: an all-pairs log-sum-exp in which every pair is weighted
// by its own distance from its optimum.  Build-defined: the reference has no pair-based loss.  Semantics: include/embnet.h.
//
//   X [N, E] fp32, N = P*K, rows c*K .. c*K+K-1 are class c.  S = X X^T.  Anchor i: positives P_i = the other rows of its class,
//   negatives N_i = the rows of other classes.  With O+ = fl(1 + m), O- = -m, D+ = fl(1 - m), D- = m taken once on the host:
//     alpha+_p = max(fl(O+ - S_ip), 0),  a+_p = fl(-gamma fl(alpha+_p fl(S_ip - D+)));
//     alpha-_n = max(fl(S_in - O-), 0),  a-_n = fl( gamma fl(alpha-_n fl(S_in - D-)));       a pair with alpha = 0 keeps logit 0
//     L+ = M+ + log sum_p e^{a+_p - M+},  L- = M- + log sum_n e^{a-_n - M-}  (M the side's largest logit: each sum >= 1)
//     z = L+ + L-,  l_i = softplus(z) = max(z, 0) + log(1 + e^{-|z|}),  sigma = sigmoid(z) from the same e^{-|z|}
//     G_ip = -(sigma gamma / sum+) alpha+_p e^{a+_p - M+},  G_in = +(sigma gamma / sum-) alpha-_n e^{a-_n - M-},  G_ii = 0:
//     alpha is a CONSTANT of the backward (the authors' and pytorch-metric-learning's detach), so G is not dl/dS with alpha free.
//   loss = (1/N) sum_i l_i;  backward demb_i = (g / N) sum_j (G_ij + G_ji) x_j: embnet_ms_loss_bwd's contract, and its kernel.
//   counts = {positive pairs N (K-1), violating anchors: max_n S_in >= min_p S_ip, negatives with alpha- > 0} on the fp32 S, exact.
//
// The logits are not monotone in S (a+ is a parabola in S), so the maxima are taken over the logits themselves: the first pass
// forms every logit.  The forward is pair_loss.h's skeleton around pair_loss.h's circle_row (xbm.hip runs the same row against
// the memory bank): one wave, one anchor's row of S in LDS, three lane-strided passes in column order (lane l reads bank l mod 32 of
// consecutive words: conflict-free, supcon.hip's pattern).  Nothing is atomic in floating point, every reduction has a fixed
// order: bitwise reproducible.  No host synchronisation, no allocation: capturable in a graph.
#include <math.h>
#include "common.h"
#include "pair_loss.h"
#include "../../include/embnet.h"

namespace embnet {

static_assert(EMBNET_CIRCLE_PER_CLASS == PAIR_PER_CLASS && EMBNET_CIRCLE_SIMILARITY_MATRIX == PAIR_MATRIX, "path constants");

// What a column is to anchor lo + ai of class [lo, lo + k)
struct CircleClassRole {
  int lo, hi, self;
  __device__ int operator()(int col) const { return col == self ? 0 : (col >= lo && col < hi) ? 1 : -1; }
};

struct CircleBody : PairDotBody {
  using Args = CircleArgs;
  using Sum = float;

  static __device__ PairAnchorOut<float> anchor(const float* srow, int n, int k, int lo, int ai, const Args& a, float* grow, int lane) {
    const CircleRowOut o = circle_row(srow, n, CircleClassRole{lo, lo + k, lo + ai}, a, grow, lane);
    return PairAnchorOut<float>{o.loss, o.viol, o.cn};
  }
  static __device__ int third(const PairAnchorOut<float>&) { return 0; }
  static __device__ void finish(const PairParams<CircleBody>& q, double total, int c0, int c1, int) {
    q.counts[0] = q.n * (q.k - 1);                       // <= 4096 * 2047 < 2^23
    q.counts[1] = c0;                                    // <= n
    q.counts[2] = c1;                                    // <= n (n - k) < 2^24
    *q.mean = (float)(total / (double)q.n);
  }
};

__global__ __launch_bounds__(PAIR_CLASS_THREADS) void circle_class_fwd_kernel(PairParams<CircleBody> q) { pair_class_fwd<CircleBody>(q); }
__global__ __launch_bounds__(PAIR_SWEEP_THREADS) void circle_sweep_kernel(PairParams<CircleBody> q) { pair_sweep_fwd<CircleBody>(q); }

static const PairKernels<CircleBody> circle_kernels{circle_class_fwd_kernel, "embnet::circle_class_fwd_kernel", circle_sweep_kernel,
                                                    "embnet::circle_sweep_kernel"};

}  // namespace embnet

using namespace embnet;

extern "C" size_t embnet_circle_loss_workspace_bytes(int p, int k, int e) { return pair_workspace_bytes<CircleBody>(p, k, e); }

extern "C" int embnet_circle_loss_path(int p, int k, int e) { return pair_path(p, k, e); }

extern "C" int embnet_circle_loss_fwd(const float* emb, int p, int k, int e, float m, float gamma, int path, float* pair_g,
                                      int32_t* counts, float* mean_loss, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = pair_check_common("circle_loss_fwd", emb && pair_g && counts && mean_loss && workspace, p, k, e);
  if (rc != EMBNET_OK) return rc;
  CircleArgs a;
  rc = circle_args("circle_loss_fwd", m, gamma, a);
  if (rc != EMBNET_OK) return rc;
  rc = pair_check_path_and_workspace("circle_loss_fwd", p, k, e, path, workspace, workspace_bytes,
                                     embnet_circle_loss_workspace_bytes(p, k, e));
  if (rc != EMBNET_OK) return rc;
  return pair_launch<CircleBody>("circle_loss_fwd", circle_kernels, emb, p, k, e, a, path, pair_g, counts, mean_loss, workspace, stream);
}
