// Cross-Batch Memory (Wang et al., CVPR 2020, "XBM"): a ring of detached embeddings on the device and the pair losses of a batch
// against that ring.  Build-defined: the reference has no memory.  Semantics: include/embnet.h.
//
//   ring: mem [m, e] fp32, mem_labels [m] int32 (-1: empty), *cursor (device int32): row i of the batch goes to slot
//   (cursor + i) mod m, slots[i] says where, and the LAST workgroup to arrive (common.h's ticket) advances the cursor: every
//   workgroup has read it by then and drained what it stored, so none sees the advanced value.  The cursor is read from device memory
//   by the kernel: a captured graph replays with the ring's current state.  One launch, no memset.
//   loss: X [n, e] batch, y [n] labels, Y [m, e] bank, z [m] bank labels (negative = belongs to no set), self_slots [n] (the column
//   that is the anchor's own copy, excluded).  The anchors are the batch, the others the bank: S = X Y^T into the workspace and
//   then the sweep (rect_loss.h's rect_sweep_launch), one wave per anchor walking its row of S from L2 (a row of 65 536 floats is
//   256 KiB, so the rectangle never fits a workgroup the way the proxies' small path does: ONE forward path, EMBNET_XBM_SWEEP;
//   embnet_xbm_loss_path exists so that a second one can join).  The two kinds are Bodies of that sweep; the predicate "same label, labelled, not my own slot" stands where the P x K losses test
//   [lo, lo + k).
//     contrastive (the XBM paper's criterion): one pass, the kept terms join a per-lane f64 chain (exact products are not needed:
//       the terms are fp32 numbers, the chain has ceil(m / 64) f64 additions and the butterfly six).
//     multi-similarity: MsBody's mining comparisons, pair_loss.h's t, term and side, three passes over the row (extrema, sums, weights).
//     circle (an entry point of its own, embnet_xbm_circle_loss_fwd): pair_loss.h's circle_row, the row of circle_loss.hip.
//   per-anchor partials, the arrival ticket, pair_loss.h's fixed-order f64 reduction by the last workgroup, which also counts the
//   labelled bank slots (integers, any order).
//   backward: demb = (g / n) G Y on the f64 matrix instructions; the bank is detached and there is no column role.  A batch against a
//   long bank leaves the grid ceil(n/32) ceil(e/32) workgroups with m / 32 serial rounds each (128 x 128 against 8192 slots: 16
//   workgroups, 256 rounds, 0.56 ms measured): the slots are then split (rect_loss.h's split product), the slices where the forward
//   kept S.
// A label is only ever compared, never used as an index; a self slot is only ever compared with a column index.  Nothing is atomic
// in floating point, every reduction has a fixed order: bitwise reproducible.  No host synchronisation, no allocation: capturable.
#include <math.h>
#include "rect_loss.h"
#include "../../include/embnet.h"

namespace embnet {

constexpr int XBM_MAX_N = 4096;
constexpr int XBM_MAX_M = 65536;
constexpr int XBM_MAX_E = 4096;
constexpr long XBM_MAX_PAIRS = 1L << 26;                 // n m: S and G are 256 MiB each at most
constexpr int XBM_THREADS = 256;                         // 4 waves: one row (enqueue) or one anchor (sweep) each
constexpr int XBM_WG_ROWS = XBM_THREADS / 64;
static_assert(XBM_THREADS == RECT_THREADS, "rect_sweep_launch launches the sweeps");

// ---- the ring: grid = ceil(n / 4) workgroups, one wave copies one row ---------------------------------------------------------------
__global__ __launch_bounds__(XBM_THREADS) void xbm_enqueue_kernel(const float* __restrict__ emb, const int32_t* __restrict__ labels,
                                                                  int n, int e, float* __restrict__ mem,
                                                                  int32_t* __restrict__ mem_labels, int m, int32_t* cursor,
                                                                  int32_t* __restrict__ slots, int* ticket) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * XBM_WG_ROWS + (threadIdx.x >> 6);
  // whatever the word holds, the slot is inside the ring
  const unsigned cur = (unsigned)__hip_atomic_load(cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) % (unsigned)m;
  if (i < n) {                                           // wave-uniform
    const int slot = (int)((cur + (unsigned)i) % (unsigned)m);
    const float* src = emb + (long)i * e;
    float* dst = mem + (long)slot * e;
    for (int k = lane; k < e; k += 64) dst[k] = src[k];
    if (lane == 0) { mem_labels[slot] = labels[i]; slots[i] = slot; }
  }
  if (!last_workgroup_to_arrive(ticket)) return;
  if (threadIdx.x == 0) *cursor = (int32_t)((cur + (unsigned)n) % (unsigned)m);
}

// ---- the loss of a batch against the bank ----------------------------------------------------------------------------------------------
struct XbmParams {
  const int32_t* labels;                                 // [n]
  const int32_t* mem_labels;                             // [m]
  const int32_t* self_slots;                             // [n] or NULL
  int n, m, kind;
  float a, b, c, d;                                      // margin | alpha, beta, base, epsilon | gamma, O+, D+, m (Circle)
  float* g; int32_t* counts; float* mean;
  int* ticket; double* part_loss; int4* part_cnt;        // workspace: arrival counter (zero between launches), partials
  const float* s;                                        // S [n][m]
};

struct XbmAnchorOut { double loss; int cp, cn; int act = -1; };       // act: whether the anchor is active; -1 = iff it keeps a pair

// What a column is to an anchor of label yi >= 0 whose own copy sits in column self: +1 a positive, -1 a negative, 0 neither.
__device__ __forceinline__ int xbm_role(int z, int col, int yi, int self) {
  if (z < 0 || col == self) return 0;
  return z == yi ? 1 : -1;
}

// The XBM paper's contrastive criterion, one wave, one anchor: a positive is kept iff fl(1 - s) > 0, its term is that difference
// and G = -1; a negative iff s > margin, its term is s and G = +1.  Writes all m entries of the row of G.
struct XbmContrastiveBody {
  static __device__ XbmAnchorOut anchor(const float* __restrict__ srow, const XbmParams& P, int yi, int self, float* __restrict__ grow,
                                        int lane) {
    const int m = P.m;
    const float margin = P.a;
    double sum = 0.0;
    int cp = 0, cn = 0;
    for (int col = lane; col < m; col += 64) {           // lane-strided, column order
      const int role = xbm_role(P.mem_labels[col], col, yi, self);
      const float s = srow[col];
      float g = 0.f;
      if (role > 0) {
        const float t = __fsub_rn(1.f, s);
        if (t > 0.f) { sum += (double)t; g = -1.f; ++cp; }
      } else if (role < 0 && s > margin) {
        sum += (double)s; g = 1.f; ++cn;
      }
      grow[col] = g;
    }
    return XbmAnchorOut{wave_sum(sum), wave_sum(cp), wave_sum(cn)};
  }
};

// Multi-similarity over the label sets: the mining rule, t, the stable sides, l_i and G of multi_similarity.hip's MsBody (the pieces
// are pair_loss.h's), three passes over the row.  An empty side leaves mn = +inf or mx = -inf: the anchor is inactive.
struct XbmMsBody {
  static __device__ XbmAnchorOut anchor(const float* __restrict__ srow, const XbmParams& P, int yi, int self, float* __restrict__ grow,
                                        int lane) {
    const int m = P.m;
    const float alpha = P.a, beta = P.b, base = P.c, eps = P.d;
    float mn = INFINITY, mx = -INFINITY;
    for (int col = lane; col < m; col += 64) {
      const int role = xbm_role(P.mem_labels[col], col, yi, self);
      const float s = srow[col];
      if (role > 0) mn = fminf(mn, s);
      else if (role < 0) mx = fmaxf(mx, s);
    }
    mn = wave_min(mn);                                   // min over the positives (+inf: none)
    mx = wave_max(mx);                                   // max over the negatives (-inf: none)
    const float mxe = __fadd_rn(mx, eps);
    if (!(mxe > mn)) {                                   // inactive (wave-uniform): nothing kept on either side
      for (int col = lane; col < m; col += 64) grow[col] = 0.f;
      return XbmAnchorOut{0.0, 0, 0};
    }
    const float mp = fmaxf(0.f, ms_t(-alpha, mn, base));
    const float mg = fmaxf(0.f, ms_t(beta, mx, base));
    float sp = 0.f, sn = 0.f;
    int cp = 0, cn = 0;
    for (int col = lane; col < m; col += 64) {           // lane-strided, column order
      const int role = xbm_role(P.mem_labels[col], col, yi, self);
      const float s = srow[col];
      if (role > 0) {
        if (mxe > s) { sp += ms_term(-alpha, s, base, mp); ++cp; }
      } else if (role < 0 && __fadd_rn(s, eps) > mn) {
        sn += ms_term(beta, s, base, mg); ++cn;
      }
    }
    const float dp = __fadd_rn(expf(-mp), wave_sum(sp));   // e^{-m} + sum e^{t - m}
    const float dn = __fadd_rn(expf(-mg), wave_sum(sn));
    for (int col = lane; col < m; col += 64) {
      const int role = xbm_role(P.mem_labels[col], col, yi, self);
      const float s = srow[col];
      float g = 0.f;
      if (role > 0) {
        if (mxe > s) g = -__fdiv_rn(ms_term(-alpha, s, base, mp), dp);
      } else if (role < 0 && __fadd_rn(s, eps) > mn) {
        g = __fdiv_rn(ms_term(beta, s, base, mg), dn);
      }
      grow[col] = g;
    }
    return XbmAnchorOut{(double)__fadd_rn(ms_side(mp, dp, alpha), ms_side(mg, dn, beta)), wave_sum(cp), wave_sum(cn)};
  }
};

// Circle loss over the label sets: pair_loss.h's circle_row, the row circle_loss.hip runs in LDS, here on the row in global memory.
// An anchor is active when it has a positive and a negative, whether or not any of them still has alpha > 0.
struct XbmCircleRole {
  const int32_t* __restrict__ z; int yi, self;
  __device__ int operator()(int col) const { return xbm_role(z[col], col, yi, self); }
};

struct XbmCircleBody {
  static __device__ XbmAnchorOut anchor(const float* __restrict__ srow, const XbmParams& P, int yi, int self, float* __restrict__ grow,
                                        int lane) {
    const CircleRowOut o = circle_row(srow, P.m, XbmCircleRole{P.mem_labels, yi, self}, CircleArgs{P.a, P.b, -P.d, P.c, P.d}, grow, lane);
    return XbmAnchorOut{(double)o.loss, o.cp, o.cn, o.active};
  }
};

// labelled bank slots, the same in every thread of the workgroup (integers: any order)
__device__ __forceinline__ int xbm_labelled_slots(const int32_t* __restrict__ mem_labels, int m) {
  int l = 0;
  for (int j = threadIdx.x; j < m; j += XBM_THREADS) l += mem_labels[j] >= 0;
  return block_total256(l);
}

// grid = ceil(n / 4) workgroups, one wave walks one anchor's row of S from L2
template <class Body>
__device__ __forceinline__ void xbm_sweep(const XbmParams& P) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int a = blockIdx.x * XBM_WG_ROWS + wave;
  if (a < P.n) {                                         // wave-uniform
    float* grow = P.g + (long)a * P.m;
    const int yi = P.labels[a];
    XbmAnchorOut o{0.0, 0, 0};
    if (yi < 0) {                                        // unlabelled (wave-uniform): a zero row, no loss
      for (int col = lane; col < P.m; col += 64) grow[col] = 0.f;
    } else {
      o = Body::anchor(P.s + (long)a * P.m, P, yi, P.self_slots ? P.self_slots[a] : -1, grow, lane);
    }
    if (lane == 0) {
      P.part_loss[a] = o.loss;
      P.part_cnt[a] = make_int4(o.cp, o.cn, o.act < 0 ? o.cp + o.cn > 0 : o.act, 0);
    }
  }
  if (!last_workgroup_to_arrive(P.ticket)) return;
  const int slots = xbm_labelled_slots(P.mem_labels, P.m);
  double ts[1];
  int tc[3];
  if (reduce_partials<XBM_THREADS>(P.part_loss, P.part_cnt, P.n, ts, tc)) {
    P.counts[0] = tc[0];                                 // <= n m <= 2^26
    P.counts[1] = tc[1];
    P.counts[2] = tc[2];
    P.counts[3] = slots;
    *P.mean = (float)(ts[0] / (double)P.n);
  }
}

__global__ __launch_bounds__(XBM_THREADS) void xbm_contrastive_sweep_kernel(XbmParams P) { xbm_sweep<XbmContrastiveBody>(P); }
__global__ __launch_bounds__(XBM_THREADS) void xbm_ms_sweep_kernel(XbmParams P) { xbm_sweep<XbmMsBody>(P); }
__global__ __launch_bounds__(XBM_THREADS) void xbm_circle_sweep_kernel(XbmParams P) { xbm_sweep<XbmCircleBody>(P); }

// ---- backward: demb = (g / n) G Y, split over the slots where the bank is long (rect_loss.h's split product) ---------------------------
__global__ __launch_bounds__(256) void xbm_bwd_kernel(const float* __restrict__ G, const float* __restrict__ mem, int n, int m, int e,
                                                      const float* __restrict__ upstream, float* __restrict__ demb) {
  mm_f64_tile<MM_DIRECT, false>(G, nullptr, mem, n, m, e, 0, m, RectScaledOut<true>{upstream, n, demb});
}

__global__ __launch_bounds__(256) void xbm_bwd_part_kernel(const float* __restrict__ G, const float* __restrict__ mem, int n, int m,
                                                           int e, int jchunk, double* __restrict__ part) {
  rect_mm_part<MM_DIRECT, false>(G, nullptr, mem, n, m, e, jchunk, part);
}

__global__ __launch_bounds__(256) void xbm_bwd_sum_kernel(const double* __restrict__ part, int splits, long ne, int n,
                                                          const float* __restrict__ upstream, float* __restrict__ demb) {
  rect_mm_sum<true>(part, splits, ne, n, upstream, demb);
}

// ---- host side: range, workspace layout ---------------------------------------------------------------------------------------------
inline bool xbm_range_ok(int n, int m, int e) {
  return n >= 2 && n <= XBM_MAX_N && m >= n && m <= XBM_MAX_M && (long)n * m <= XBM_MAX_PAIRS && e >= 1 && e <= XBM_MAX_E;
}

// [16 B ticket][n f64 partial losses][n int4 partial counts][n*m f32 S]
struct XbmWorkspace {
  size_t part_loss, part_cnt, s, bytes;
  XbmWorkspace(int n, int m) {
    part_loss = 16;
    part_cnt = part_loss + pair_align16((size_t)n * 8);
    s = part_cnt + (size_t)n * 16;
    bytes = s + pair_align16((size_t)n * m * 4);
  }
};

inline int xbm_check_range(const char* what, int n, int m, int e) {
  EMBNET_CHECK_ARG(n >= 2 && n <= XBM_MAX_N, "%s: n=%d outside [2, %d]", what, n, XBM_MAX_N);
  EMBNET_CHECK_ARG(m >= n && m <= XBM_MAX_M, "%s: m=%d outside [n=%d, %d]", what, m, n, XBM_MAX_M);
  EMBNET_CHECK_ARG((long)n * m <= XBM_MAX_PAIRS, "%s: n*m = %ld > 2^26", what, (long)n * m);
  EMBNET_CHECK_ARG(e >= 1 && e <= XBM_MAX_E, "%s: e=%d outside [1, %d]", what, e, XBM_MAX_E);
  return EMBNET_OK;
}

}  // namespace embnet

using namespace embnet;

extern "C" int embnet_xbm_enqueue(const float* emb, const int32_t* labels, int n, int e, float* mem, int32_t* mem_labels, int m,
                                  int32_t* cursor, int32_t* slots, void* workspace, void* stream) {
  const char* what = "xbm_enqueue";
  EMBNET_CHECK_ARG(emb && labels && mem && mem_labels && cursor && slots && workspace, "%s: null pointer", what);
  EMBNET_CHECK_ARG(m >= 1 && m <= XBM_MAX_M, "%s: m=%d outside [1, %d]", what, m, XBM_MAX_M);
  EMBNET_CHECK_ARG(n >= 1 && n <= m, "%s: n=%d outside [1, m=%d]", what, n, m);
  EMBNET_CHECK_ARG(e >= 1 && e <= XBM_MAX_E, "%s: e=%d outside [1, %d]", what, e, XBM_MAX_E);
  EMBNET_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "%s: workspace must be 16-byte aligned", what);
  EMBNET_TRACE("embnet::xbm_enqueue_kernel", TRACE_BYTES, 8.0 * n * e + 12.0 * n, stream);
  xbm_enqueue_kernel<<<cdiv(n, XBM_WG_ROWS), XBM_THREADS, 0, (hipStream_t)stream>>>(emb, labels, n, e, mem, mem_labels, m, cursor,
                                                                                     slots, (int*)workspace);
  return check_launch(what);
}

extern "C" size_t embnet_xbm_loss_workspace_bytes(int n, int m, int e) {
  return xbm_range_ok(n, m, e) ? XbmWorkspace(n, m).bytes : 0;
}

extern "C" int embnet_xbm_loss_path(int n, int m, int e) { return xbm_range_ok(n, m, e) ? EMBNET_XBM_SWEEP : 0; }

extern "C" int embnet_xbm_loss_fwd(const float* emb, const int32_t* labels, const float* mem, const int32_t* mem_labels,
                                   const int32_t* self_slots, int n, int m, int e, int kind, float a, float b, float c, float d,
                                   float* pair_g, int32_t* counts, float* mean_loss, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  const char* what = "xbm_loss_fwd";
  EMBNET_CHECK_ARG(emb && labels && mem && mem_labels && pair_g && counts && mean_loss && workspace, "%s: null pointer", what);
  const int rc = xbm_check_range(what, n, m, e);
  if (rc != EMBNET_OK) return rc;
  EMBNET_CHECK_ARG(kind == EMBNET_XBM_CONTRASTIVE || kind == EMBNET_XBM_MULTI_SIMILARITY, "%s: unknown kind %d", what, kind);
  if (kind == EMBNET_XBM_CONTRASTIVE) {
    EMBNET_CHECK_ARG(isfinite(a), "%s: margin=%g must be finite", what, (double)a);
  } else {
    EMBNET_CHECK_ARG(isfinite(a) && a > 0.f, "%s: alpha=%g must be finite and positive", what, (double)a);
    EMBNET_CHECK_ARG(isfinite(b) && b > 0.f, "%s: beta=%g must be finite and positive", what, (double)b);
    EMBNET_CHECK_ARG(isfinite(c), "%s: base=%g must be finite", what, (double)c);
    EMBNET_CHECK_ARG(isfinite(d) && d >= 0.f, "%s: epsilon=%g must be finite and non-negative", what, (double)d);
  }
  const XbmWorkspace L(n, m);
  const int rw = check_workspace(what, workspace, workspace_bytes, L.bytes);
  if (rw != EMBNET_OK) return rw;
  char* ws = (char*)workspace;
  float* s = (float*)(ws + L.s);
  XbmParams P{labels, mem_labels, self_slots, n, m, kind, a, b, c, d, pair_g, counts, mean_loss,
              (int*)ws, (double*)(ws + L.part_loss), (int4*)(ws + L.part_cnt), s};
  const int grid = cdiv(n, XBM_WG_ROWS);
  if (kind == EMBNET_XBM_CONTRASTIVE)
    return rect_sweep_launch(what, xbm_contrastive_sweep_kernel, "embnet::xbm_contrastive_sweep_kernel",
                             8.0 * n * m + 4.0 * m * (grid + 1.0), P, emb, mem, s, n, m, e, stream);
  return rect_sweep_launch(what, xbm_ms_sweep_kernel, "embnet::xbm_ms_sweep_kernel", 16.0 * n * m + 4.0 * m * (3.0 * grid + 1.0), P, emb,
                           mem, s, n, m, e, stream);
}

extern "C" int embnet_xbm_circle_loss_fwd(const float* emb, const int32_t* labels, const float* mem, const int32_t* mem_labels,
                                          const int32_t* self_slots, int n, int m_slots, int e, float m, float gamma, float* pair_g,
                                          int32_t* counts, float* mean_loss, void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "xbm_circle_loss_fwd";
  EMBNET_CHECK_ARG(emb && labels && mem && mem_labels && pair_g && counts && mean_loss && workspace, "%s: null pointer", what);
  const int rc = xbm_check_range(what, n, m_slots, e);
  if (rc != EMBNET_OK) return rc;
  CircleArgs a;
  const int ra = circle_args(what, m, gamma, a);
  if (ra != EMBNET_OK) return ra;
  const XbmWorkspace L(n, m_slots);
  const int rw = check_workspace(what, workspace, workspace_bytes, L.bytes);
  if (rw != EMBNET_OK) return rw;
  char* ws = (char*)workspace;
  float* s = (float*)(ws + L.s);
  XbmParams P{labels, mem_labels, self_slots, n, m_slots, 0, a.gamma, a.op, a.dp, a.dn, pair_g, counts, mean_loss,
              (int*)ws, (double*)(ws + L.part_loss), (int4*)(ws + L.part_cnt), s};
  const int grid = cdiv(n, XBM_WG_ROWS);
  return rect_sweep_launch(what, xbm_circle_sweep_kernel, "embnet::xbm_circle_sweep_kernel",
                           16.0 * n * m_slots + 4.0 * m_slots * (3.0 * grid + 1.0), P, emb, mem, s, n, m_slots, e, stream);
}

extern "C" int embnet_xbm_loss_bwd(const float* mem, int n, int m, int e, const float* pair_g, const float* upstream, float* demb,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "xbm_loss_bwd";
  EMBNET_CHECK_ARG(mem && pair_g && demb && workspace, "%s: null pointer", what);
  const int rc = xbm_check_range(what, n, m, e);
  if (rc != EMBNET_OK) return rc;
  const XbmWorkspace L(n, m);
  const int rw = check_workspace(what, workspace, workspace_bytes, L.bytes);
  if (rw != EMBNET_OK) return rw;
  hipStream_t s = (hipStream_t)stream;
  const double flop = 2.0 * n * m * e, bytes = 4.0 * ((double)n * m + (double)m * e + (double)n * e);
  // towards 2048 workgroups; the slices' f64 sums (splits n e doubles) live in S's place (n m floats, not needed any more), so
  // splits <= m / (2 e)
  int splits, jchunk;
  rect_mm_split(n, m, e, 2048, m / (2 * e), splits, jchunk);
  double* part = (double*)((char*)workspace + L.s);
  rect_mm_launch({"embnet::xbm_bwd_kernel", "embnet::xbm_bwd_part_kernel", "embnet::xbm_bwd_sum_kernel"}, flop, bytes,
                 bytes + 8.0 * splits * n * e, n, e, splits, stream,
                 [&](dim3 grid) { xbm_bwd_kernel<<<grid, 256, 0, s>>>(pair_g, mem, n, m, e, upstream, demb); },
                 [&](dim3 grid) { xbm_bwd_part_kernel<<<grid, 256, 0, s>>>(pair_g, mem, n, m, e, jchunk, part); },
                 [&](int grid) { xbm_bwd_sum_kernel<<<grid, 256, 0, s>>>(part, splits, (long)n * e, n, upstream, demb); });
  return check_launch(what);
}
