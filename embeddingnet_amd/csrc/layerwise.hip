// Layer-wise adaptive updates (LARS: You et al. 2017, in the form of SimCLR's LARSOptimizer; LAMB: You et al. 2020) over the
// optimizer's descriptor table and chunk list (optimizer.hip, multi_tensor.h).  Every tensor's step is scaled by a trust ratio
// r = eta |w| / |u|, u the update direction, so two f64 norms per tensor stand in front of every update: two launches.
//   lw_norms_kernel  a bounded grid walks the chunks and writes each chunk's two f64 partials (LAMB: also m and v); the last
//                    workgroup to arrive adds every tensor's partials in a fixed order and writes {W2, U2, r} per tensor
//   lw_step_kernel   one workgroup per chunk applies the update at lr_g * r (LAMB recomputes u from the stored m, v and w by the
//                    same expression, so the norm is of the vector that is applied and no model-sized scratch buffer exists)
// HBM-bound: LARS 8 + 20 bytes per element, LAMB 24 + 16.  The contract, with every rounding, is in include/embnet.h.
#include "common.h"
#include "multi_tensor.h"
#include "../../include/embnet.h"

#pragma clang fp contract(off)            // every rounding of this file is the one written: fmaf where one is meant, none elsewhere

namespace embnet {

struct LwTensor { float* w; const float* g; float* s1; float* s2; long n; float l2x2; int group; };   // the optimizer's descriptor
static_assert(sizeof(LwTensor) == 48, "descriptor layout is part of the ABI (include/embnet.h)");
struct LwStats { double w2, u2; float r, pad; };
static_assert(sizeof(LwStats) == 24, "stats_out layout is part of the ABI (include/embnet.h)");

struct LwGroups { float v[EMBNET_OPT_MAX_GROUPS][4]; };               // lr, unused, wd, eta
struct LwShared { float b1, b2, eps, c1, c2, momentum, clipvalue; int n_groups; };
struct LwRow { float lr, wd, eta; };

// What is workgroup-uniform about a tensor's update: the shared scalars (from device memory under graph replay) and its group's row.
__device__ __forceinline__ void lw_shared(LwShared& h, const float* __restrict__ coef_dev) {
  if (coef_dev) { h.b1 = coef_dev[1]; h.b2 = coef_dev[2]; h.eps = coef_dev[3]; h.c1 = coef_dev[4]; h.c2 = coef_dev[5]; }
}
__device__ __forceinline__ LwRow lw_row(int group, const LwGroups& G, int n_groups, const float* __restrict__ group_dev) {
  const int gi = min(max(group, 0), n_groups - 1);        // whatever the word holds, the row is inside the arrays
  if (group_dev) return LwRow{group_dev[4 * gi], group_dev[4 * gi + 2], group_dev[4 * gi + 3]};
  return LwRow{G.v[gi][0], G.v[gi][2], G.v[gi][3]};
}
// A tensor takes part in a step when it has a gradient (and the slots its rule keeps: a NULL slot reads as no gradient).
template <int RULE>
__device__ __forceinline__ bool lw_live(const LwTensor& t) {
  return t.g && t.s1 && (RULE != EMBNET_LAYERWISE_LAMB || t.s2);
}

// g' of embnet_optimizer_step_groups, in its order and forms, so that embnet_optimizer_grad_norm composes in front
__device__ __forceinline__ float lw_gradient(float w, float g, float l2x2, float clipvalue, bool scaled, float scale) {
  g = fmaf(l2x2, w, g);
  if (clipvalue > 0.f) g = fminf(fmaxf(g, -clipvalue), clipvalue);
  if (scaled) g = g * scale;
  return g;
}
__device__ __forceinline__ void lamb_moments(float& m, float& v, float g, const LwShared& h) {
  m = fmaf(1.f - h.b1, g, h.b1 * m);
  v = fmaf((1.f - h.b2) * g, g, h.b2 * v);
}
// LAMB's direction from the moments as stored: the norms pass and the step form it by this one expression
__device__ __forceinline__ float lamb_direction(float w, float m, float v, float wd, const LwShared& h) {
  return fmaf(wd, w, (m * h.c1) / (sqrtf(v * h.c2) + h.eps));
}

__device__ __forceinline__ void lw_write_stats(LwStats* out, double w2, double u2, float eta) {
  const float r = (eta > 0.f && w2 > 0.0 && u2 > 0.0) ? (float)((double)eta * sqrt(w2) / sqrt(u2)) : 1.f;
  out->w2 = w2;
  out->u2 = u2;
  *reinterpret_cast<float2*>(&out->r) = make_float2(r, 0.f);
}

// ---- the norms (embnet_optimizer_layerwise_norms) ---------------------------------------------------------------------------------
// At most LW_NORM_GRID workgroups, each taking chunks c = blockIdx, blockIdx + grid, ...: every arrival is an atomic on the one ticket
// word and same-address atomics serialise at the memory side (opt_grad_norm_kernel's comment has the measurement).  Thread j of a
// workgroup owns elements first + 1024 it + 4 j .. + 3 of a chunk on both paths, so a tail or an unaligned tensor gets the partials
// (and LAMB's moments) of a whole aligned chunk.
constexpr int LW_NORM_GRID = 512;
struct LwWorkspace { int ticket; int pad[3]; };                         // the partials (double [n_chunks][2]) follow
static_assert(sizeof(LwWorkspace) == 16, "embnet_optimizer_layerwise_workspace_bytes");

template <int RULE>
__global__ __launch_bounds__(256) void lw_norms_kernel(const LwTensor* __restrict__ table, const int* __restrict__ chunks,
                                                       int n_chunks, LwGroups G, LwShared h, const float* __restrict__ coef_dev,
                                                       const float* __restrict__ group_dev,
                                                       const float* __restrict__ clip_scale_dev, int* ticket, double* part,
                                                       LwStats* stats) {
  constexpr bool LAMB = RULE == EMBNET_LAYERWISE_LAMB;
  __shared__ double s_sum[2][4];
  lw_shared(h, coef_dev);
  const bool scaled = clip_scale_dev != nullptr;
  const float cs = scaled ? *clip_scale_dev : 1.f;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const MtChunk ch = mt_chunk(chunks, c);
    const LwTensor t = table[ch.tensor];
    double w2 = 0.0, u2 = 0.0;
    if (lw_live<RULE>(t)) {                                // workgroup-uniform
      const float wd = lw_row(t.group, G, h.n_groups, group_dev).wd;
      const long end = min(ch.first + MT_CHUNK, t.n);
      const uintptr_t bits = (uintptr_t)t.w | (uintptr_t)t.g | (LAMB ? (uintptr_t)t.s1 | (uintptr_t)t.s2 : 0);
      const bool vec = (bits & 15) == 0 && end - ch.first == MT_CHUNK;
#pragma unroll
      for (int it = 0; it < MT_CHUNK / 1024; ++it) {
        const long i = ch.first + it * 1024 + threadIdx.x * 4;
        float w[4] = {0.f, 0.f, 0.f, 0.f}, g[4] = {0.f, 0.f, 0.f, 0.f}, m[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec) {
          *reinterpret_cast<float4*>(w) = *reinterpret_cast<const float4*>(t.w + i);
          *reinterpret_cast<float4*>(g) = *reinterpret_cast<const float4*>(t.g + i);
          if (LAMB) {
            *reinterpret_cast<float4*>(m) = *reinterpret_cast<const float4*>(t.s1 + i);
            *reinterpret_cast<float4*>(v) = *reinterpret_cast<const float4*>(t.s2 + i);
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (i + j >= end) break;
            w[j] = t.w[i + j]; g[j] = t.g[i + j];
            if (LAMB) { m[j] = t.s1[i + j]; v[j] = t.s2[i + j]; }
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (!vec && i + j >= end) break;
          const float gp = lw_gradient(w[j], g[j], t.l2x2, h.clipvalue, scaled, cs);
          float u;
          if (LAMB) { lamb_moments(m[j], v[j], gp, h); u = lamb_direction(w[j], m[j], v[j], wd, h); }
          else u = fmaf(wd, w[j], gp);
          w2 += (double)w[j] * (double)w[j];
          u2 += (double)u * (double)u;
        }
        if (LAMB) {
          if (vec) {
            *reinterpret_cast<float4*>(t.s1 + i) = *reinterpret_cast<const float4*>(m);
            *reinterpret_cast<float4*>(t.s2 + i) = *reinterpret_cast<const float4*>(v);
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              if (i + j >= end) break;
              t.s1[i + j] = m[j]; t.s2[i + j] = v[j];
            }
          }
        }
      }
    }
    w2 = wave_sum(w2);
    u2 = wave_sum(u2);
    __syncthreads();                                       // s_sum, between two chunks
    if (lane == 0) { s_sum[0][wave] = w2; s_sum[1][wave] = u2; }
    __syncthreads();
    if (threadIdx.x == 0) {
      part[2 * c] = s_sum[0][0] + s_sum[0][1] + s_sum[0][2] + s_sum[0][3];
      part[2 * c + 1] = s_sum[1][0] + s_sum[1][1] + s_sum[1][2] + s_sum[1][3];
    }
  }
  if (!last_workgroup_to_arrive(ticket)) return;
  // Every tensor's partials, chunk by chunk p_0 .. p_{k-1}: lane j of one wave adds p_j, p_{j+64}, ... in ascending order onto 0,
  // the 64 sums meet in wave_sum's butterfly.  A tensor's chunks are consecutive and ascending in the list, so the chunk whose
  // index within its tensor is 0 starts the run.  With k = 1 that order gives p_0 itself, which the lane that found the run
  // writes directly; the runs of several chunks of a 64-chunk window follow one by one.  No barrier from here on: the waves
  // take windows of their own.
  for (int base = wave * 64; base < n_chunks; base += 256) {
    const int c = base + lane;
    int tensor = -1, k = 0;
    bool live = false;
    float eta = 0.f;
    if (c < n_chunks && chunks[2 * c + 1] == 0) {
      tensor = chunks[2 * c];
      const LwTensor t = table[tensor];
      k = (int)min((t.n + MT_CHUNK - 1) / MT_CHUNK, (long)(n_chunks - c));      // never past the partials, whatever n holds
      live = lw_live<RULE>(t);
      eta = lw_row(t.group, G, h.n_groups, group_dev).eta;
    }
    if (tensor >= 0 && !live) lw_write_stats(stats + tensor, 0.0, 0.0, 0.f);    // no gradient: {0, 0, 1}
    if (tensor >= 0 && live && k <= 1)
      lw_write_stats(stats + tensor, __hip_atomic_load(&part[2 * c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                     __hip_atomic_load(&part[2 * c + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), eta);
    unsigned long long runs = __ballot(tensor >= 0 && live && k > 1);
    while (runs) {                                         // wave-uniform
      const int src = __ffsll((long long)runs) - 1;
      runs &= runs - 1;
      const int kk = __shfl(k, src), tn = __shfl(tensor, src);
      const float e = __shfl(eta, src);
      const double* p = part + 2 * (long)(base + src);
      double a = 0.0, b = 0.0;
      for (int i = lane; i < kk; i += 64) {
        a += __hip_atomic_load(&p[2 * i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        b += __hip_atomic_load(&p[2 * i + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      a = wave_sum(a);
      b = wave_sum(b);
      if (lane == 0) lw_write_stats(stats + tn, a, b, e);
    }
  }
}

// ---- the update (embnet_optimizer_layerwise_step) ---------------------------------------------------------------------------------
template <int RULE, bool NESTEROV>
__global__ __launch_bounds__(256) void lw_step_kernel(const LwTensor* __restrict__ table, const int* __restrict__ chunks, LwGroups G,
                                                      LwShared h, const float* __restrict__ coef_dev,
                                                      const float* __restrict__ group_dev,
                                                      const float* __restrict__ clip_scale_dev, const LwStats* __restrict__ stats) {
  constexpr bool LAMB = RULE == EMBNET_LAYERWISE_LAMB;
  const MtChunk c = mt_chunk(chunks, blockIdx.x);
  const LwTensor t = table[c.tensor];
  if (!lw_live<RULE>(t)) return;                           // no gradient this step: weight and slots untouched
  lw_shared(h, coef_dev);
  const LwRow row = lw_row(t.group, G, h.n_groups, group_dev);
  const float s = row.lr * stats[c.tensor].r;
  const bool scaled = clip_scale_dev != nullptr;
  const float cs = scaled ? *clip_scale_dev : 1.f;
  // slot1 = LARS' velocity, read and written; LAMB's m and v (slot2) are only read here, its gradient not at all
  auto update = [&](float& w, float g, float& s1, float s2) {
    if (LAMB) {
      w = fmaf(-s, lamb_direction(w, s1, s2, row.wd, h), w);
    } else {
      const float su = s * fmaf(row.wd, w, lw_gradient(w, g, t.l2x2, h.clipvalue, scaled, cs));
      s1 = fmaf(h.momentum, s1, su);
      w = w - (NESTEROV ? fmaf(h.momentum, s1, su) : s1);
    }
  };
  const uintptr_t bits = (uintptr_t)t.w | (uintptr_t)t.s1 | (LAMB ? (uintptr_t)t.s2 : (uintptr_t)t.g);
  mt_walk(c.first, t.n, (bits & 15) == 0,
          [&](long i) {
            float4 w = *reinterpret_cast<const float4*>(t.w + i);
            float4 a = *reinterpret_cast<const float4*>(t.s1 + i);
            const float4 b = *reinterpret_cast<const float4*>((LAMB ? t.s2 : t.g) + i);      // v, or the gradient
            update(w.x, b.x, a.x, b.x); update(w.y, b.y, a.y, b.y);
            update(w.z, b.z, a.z, b.z); update(w.w, b.w, a.w, b.w);
            *reinterpret_cast<float4*>(t.w + i) = w;
            if (!LAMB) *reinterpret_cast<float4*>(t.s1 + i) = a;
          },
          [&](long i) {
            float w = t.w[i], a = t.s1[i];
            const float b = LAMB ? t.s2[i] : t.g[i];
            update(w, b, a, b);
            t.w[i] = w;
            if (!LAMB) t.s1[i] = a;
          });
}

// what both entry points refuse before a launch
static int lw_check(const char* what, int rule, const void* table, int n_tensors, const int32_t* chunks, int n_chunks,
                    const float* group_coef, int n_groups, float clipvalue, const float* clip_scale_dev) {
  EMBNET_CHECK_ARG(table && chunks && group_coef, "%s: null pointer", what);
  EMBNET_CHECK_ARG(n_tensors > 0 && n_chunks > 0, "%s: empty table", what);
  EMBNET_CHECK_ARG(rule == EMBNET_LAYERWISE_LARS || rule == EMBNET_LAYERWISE_LAMB, "%s: unknown rule %d", what, rule);
  EMBNET_CHECK_ARG(n_groups >= 1 && n_groups <= EMBNET_OPT_MAX_GROUPS, "%s: %d groups (1..%d)", what, n_groups, EMBNET_OPT_MAX_GROUPS);
  EMBNET_CHECK_ARG(clipvalue >= 0.f, "%s: negative clipvalue", what);                      // (a NaN fails too)
  EMBNET_CHECK_ARG(!(clipvalue > 0.f && clip_scale_dev), "%s: clipvalue and global_clipnorm are exclusive", what);
  return EMBNET_OK;
}

static LwGroups lw_groups(const float* group_coef, int n_groups) {
  LwGroups G = {};
  for (int i = 0; i < n_groups; ++i)
    for (int j = 0; j < 4; ++j) G.v[i][j] = group_coef[4 * i + j];
  return G;
}

}  // namespace embnet

using namespace embnet;

extern "C" size_t embnet_optimizer_layerwise_workspace_bytes(int n_chunks) {
  return n_chunks > 0 ? sizeof(LwWorkspace) + 2 * sizeof(double) * (size_t)n_chunks : 0;
}

extern "C" int embnet_optimizer_layerwise_norms(int rule, const void* table, int n_tensors, const int32_t* chunks, int n_chunks,
                                                const float* group_coef, int n_groups, float b1, float b2, float eps, float c1,
                                                float c2, float clipvalue, const float* clip_scale_dev, const float* coef_dev,
                                                const float* group_coef_dev, void* workspace, size_t workspace_bytes,
                                                void* stats_out, void* stream) {
  const char* what = "optimizer_layerwise_norms";
  if (int rc = lw_check(what, rule, table, n_tensors, chunks, n_chunks, group_coef, n_groups, clipvalue, clip_scale_dev)) return rc;
  EMBNET_CHECK_ARG(workspace && stats_out, "%s: null pointer", what);
  EMBNET_CHECK_ARG((reinterpret_cast<uintptr_t>(stats_out) & 7) == 0, "%s: stats_out must be 8-byte aligned", what);
  if (int rc = check_workspace(what, workspace, workspace_bytes, embnet_optimizer_layerwise_workspace_bytes(n_chunks))) return rc;
  const LwGroups G = lw_groups(group_coef, n_groups);
  const LwShared h{b1, b2, eps, c1, c2, 0.f, clipvalue, n_groups};
  hipStream_t s = (hipStream_t)stream;
  LwWorkspace* ws = (LwWorkspace*)workspace;
  const int grid = n_chunks < LW_NORM_GRID ? n_chunks : LW_NORM_GRID;
  // algorithmic bytes: w and g read; LAMB reads and writes both moments besides
  EMBNET_TRACE("embnet::lw_norms_kernel", TRACE_BYTES, 4.0 * n_chunks * MT_CHUNK * (rule == EMBNET_LAYERWISE_LAMB ? 6 : 2), s);
#define EMBNET_LW_NORMS(R) \
  lw_norms_kernel<R><<<grid, 256, 0, s>>>((const LwTensor*)table, chunks, n_chunks, G, h, coef_dev, group_coef_dev, clip_scale_dev, \
                                          &ws->ticket, (double*)(ws + 1), (LwStats*)stats_out)
  if (rule == EMBNET_LAYERWISE_LAMB) EMBNET_LW_NORMS(EMBNET_LAYERWISE_LAMB);
  else EMBNET_LW_NORMS(EMBNET_LAYERWISE_LARS);
#undef EMBNET_LW_NORMS
  return check_launch(what);
}

extern "C" int embnet_optimizer_layerwise_step(int rule, const void* table, int n_tensors, const int32_t* chunks, int n_chunks,
                                               const float* group_coef, int n_groups, float b1, float b2, float eps, float c1,
                                               float c2, float momentum, int nesterov, float clipvalue,
                                               const float* clip_scale_dev, const float* coef_dev, const float* group_coef_dev,
                                               const void* stats, void* stream) {
  const char* what = "optimizer_layerwise_step";
  if (int rc = lw_check(what, rule, table, n_tensors, chunks, n_chunks, group_coef, n_groups, clipvalue, clip_scale_dev)) return rc;
  EMBNET_CHECK_ARG(stats, "%s: null pointer", what);
  EMBNET_CHECK_ARG((reinterpret_cast<uintptr_t>(stats) & 7) == 0, "%s: stats must be 8-byte aligned", what);
  EMBNET_CHECK_ARG(momentum >= 0.f, "%s: negative momentum", what);
  EMBNET_CHECK_ARG(rule != EMBNET_LAYERWISE_LAMB || (momentum == 0.f && !nesterov), "%s: momentum and nesterov belong to LARS", what);
  const LwGroups G = lw_groups(group_coef, n_groups);
  const LwShared h{b1, b2, eps, c1, c2, momentum, clipvalue, n_groups};
  hipStream_t s = (hipStream_t)stream;
  // algorithmic bytes: LARS w and the velocity read and written, g read; LAMB w read and written, m and v read
  EMBNET_TRACE("embnet::lw_step_kernel", TRACE_BYTES, 4.0 * n_chunks * MT_CHUNK * (rule == EMBNET_LAYERWISE_LAMB ? 4 : 5), s);
#define EMBNET_LW_STEP(R, N) \
  lw_step_kernel<R, N><<<n_chunks, 256, 0, s>>>((const LwTensor*)table, chunks, G, h, coef_dev, group_coef_dev, clip_scale_dev, \
                                                (const LwStats*)stats)
  if (rule == EMBNET_LAYERWISE_LAMB) EMBNET_LW_STEP(EMBNET_LAYERWISE_LAMB, false);
  else if (nesterov) EMBNET_LW_STEP(EMBNET_LAYERWISE_LARS, true);
  else EMBNET_LW_STEP(EMBNET_LAYERWISE_LARS, false);
#undef EMBNET_LW_STEP
  return check_launch(what);
}
