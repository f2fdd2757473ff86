// Generalised-mean pooling (GeM): y[n,c] = (mean_hw max(x, eps)^p)^(1/p) on NHWC x[n,hw,c], with the exponent p in DEVICE memory
// (one scalar or one per channel) so that it can be a trained parameter: a captured step replays with the p the optimizer wrote.
// The contract — the arithmetic form, the summation orders, the limits — is in include/embnet.h; the kernels below are that text.
//
// Forward: the power sum is normalised by the per-(sample, channel) maximum M, r = z / M in (0, 1], so r^p = exp2f(p log2f(r)) can
// neither overflow nor flush whatever the activations' amplitude, and the largest term is exactly 1.  Two sweeps (the maximum, then
// the sums), but x comes from HBM once: gem_fwd4_kernel keeps a lane's pixels in registers while hw <= 144 (nine per lane).
// Backward: one streaming pass, 8 B per element; the per-(sample, channel) factors come through LDS once per workgroup.  The
// exponent's gradient is a float64 sum of dy * dydp in a fixed order (dydp = dy/dp is a by-product of the forward sweep);
// workgroups hand their partials over by the arrival ticket (common.h) — no floating-point atomics anywhere.
// Cost per element: one IEEE division, one log2f, one exp2f (quarter-rate instructions plus their range fix-ups).  Measured
// (DESIGN.md §6, f-21): the backward moves its 8 B per element at the GAP kernels' byte rate; the forward is bound by that
// arithmetic, at about half of GAP forward's rate.
#include "common.h"
#include "../../include/embnet.h"

namespace embnet {

constexpr float GEM_LN2 = 0.693147180559945309f;
constexpr int GEM_RES = 9;                               // pixels per lane that stay in registers: hw <= 16 * 9

struct F4 { float v[4]; };
__device__ __forceinline__ F4 ldq(const float* p, long i) {
  const float4 t = reinterpret_cast<const float4*>(p)[i];
  return F4{{t.x, t.y, t.z, t.w}};
}
__device__ __forceinline__ void stq(float* p, long i, const F4& a) {
  reinterpret_cast<float4*>(p)[i] = make_float4(a.v[0], a.v[1], a.v[2], a.v[3]);
}
__device__ __forceinline__ float4 as4(const F4& a) { return make_float4(a.v[0], a.v[1], a.v[2], a.v[3]); }
__device__ __forceinline__ F4 asq(const float4 t) { return F4{{t.x, t.y, t.z, t.w}}; }
// the exponents of channel quad cq: one scalar for all (p_stride 0) or the quad's own four
__device__ __forceinline__ F4 ldp(const float* p, int p_stride, int cq) {
  if (p_stride) return ldq(p, cq);
  const float s = p[0];
  return F4{{s, s, s, s}};
}

// one pixel's term: e = r^p joins s; e * ln r joins t
template <bool WITH_T>
__device__ __forceinline__ void gem_term(float z, float m, float p, float& s, float& t) {
#pragma clang fp contract(off)
  const float l = log2f(z / m);
  const float e = exp2f(p * l);
  s += e;
  if (WITH_T) t += e * (l * GEM_LN2);
}

// y and dy/dp from the maximum and the two sums
template <bool WITH_T>
__device__ __forceinline__ void gem_finish(float m, float sum_e, float sum_t, float p, float hw, float& y, float& dydp) {
#pragma clang fp contract(off)
  const float s = sum_e / hw;
  const float ls = log2f(s);
  y = m * exp2f(ls / p);
  if (WITH_T) {
    const float t = sum_t / hw;
    dydp = y * (t / (p * s) - (ls * GEM_LN2) / (p * p));
  }
}

__device__ __forceinline__ float gem_dx(float x, float eps, float g, float y, float pm1) {
#pragma clang fp contract(off)
  if (!(x >= eps)) return 0.f;                           // the clamp passes no gradient (torch.clamp: [x >= min])
  return g * exp2f(pm1 * log2f(x / y));
}

// Workgroup = one sample x 64 channels: 16 channel-quad lanes x 16 pixel lanes (gap_fwd4_kernel's decomposition), grid (c4/16, n).
// RES: hw <= 16 * GEM_RES, the lane's clamped pixels stay in registers between the two sweeps; otherwise the second sweep reads
// x again.
template <bool WITH_T, bool RES>
__global__ __launch_bounds__(256) void gem_fwd4_kernel(const float* __restrict__ x, int hw, int c4, const float* __restrict__ p,
                                                       int p_stride, float eps, float* __restrict__ y,
                                                       float* __restrict__ dydp) {
  __shared__ float4 sh[WITH_T ? 2 : 1][256];
  const int n = blockIdx.y, cl = threadIdx.x & 15, pl = threadIdx.x >> 4;
  const int cq = blockIdx.x * 16 + cl;
  const bool live = cq < c4;
  const float* xi = x + 4 * ((long)n * hw * c4 + (live ? cq : 0));   // pixel i of this quad: quad i * c4 behind
  F4 zr[RES ? GEM_RES : 1];
  F4 m = {{0.f, 0.f, 0.f, 0.f}};                         // (every z >= eps > 0)
  auto clamp_max = [&](F4 v) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { v.v[j] = fmaxf(v.v[j], eps); m.v[j] = fmaxf(m.v[j], v.v[j]); }
    return v;
  };
  if (live) {
    if (RES) {
#pragma unroll
      for (int k = 0; k < GEM_RES; ++k) {
        const int i = pl + 16 * k;
        if (i < hw) zr[k] = clamp_max(ldq(xi, (long)i * c4));
      }
    } else {
      for (int i = pl; i < hw; i += 16) clamp_max(ldq(xi, (long)i * c4));
    }
  }
  sh[0][threadIdx.x] = as4(m);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 16; ++k) {                         // the quad's maximum over the 16 pixel lanes, in every lane
    const F4 o = asq(sh[0][k * 16 + cl]);
#pragma unroll
    for (int j = 0; j < 4; ++j) m.v[j] = fmaxf(m.v[j], o.v[j]);
  }
  __syncthreads();                                       // sh[0] is written again below
  F4 s = {{0.f, 0.f, 0.f, 0.f}}, t = {{0.f, 0.f, 0.f, 0.f}};
  F4 pq = {{1.f, 1.f, 1.f, 1.f}};
  if (live) {
    pq = ldp(p, p_stride, cq);
    auto term = [&](const F4& z) {
#pragma unroll
      for (int j = 0; j < 4; ++j) gem_term<WITH_T>(z.v[j], m.v[j], pq.v[j], s.v[j], t.v[j]);
    };
    if (RES) {
#pragma unroll
      for (int k = 0; k < GEM_RES; ++k)
        if (pl + 16 * k < hw) term(zr[k]);
    } else {
      for (int i = pl; i < hw; i += 16) {
        F4 z = ldq(xi, (long)i * c4);
#pragma unroll
        for (int j = 0; j < 4; ++j) z.v[j] = fmaxf(z.v[j], eps);
        term(z);
      }
    }
  }
  sh[0][threadIdx.x] = as4(s);
  if (WITH_T) sh[WITH_T ? 1 : 0][threadIdx.x] = as4(t);
  __syncthreads();
  if (pl == 0 && live) {                                 // lane sums in ascending lane order, from lane 0's (this thread's)
    for (int k = 1; k < 16; ++k) {
      const F4 a = asq(sh[0][k * 16 + cl]);
#pragma unroll
      for (int j = 0; j < 4; ++j) s.v[j] += a.v[j];
      if (WITH_T) {
        const F4 b = asq(sh[WITH_T ? 1 : 0][k * 16 + cl]);
#pragma unroll
        for (int j = 0; j < 4; ++j) t.v[j] += b.v[j];
      }
    }
    F4 yo, go;
#pragma unroll
    for (int j = 0; j < 4; ++j) gem_finish<WITH_T>(m.v[j], s.v[j], t.v[j], pq.v[j], (float)hw, yo.v[j], go.v[j]);
    stq(y, (long)n * c4 + cq, yo);
    if (WITH_T) stq(dydp, (long)n * c4 + cq, go);
  }
}

// c % 4 != 0: one thread per (sample, channel), pixels in ascending order
template <bool WITH_T>
__global__ __launch_bounds__(256) void gem_fwd_kernel(const float* __restrict__ x, int n, int hw, int c,
                                                      const float* __restrict__ p, int p_stride, float eps,
                                                      float* __restrict__ y, float* __restrict__ dydp) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)n * c) return;
  const int col = (int)(i % c);
  const float* xi = x + (i / c) * hw * c + col;
  float m = 0.f;
  for (int k = 0; k < hw; ++k) m = fmaxf(m, fmaxf(xi[(long)k * c], eps));
  const float pe = p[(long)col * p_stride];
  float s = 0.f, t = 0.f;
  for (int k = 0; k < hw; ++k) gem_term<WITH_T>(fmaxf(xi[(long)k * c], eps), m, pe, s, t);
  float yo, go;
  gem_finish<WITH_T>(m, s, t, pe, (float)hw, yo, go);
  y[i] = yo;
  if (WITH_T) dydp[i] = go;
}

// dx: workgroup = one sample x 64 channels x 256 pixels (16 per lane), grid (c4/16, hw/256, n).  The first 16 threads fetch the
// quads' factors dy / hw, y and p - 1 for all.
__global__ __launch_bounds__(256) void gem_bwd4_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                       const float* __restrict__ y, const float* __restrict__ p, int p_stride,
                                                       float eps, int hw, int c4, float* __restrict__ dx) {
  __shared__ float4 sh_g[16], sh_y[16], sh_q[16];
  const int n = blockIdx.z, cl = threadIdx.x & 15, pl = threadIdx.x >> 4;
  if (threadIdx.x < 16) {
    const int q = blockIdx.x * 16 + (int)threadIdx.x;
    if (q < c4) {
      F4 g = ldq(dy, (long)n * c4 + q), e = ldp(p, p_stride, q);
#pragma unroll
      for (int j = 0; j < 4; ++j) { g.v[j] = g.v[j] / (float)hw; e.v[j] = e.v[j] - 1.f; }
      sh_g[threadIdx.x] = as4(g);
      sh_y[threadIdx.x] = reinterpret_cast<const float4*>(y)[(long)n * c4 + q];
      sh_q[threadIdx.x] = as4(e);
    }
  }
  __syncthreads();
  const int cq = blockIdx.x * 16 + cl;
  if (cq >= c4) return;
  const F4 g = asq(sh_g[cl]), yy = asq(sh_y[cl]), pm1 = asq(sh_q[cl]);
  const int i0 = blockIdx.y * 256 + pl;
#pragma unroll 4
  for (int k = 0; k < 16; ++k) {
    const int i = i0 + 16 * k;
    if (i < hw) {
      const long at = ((long)n * hw + i) * c4 + cq;
      const F4 xv = ldq(x, at);
      F4 o;
#pragma unroll
      for (int j = 0; j < 4; ++j) o.v[j] = gem_dx(xv.v[j], eps, g.v[j], yy.v[j], pm1.v[j]);
      stq(dx, at, o);
    }
  }
}

__global__ __launch_bounds__(256) void gem_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                      const float* __restrict__ y, const float* __restrict__ p, int p_stride,
                                                      float eps, long total, int hw, int c, float* __restrict__ dx) {
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int col = (int)(i % c);
    const long nc = i / ((long)hw * c) * c + col;
    dx[i] = gem_dx(x[i], eps, dy[nc] / (float)hw, y[nc], p[(long)col * p_stride] - 1.f);
  }
}

// The exponent's gradient: float64 sums of dy * dydp (a product of two floats is exact in float64).  Workgroup = 16 channels x 16
// sample lanes, grid c/16.  per_channel: dp[ch].  Otherwise the workgroup's 16 channel sums are added in ascending order into its
// partial, and the last workgroup to arrive adds the partials.
struct GemDpWorkspace { int ticket; int pad[3]; };       // the partials (double [c/16]) follow
static_assert(sizeof(GemDpWorkspace) == 16, "embnet_gem_bwd_workspace_bytes");

__global__ __launch_bounds__(256) void gem_dp_kernel(const float* __restrict__ dy, const float* __restrict__ dydp, int n, int c,
                                                     int per_channel, float* __restrict__ dp, int* ticket, double* part) {
  __shared__ double sh[256];
  __shared__ double sh_ch[16];
  const int cl = threadIdx.x & 15, nl = threadIdx.x >> 4;
  const int ch = blockIdx.x * 16 + cl;
  double acc = 0.0;
  if (ch < c)
    for (int b = nl; b < n; b += 16) acc += (double)dy[(long)b * c + ch] * (double)dydp[(long)b * c + ch];
  sh[threadIdx.x] = acc;
  __syncthreads();
  if (nl == 0) {
    for (int k = 1; k < 16; ++k) acc += sh[k * 16 + cl];
    if (per_channel) { if (ch < c) dp[ch] = (float)acc; }
    else sh_ch[cl] = acc;
  }
  if (per_channel) return;                               // (a kernel argument: the whole grid leaves)
  __syncthreads();
  if (threadIdx.x == 0) {
    double w = sh_ch[0];
    for (int k = 1; k < 16; ++k) w += sh_ch[k];
    part[blockIdx.x] = w;
  }
  if (!last_workgroup_to_arrive(ticket)) return;
  double tot = 0.0;
  for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) tot += __hip_atomic_load(&part[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  tot = block_sum256(tot);
  if (threadIdx.x == 0) dp[0] = (float)tot;
}

static inline bool aligned16(const void* a) { return (reinterpret_cast<uintptr_t>(a) & 15) == 0; }
static inline int gem_ew_blocks(long total) { const long b = (total + 255) / 256; return (int)(b > 4096 ? 4096 : b); }

}  // namespace embnet

using namespace embnet;

static int gem_check_common(const char* what, int n, int hw, int c, const float* p, int p_stride, float eps) {
  EMBNET_CHECK_ARG(n > 0 && hw > 0 && c > 0, "%s: bad argument (n %d, hw %d, c %d)", what, n, hw, c);
  EMBNET_CHECK_ARG(n <= 65535, "%s: n %d > 65535", what, n);
  EMBNET_CHECK_ARG(p_stride == 0 || p_stride == 1, "%s: p_stride must be 0 (scalar) or 1 (per channel), got %d", what, p_stride);
  EMBNET_CHECK_ARG(eps > 0.f, "%s: eps must be > 0 (got %g)", what, (double)eps);   // (a NaN fails too)
  EMBNET_CHECK_ARG((c & 3) || !p_stride || aligned16(p), "%s: a per-channel p must be 16-byte aligned", what);
  return EMBNET_OK;
}

extern "C" int embnet_gem_fwd(const float* x, int n, int hw, int c, const float* p, int p_stride, float eps, float* y, float* dydp,
                              void* stream) {
  EMBNET_CHECK_ARG(x && p && y, "gem_fwd: null pointer");
  if (int rc = gem_check_common("gem_fwd", n, hw, c, p, p_stride, eps)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if ((c & 3) == 0) {
    EMBNET_CHECK_ARG(aligned16(x) && aligned16(y) && aligned16(dydp), "gem_fwd: x, y and dydp must be 16-byte aligned");
    const dim3 grid(cdiv(c / 4, 16), n);
    const int c4 = c / 4;
    const bool res = hw <= 16 * GEM_RES;
    EMBNET_TRACE("embnet::gem_fwd4_kernel", TRACE_BYTES, 4.0 * n * hw * c, stream);
    if (dydp) {
      if (res) gem_fwd4_kernel<true, true><<<grid, 256, 0, s>>>(x, hw, c4, p, p_stride, eps, y, dydp);
      else gem_fwd4_kernel<true, false><<<grid, 256, 0, s>>>(x, hw, c4, p, p_stride, eps, y, dydp);
    } else {
      if (res) gem_fwd4_kernel<false, true><<<grid, 256, 0, s>>>(x, hw, c4, p, p_stride, eps, y, dydp);
      else gem_fwd4_kernel<false, false><<<grid, 256, 0, s>>>(x, hw, c4, p, p_stride, eps, y, dydp);
    }
  } else {
    const int blocks = cdiv((long)n * c, 256);
    EMBNET_TRACE("embnet::gem_fwd_kernel", TRACE_BYTES, 4.0 * n * hw * c, stream);
    if (dydp) gem_fwd_kernel<true><<<blocks, 256, 0, s>>>(x, n, hw, c, p, p_stride, eps, y, dydp);
    else gem_fwd_kernel<false><<<blocks, 256, 0, s>>>(x, n, hw, c, p, p_stride, eps, y, dydp);
  }
  return check_launch("gem_fwd");
}

extern "C" size_t embnet_gem_bwd_workspace_bytes(int c) {
  return c > 0 ? sizeof(GemDpWorkspace) + sizeof(double) * (size_t)cdiv(c, 16) : 0;
}

extern "C" int embnet_gem_bwd(const float* dy, const float* x, const float* y, const float* p, int p_stride, float eps, int n,
                              int hw, int c, float* dx, const float* dydp, float* dp, void* workspace, size_t workspace_bytes,
                              void* stream) {
  EMBNET_CHECK_ARG(dy && x && y && p && dx, "gem_bwd: null pointer");
  if (int rc = gem_check_common("gem_bwd", n, hw, c, p, p_stride, eps)) return rc;
  EMBNET_CHECK_ARG(!dp || dydp, "gem_bwd: dp needs dydp");
  if (dp) {
    EMBNET_CHECK_ARG(workspace, "gem_bwd: dp needs a workspace");
    if (int rc = check_workspace("gem_bwd", workspace, workspace_bytes, embnet_gem_bwd_workspace_bytes(c))) return rc;
  }
  hipStream_t s = (hipStream_t)stream;
  if ((c & 3) == 0) {
    EMBNET_CHECK_ARG(aligned16(dy) && aligned16(x) && aligned16(y) && aligned16(dx), "gem_bwd: dy, x, y and dx must be 16-byte aligned");
    EMBNET_TRACE("embnet::gem_bwd4_kernel", TRACE_BYTES, 8.0 * n * hw * c, stream);
    gem_bwd4_kernel<<<dim3(cdiv(c / 4, 16), cdiv(hw, 256), n), 256, 0, s>>>(dy, x, y, p, p_stride, eps, hw, c / 4, dx);
  } else {
    const long total = (long)n * hw * c;
    EMBNET_TRACE("embnet::gem_bwd_kernel", TRACE_BYTES, 8.0 * n * hw * c, stream);
    gem_bwd_kernel<<<gem_ew_blocks(total), 256, 0, s>>>(dy, x, y, p, p_stride, eps, total, hw, c, dx);
  }
  if (dp) {
    GemDpWorkspace* w = (GemDpWorkspace*)workspace;
    EMBNET_TRACE("embnet::gem_dp_kernel", TRACE_BYTES, 8.0 * n * c, stream);
    gem_dp_kernel<<<cdiv(c, 16), 256, 0, s>>>(dy, dydp, n, c, p_stride, dp, &w->ticket, (double*)(w + 1));
  }
  return check_launch("gem_bwd");
}
