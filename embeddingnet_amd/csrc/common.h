// Shared host/device helpers for libembnet_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <stdlib.h>
#include <atomic>

namespace embnet {

// ---- error reporting (embnet_last_error) ---------------------------------
char* last_error_buf();                      // thread-local, 512 bytes
int fail(int code, const char* fmt, ...);    // formats into last_error_buf, returns code

enum : int {
  EMBNET_OK = 0,
  EMBNET_EINVAL = -1,      // bad argument (null pointer, size <= 0, unsupported shape)
  EMBNET_ELAUNCH = -2,     // hipLaunch / hipGetLastError failure
  EMBNET_EWORKSPACE = -3,  // caller's workspace too small
};

#define EMBNET_CHECK_ARG(cond, ...) \
  do { if (!(cond)) return ::embnet::fail(::embnet::EMBNET_EINVAL, __VA_ARGS__); } while (0)

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(EMBNET_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
  return EMBNET_OK;
}

// A caller's workspace: 16-byte aligned and at least `need` bytes.  `what` is the entry point's name without `embnet_`.
inline int check_workspace(const char* what, const void* workspace, size_t workspace_bytes, size_t need) {
  EMBNET_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "%s: workspace must be 16-byte aligned", what);
  if (workspace_bytes < need) return fail(EMBNET_EWORKSPACE, "%s: workspace %zu < %zu bytes", what, workspace_bytes, need);
  return EMBNET_OK;
}

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// ---- dynamic LDS beyond the 64 KB a launch gets by default ----------------
// A kernel that asks for more has to opt in, per device; BIG_LDS_BYTES (a gfx950 CU's 160 KB) is the bound of that opt-in and of
// every plan that sizes dynamic LDS.  allow_big_lds<kernel>() in front of such a launch opts the kernel in on the CURRENT device
// the first time it runs there: bit d of the kernel's own word says device d is done, so a launch costs hipGetDevice and one load.
// Two threads may both find the bit clear and both set the attribute (the same value); the acquire / release pair orders the one
// that finds it set behind the call that set it.  A device number past the word is never remembered, only slower.
// STATIC_BYTES: the LDS the kernel declares statically besides; the two together must stay within the CU's, or the runtime
// refuses the attribute (and leaves its error for the next hipGetLastError).
constexpr int BIG_LDS_BYTES = 160 * 1024;
template <auto Kernel, int STATIC_BYTES = 0>
inline void allow_big_lds() {
  static std::atomic<uint64_t> done{0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  const uint64_t bit = (unsigned)dev < 64 ? 1ull << dev : 0;
  if (done.load(std::memory_order_acquire) & bit) return;
  (void)hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, BIG_LDS_BYTES - STATIC_BYTES);
  done.fetch_or(bit, std::memory_order_release);
}

// ---- optional per-kernel timing (embnet_trace_*, include/embnet.h) --------
// A TraceScope around ONE kernel launch records a HIP event before and after it on the launch stream together with
// the kernel's name and its ALGORITHMIC work (FLOP for the MFMA-bound kernels, bytes for the HBM-bound ones).  Off
// (the default) it costs one relaxed load per launch.  bench.py turns it on for a sample of the timed steps.
enum : int { TRACE_FLOP = 0, TRACE_BYTES = 1 };
bool trace_on();
struct TraceScope {
  int idx;
  hipStream_t s;
  TraceScope(const char* name, int unit, double work, void* stream, double bytes = -1.0);
  ~TraceScope();
};
#define EMBNET_CAT2(a, b) a##b
#define EMBNET_CAT(a, b) EMBNET_CAT2(a, b)
#define EMBNET_TRACE(name, unit, work, stream) \
  ::embnet::TraceScope EMBNET_CAT(trace_scope_, __LINE__)(name, unit, (double)(work), (void*)(stream))
// MFMA-bound kernel: FLOP plus the bytes its operands and result occupy (what it must move once)
#define EMBNET_TRACE_FLOP(name, flop, bytes, stream) \
  ::embnet::TraceScope EMBNET_CAT(trace_scope_, __LINE__)(name, ::embnet::TRACE_FLOP, (double)(flop), (void*)(stream), (double)(bytes))

// tuning knobs: read once per process (each call site keeps its own `static const`)
inline long env_long(const char* name, long dflt) { const char* e = getenv(name); return e ? atol(e) : dflt; }
// The format of the pre-split planes of this process (gemm_engine.h): two fp16 pieces + a power-of-two scale per tensor, three matrix
// products per fp32 product (default), or EMBNET_PLANES_F16=0: three bf16 pieces, six products (rounds 2-5).  Read once: every
// producer and consumer of planes in a process uses the same format.
inline bool planes_f16() { static const bool on = env_long("EMBNET_PLANES_F16", 1) != 0; return on; }

// ---- device helpers ------------------------------------------------------
constexpr int WAVE = 64;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// |row|^2 of e floats by the calling wave: lane-strided fma chain, then wave_sum — the same bits in every lane.  The distance
// kernels (pairwise.hip, retrieval.hip) compare each other's results bit for bit, so their norms all come from here.
__device__ __forceinline__ float row_sqnorm(const float* __restrict__ r, int e) {
  float s = 0.f;
  for (int k = threadIdx.x & 63; k < e; k += 64) s = fmaf(r[k], r[k], s);
  return wave_sum(s);
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// Maximum / sum over a 256-thread workgroup (every thread calls): the four waves' results through one LDS array, combined in a
// fixed order (the sum left to right).  The result is thread 0's; block_max256<true> hands it to every thread.  The array
// belongs to the function, not to the call: a kernel that calls one of them twice puts a __syncthreads() between the calls.
template <bool ALL = false>
__device__ __forceinline__ float block_max256(float v) {
  __shared__ float wave_m[4];
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) wave_m[(threadIdx.x >> 6) & 3] = v;
  __syncthreads();
  if (ALL || threadIdx.x == 0) v = fmaxf(fmaxf(wave_m[0], wave_m[1]), fmaxf(wave_m[2], wave_m[3]));
  return v;
}
template <class T>   // float or double
__device__ __forceinline__ T block_sum256(T v) {
  __shared__ T wave_s[4];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) wave_s[(threadIdx.x >> 6) & 3] = v;
  __syncthreads();
  if (threadIdx.x == 0) v = wave_s[0] + wave_s[1] + wave_s[2] + wave_s[3];
  return v;
}
// NV integer totals over a 256-thread workgroup from one pass of the caller's, the same in every thread.  ONCE per kernel: the
// array belongs to the function and no barrier follows the reads, so a second call's writes could overtake the first's reads.
template <int NV>
__device__ __forceinline__ void block_total256(int (&v)[NV]) {
  __shared__ int wave_t[NV][4];
#pragma unroll
  for (int j = 0; j < NV; ++j) v[j] = wave_sum(v[j]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < NV; ++j) wave_t[j][threadIdx.x >> 6] = v[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NV; ++j) v[j] = wave_t[j][0] + wave_t[j][1] + wave_t[j][2] + wave_t[j][3];
}
__device__ __forceinline__ int block_total256(int v) {   // (scalar, not through the array form: the callers' kernels keep their code)
  __shared__ int wave_t[4];
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) wave_t[threadIdx.x >> 6] = v;
  __syncthreads();
  return wave_t[0] + wave_t[1] + wave_t[2] + wave_t[3];
}

// Arrival ticket: whether the calling workgroup is the last of its grid to get here (every thread calls; the answer is
// workgroup-uniform).  `ticket` is zero before the launch and zero again after it: the last arriver re-arms it.  The hand-off
// is the order MI355X_MICROARCH.md prescribes: every storing wave drains its stores, barrier, one lane releases at agent scope,
// drains, then takes the ticket; the last arriver acquires, drains, and a barrier lets its waves read what the other workgroups
// wrote (with relaxed agent-scope loads).
__device__ __forceinline__ bool last_workgroup_to_arrive(int* ticket) {
  __shared__ int s_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int t = atomicAdd(ticket, 1);
    s_last = t == (int)gridDim.x - 1;
    if (s_last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      *ticket = 0;                                       // re-arm the counter for the next launch
    }
  }
  __syncthreads();
  return s_last != 0;
}

// Range emission (conv.hip "Ranges"): the workgroup's max |value| joins a range word — the bit pattern of a non-negative float
// under an unsigned maximum, independent of the order, so reproducible.  One atomic per workgroup (256 threads, every thread
// calls; amax >= 0, threads without an element pass 0).  A kernel of thousands of workgroups must NOT aim them all at one word
// (same-address atomics serialise at the memory side: a BatchNorm-backward pass ran 4x longer): the BatchNorm passes spread
// theirs over the RANGE_PARTIALS words behind the slot's first (word 1 + blockIdx % RANGE_PARTIALS, zeroed by the finalize kernel
// in front) and a one-workgroup kernel folds them into word 0, which is what the consumers read.
constexpr int RANGE_PARTIALS = 1024;
__device__ __forceinline__ void range_emit_block(uint32_t* word, float amax) {
  amax = block_max256(amax);
  if (threadIdx.x == 0) atomicMax(word, __float_as_uint(amax));
}
__device__ __forceinline__ float amax4(float m, float4 v) {
  return fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
}

// Activation fused behind the BN affine: 0 none, 1 ReLU, 2 swish (z * sigmoid(z)).  Backward recomputes
// z = x*scale + shift from the saved input, so no activation tensor or mask is stored.
__device__ __forceinline__ float act_apply(int act, float z) {
  return act == 1 ? fmaxf(z, 0.f) : (act == 2 ? z / (1.f + __expf(-z)) : z);
}
__device__ __forceinline__ float act_grad(int act, float z, float dy) {
  if (act == 1) return z <= 0.f ? 0.f : dy;
  if (act == 2) { const float sg = 1.f / (1.f + __expf(-z)); return dy * (sg + z * sg * (1.f - sg)); }
  return dy;
}

// Counter-based RNG: one 64-bit mix (splitmix64 finaliser) of (seed, a, b).
// Used for the two random negative-selection rules and for dropout masks.
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint32_t rng_u32(uint64_t seed, uint64_t a, uint64_t b) {
  return (uint32_t)(mix64(mix64(seed ^ (a * 0xD6E8FEB86659FD93ull)) + b) >> 32);
}

// Hermans batch-hard for anchor row a of the class that owns columns [lo, lo + k), by the calling wave, on the anchor's distance
// row (n floats, global memory or LDS): ip = the farthest same-class column other than a, in_ = the closest other-class column,
// the first index on ties; the same in every lane.  A NaN never compares, +inf never wins among the negatives.  When no column of
// a set compares (a non-finite embedding row), the set's first column is taken — NumPy's arg-max / arg-min on an all-NaN or
// all-inf set — so both indices lie in [0, n) whatever the row holds.  Needs k >= 2 and n >= 2 k.
__device__ __forceinline__ void batch_hard_select(const float* row, int n, int k, int a, int lo, int& ip, int& in_) {
  const int lane = threadIdx.x & 63, hi = lo + k;
  float bp = -INFINITY, bn = INFINITY;
  ip = in_ = 0x7fffffff;
  for (int c0 = lane; c0 < n; c0 += 4 * 64) {              // four loads in flight per lane; ascending columns per lane
    float vv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) vv[u] = c0 + 64 * u < n ? row[c0 + 64 * u] : 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = c0 + 64 * u;
      if (c >= n) break;
      const float v = vv[u];
      if (c >= lo && c < hi) { if (c != a && v > bp) { bp = v; ip = c; } }
      else if (v < bn) { bn = v; in_ = c; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bp, o, 64); const int oi = __shfl_xor(ip, o, 64);
    if (ov > bp || (ov == bp && oi < ip)) { bp = ov; ip = oi; }
    const float nv = __shfl_xor(bn, o, 64); const int ni = __shfl_xor(in_, o, 64);
    if (nv < bn || (nv == bn && ni < in_)) { bn = nv; in_ = ni; }
  }
  if (ip == 0x7fffffff) ip = a == lo ? lo + 1 : lo;        // no positive compared: the first same-class row other than the anchor
  if (in_ == 0x7fffffff) in_ = lo > 0 ? 0 : hi;            // no negative compared: the first other-class row
}

}  // namespace embnet
