// Averaged copies of a model's tensors — an exponential moving average (EMA) or a stochastic weight average (SWA, Izmailov et
// al.) — kept by ONE launch per step over every tensor, in the multi-tensor form (multi_tensor.h) over a table of {w, avg, n}
// descriptors, so the averaging costs one kernel beside the one-launch update instead of one framework launch per tensor
// (ResNet18: 62 parameters plus 40 BatchNorm statistics).
// Both rules are the same per-element step with a host-computed coefficient c (weight_average.py): EMA c = 1 - decay, SWA
// c = 1 / (snapshots + 1).  A second kernel exchanges w and avg, so that the averaged model can be evaluated in place.
// HBM-bound: update 12 B/element (w r, avg r+w), swap 16 B/element.  No atomics, no workspace.
#include "common.h"
#include "multi_tensor.h"
#include "../../include/embnet.h"

namespace embnet {

struct AvgTensor { float* w; float* avg; long n; long reserved; };
static_assert(sizeof(AvgTensor) == 32, "descriptor layout is part of the ABI (include/embnet.h)");

// avg += c (w - avg) in three roundings, no fma: NumPy float32 arithmetic restates it exactly (tests/weight_average_ref.py)
__device__ __forceinline__ float avg_step(float w, float a, float c) {
#pragma clang fp contract(off)
  const float d = w - a;
  const float p = c * d;
  return a + p;
}

// One workgroup's chunk of one tensor -> (descriptor, first element); false when the list points outside the table or the tensor.
__device__ __forceinline__ bool avg_chunk(const AvgTensor* __restrict__ table, int n_tensors, const int* __restrict__ chunks,
                                          AvgTensor& t, long& first) {
  const MtChunk c = mt_chunk(chunks, blockIdx.x);
  if (c.tensor < 0 || c.tensor >= n_tensors) return false;
  t = table[c.tensor];
  first = c.first;
  return first >= 0 && first < t.n;
}

__device__ __forceinline__ bool avg_aligned(const AvgTensor& t) { return (((uintptr_t)t.w | (uintptr_t)t.avg) & 15) == 0; }

__global__ __launch_bounds__(256) void weight_average_update_kernel(const AvgTensor* __restrict__ table, int n_tensors,
                                                                    const int* __restrict__ chunks, float c,
                                                                    const float* __restrict__ c_dev) {
  if (c_dev) c = *c_dev;                                   // a captured step replays with the step's current coefficient
  if (!(c > 0.f)) return;                                  // no update this step (a NaN too): nothing is read or written
  AvgTensor t; long first;
  if (!avg_chunk(table, n_tensors, chunks, t, first)) return;
  const bool copy = c >= 1.f;                              // avg = w bit for bit: a + 1 (w - a) is not w in fp32
  mt_walk(first, t.n, avg_aligned(t),
          [&](long i) {
            const float4 w = *reinterpret_cast<const float4*>(t.w + i);
            if (copy) { *reinterpret_cast<float4*>(t.avg + i) = w; return; }
            float4 a = *reinterpret_cast<const float4*>(t.avg + i);
            a.x = avg_step(w.x, a.x, c); a.y = avg_step(w.y, a.y, c); a.z = avg_step(w.z, a.z, c); a.w = avg_step(w.w, a.w, c);
            *reinterpret_cast<float4*>(t.avg + i) = a;
          },
          [&](long i) { t.avg[i] = copy ? t.w[i] : avg_step(t.w[i], t.avg[i], c); });
}

// w <-> avg as 32-bit words: no arithmetic touches them, NaN payloads survive
__global__ __launch_bounds__(256) void weight_average_swap_kernel(const AvgTensor* __restrict__ table, int n_tensors,
                                                                  const int* __restrict__ chunks) {
  AvgTensor t; long first;
  if (!avg_chunk(table, n_tensors, chunks, t, first)) return;
  uint32_t* w = reinterpret_cast<uint32_t*>(t.w);
  uint32_t* a = reinterpret_cast<uint32_t*>(t.avg);
  mt_walk(first, t.n, avg_aligned(t),
          [&](long i) {
            const uint4 x = *reinterpret_cast<const uint4*>(w + i);
            const uint4 y = *reinterpret_cast<const uint4*>(a + i);
            *reinterpret_cast<uint4*>(w + i) = y;
            *reinterpret_cast<uint4*>(a + i) = x;
          },
          [&](long i) {
            const uint32_t x = w[i], y = a[i];
            w[i] = y;
            a[i] = x;
          });
}

}  // namespace embnet

using namespace embnet;

extern "C" int embnet_weight_average_update(const void* table, int n_tensors, const int32_t* chunks, int n_chunks, float c,
                                            const float* c_dev, void* stream) {
  EMBNET_CHECK_ARG(table && chunks, "weight_average_update: null pointer");
  EMBNET_CHECK_ARG(n_tensors > 0 && n_chunks > 0, "weight_average_update: empty table");
  EMBNET_CHECK_ARG(c_dev || (c >= 0.f && c <= 1.f), "weight_average_update: coefficient %g outside [0, 1]", (double)c);   // (a NaN fails too)
  hipStream_t s = (hipStream_t)stream;
  // algorithmic bytes: chunk count x chunk size x 4 B x (w read, avg read+write)
  EMBNET_TRACE("embnet::weight_average_update_kernel", TRACE_BYTES, 12.0 * n_chunks * MT_CHUNK, s);
  weight_average_update_kernel<<<n_chunks, 256, 0, s>>>((const AvgTensor*)table, n_tensors, chunks, c, c_dev);
  return check_launch("weight_average_update");
}

extern "C" int embnet_weight_average_swap(const void* table, int n_tensors, const int32_t* chunks, int n_chunks, void* stream) {
  EMBNET_CHECK_ARG(table && chunks, "weight_average_swap: null pointer");
  EMBNET_CHECK_ARG(n_tensors > 0 && n_chunks > 0, "weight_average_swap: empty table");
  hipStream_t s = (hipStream_t)stream;
  // algorithmic bytes: both tensors read and written
  EMBNET_TRACE("embnet::weight_average_swap_kernel", TRACE_BYTES, 16.0 * n_chunks * MT_CHUNK, s);
  weight_average_swap_kernel<<<n_chunks, 256, 0, s>>>((const AvgTensor*)table, n_tensors, chunks);
  return check_launch("weight_average_swap");
}
