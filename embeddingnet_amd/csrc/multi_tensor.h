// The multi-tensor launch form: one launch over every tensor of a model.  A kernel takes a device table of per-tensor descriptors
// (each file's own struct; the layouts are in include/embnet.h) and a device list of int32 (tensor index, chunk index) pairs, one
// workgroup of 256 threads per pair; chunk c of a tensor is its elements [c * MT_CHUNK, min((c + 1) * MT_CHUNK, n)).
// embeddingnet_amd/multi_tensor.py builds both arrays.
#pragma once
#include <hip/hip_runtime.h>

namespace embnet {

constexpr int MT_CHUNK = 4096;           // elements per workgroup: 256 threads x 4 float4 — what every *_chunk_elems() returns

struct MtChunk { int tensor; long first; };               // row of the table, first element of the chunk

// pair number c of the list (blockIdx.x, or the loop variable of a kernel that takes several chunks per workgroup)
__device__ __forceinline__ MtChunk mt_chunk(const int* __restrict__ chunks, int c) {
  return MtChunk{chunks[2 * c], (long)chunks[2 * c + 1] * MT_CHUNK};
}

// One workgroup's walk over its chunk of a tensor of n elements: vec4(i) on four elements from i where the chunk is whole and
// every pointer 16-byte aligned (`aligned`), one(i) element by element on tails and unaligned tensors.
template <class Vec4, class One>
__device__ __forceinline__ void mt_walk(long first, long n, bool aligned, Vec4 vec4, One one) {
  const long end = min(first + MT_CHUNK, n);
  if (aligned && end - first == MT_CHUNK) {
#pragma unroll
    for (int it = 0; it < MT_CHUNK / 1024; ++it) vec4(first + it * 1024 + threadIdx.x * 4);
    return;
  }
  for (long i = first + threadIdx.x; i < end; i += 256) one(i);
}

}  // namespace embnet
