// Retrieval evaluation (Recall@K, MRR) without the distance matrix: rank of each query's nearest same-class gallery item.
//
// The distances are cross_dist_kernel's (pairwise.hip): d2 = fmaxf(|q|^2 + |x|^2 - 2 g, 0), g from the fp32 MFMA chain of
// gemm_engine.h, the norms from the same lane-strided fma chain as row_sqnorm_kernel; a NaN d2 counts as +inf.  Instead of
// storing d2 the epilogue consumes it in registers.  Gallery items are ordered by (d2, index); with d2 >= 0 that is the order
// of the 64-bit key (bits of d2) << 32 | index under unsigned comparison.  Then
//   pass 1: key[r]   = min over the positives of query r (same label, not the excluded column) of their key,
//   pass 2: count[r] = number of negatives (other label, not excluded) whose key is below key[r],
//   rank[r] = 1 + count[r], or 0 when the query has no positive.
// A minimum and an integer count: exact and independent of the order, so the atomics below leave the result bitwise
// reproducible.  Pass 1 only needs the tiles that can hold a positive: every tile of 64 / 128 rows carries a 1 024-bit Bloom
// filter of its labels (retrieval_bloom_kernel), and pass 1 skips a gallery tile whose filter shares no bit with the query
// tile's.  With labels that come grouped by class (how encodings are produced) pass 1 is a sliver of pass 2; with labels
// in random order nothing is skipped and the cost is two full passes — the result is the same either way.
// A workgroup takes one tile of queries and WALKS a range of gallery tiles, keeping the minima / counts of
// its rows in registers; it meets global memory with one atomic per row per wave at the end of the walk, so a row sees
// (gallery splits) x (waves across the tile) atomics per pass, not one per gallery tile.
// ONE walk (retrieval_walk) defines the metric for every kernel of this file: tile range, filter skip, d2, key, exclusion.  What
// a pass keeps is its epilogue struct: NearestPositive and NegativesBelow here, StorePositives and CountByPosition for MAP@R.
// Roofline: MFMA f32, 2 passes x 2*nq*n*e FLOP; HBM traffic O((nq + n) e), workspace O(nq + n).
#include "retrieval_walk.h"

namespace embnet {

// one wave per row: the squared norms of queries and gallery (row_sqnorm, as row_sqnorm_kernel), and the reset of the row's
// key and counter — by this kernel, not a memset node, so a replayed graph starts from a clean state
__global__ __launch_bounds__(256) void retrieval_prep_kernel(const float* __restrict__ q, int nq, const float* __restrict__ x,
                                                             int n, int e, float* __restrict__ qn, float* __restrict__ xn,
                                                             unsigned long long* __restrict__ key, int32_t* __restrict__ count) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row < nq) {
    const float s = row_sqnorm(q + (long)row * e, e);
    if (lane == 0) { qn[row] = s; key[row] = NO_KEY; count[row] = 0; }
  }
  if (row < n) {
    const float s = row_sqnorm(x + (long)row * e, e);
    if (lane == 0) xn[row] = s;
  }
}

// The labels of one tile of rows as a Bloom filter of BLOOM_WORDS x 32 bits, one bit per label (multiplicative hash, top bits).
// No common bit between a query tile's and a gallery tile's filter: no positive in that tile pair.  (BLOOM_WORDS: retrieval_walk.h)
__device__ __forceinline__ unsigned bloom_bit(int32_t label) { return ((unsigned)label * 2654435761u) >> 22; }

// one workgroup per tile of rows_per_tile rows: blockIdx.x < q_tiles the query tiles, the gallery tiles behind them
__global__ __launch_bounds__(256) void retrieval_bloom_kernel(const int32_t* __restrict__ ql, int nq, const int32_t* __restrict__ xl,
                                                              int n, int rows_per_tile, int q_tiles,
                                                              unsigned* __restrict__ qbloom, unsigned* __restrict__ xbloom) {
  __shared__ unsigned s[BLOOM_WORDS];
  const bool is_q = (int)blockIdx.x < q_tiles;
  const int tile = is_q ? blockIdx.x : blockIdx.x - q_tiles;
  const int32_t* labels = is_q ? ql : xl;
  const int rows = is_q ? nq : n;
  if (threadIdx.x < BLOOM_WORDS) s[threadIdx.x] = 0u;
  __syncthreads();
  for (int i = threadIdx.x; i < rows_per_tile; i += 256) {
    const long row = (long)tile * rows_per_tile + i;
    if (row < rows) {
      const unsigned b = bloom_bit(labels[row]);
      atomicOr(&s[b >> 5], 1u << (b & 31));
    }
  }
  __syncthreads();
  if (threadIdx.x < BLOOM_WORDS) (is_q ? qbloom : xbloom)[(long)tile * BLOOM_WORDS + threadIdx.x] = s[threadIdx.x];
}

// pass 1 of Recall@K: the smallest key among each row's positives (key: of the tile's first row)
struct NearestPositive : WalkEpilogue {
  static constexpr bool FILTER = true;
  using Slot = unsigned long long;
  static constexpr Slot INIT = NO_KEY;
  unsigned long long* key;
  __device__ __forceinline__ Slot visit(Slot best, int, int, int, unsigned long long k, bool live, bool same) const {
    // positives are rare.  Said so, the compiler keeps the update behind a branch, as it did when this was a conditional store
    // into an array; as two selects per element a full pass 1 at 128x128 was 3.4 % slower in the one traced call of one
    // session that compared them.
    if (__builtin_expect(live && same, 0)) best = k < best ? k : best;
    return best;
  }
  __device__ static __forceinline__ Slot half_wave(Slot k) { return half_wave_min(k); }
  __device__ __forceinline__ void commit(int rt, Slot k) const { if (k != NO_KEY) atomicMin(&key[rt], k); }
};

// pass 2 of Recall@K: the negatives below the row's pass-1 key (s_thr: the tile's keys in LDS; count: of the tile's first row)
struct NegativesBelow : WalkEpilogue {
  const unsigned long long* s_thr; int32_t* count;
  __device__ __forceinline__ unsigned long long row(int rt) const { return s_thr[rt]; }
  __device__ __forceinline__ int visit(int cnt, int, unsigned long long thr, int, unsigned long long k, bool live, bool same) const {
    return cnt + ((live && !same && k < thr) ? 1 : 0);
  }
  __device__ __forceinline__ void commit(int rt, int c) const { if (c != 0) atomicAdd(&count[rt], c); }
};

struct RetrievalParams {
  WalkParams w;
  unsigned long long* key; int32_t* count;
};

// PASS 1: nearest positive per row; PASS 2: negatives in front of it.  grid = (query tiles, gallery splits).
// (two workgroups per CU asked for where the registers allow them without scratch at 128x128: every instantiation but pass 1
// behind the scalar loader of unaligned or ragged operands, which keeps 12 more address registers next to the 64-bit minima)
template <class G, bool VEC, int PASS>
__global__ __launch_bounds__(256, (VEC || PASS == 2) ? 2 : 1) void retrieval_walk_kernel(RetrievalParams p) {
  __shared__ unsigned long long s_thr[PASS == 2 ? G::BM : 1];
  prio_hi();
  const int m0 = blockIdx.x * G::BM;
  if constexpr (PASS == 1) {
    retrieval_walk<G, VEC>(p.w, NearestPositive{{}, p.key + m0});
  } else {
    for (int i = threadIdx.x; i < G::BM; i += NTHREADS) s_thr[i] = p.key[min(m0 + i, p.w.nq - 1)];
    retrieval_walk<G, VEC>(p.w, NegativesBelow{{}, s_thr, p.count + m0});
  }
}

__global__ __launch_bounds__(256) void retrieval_finish_kernel(const unsigned long long* __restrict__ key,
                                                               const int32_t* __restrict__ count, int nq,
                                                               int32_t* __restrict__ rank, int32_t* __restrict__ pos_index,
                                                               float* __restrict__ pos_d2) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= nq) return;
  const unsigned long long k = key[row];
  const bool none = k == NO_KEY;
  rank[row] = none ? 0 : 1 + count[row];
  pos_index[row] = none ? -1 : (int32_t)(unsigned)(k & 0xffffffffull);
  pos_d2[row] = none ? INFINITY : __uint_as_float((unsigned)(k >> 32));
}

// hits[j] = #{0 < rank <= ks[j]}, *n_valid = #{rank > 0}, *sum_inv_rank = sum 1 / rank over rank > 0 in f64.
// One workgroup, strided partial sums folded in a fixed order: no float atomics, two runs are bitwise equal.
__global__ __launch_bounds__(1024) void retrieval_reduce_kernel(const int32_t* __restrict__ rank, int nq,
                                                                const int32_t* __restrict__ ks, int nk,
                                                                int32_t* __restrict__ hits, int32_t* __restrict__ n_valid,
                                                                double* __restrict__ sum_inv_rank) {
  __shared__ double s_sum[16];
  __shared__ int s_cnt[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double s = 0.0; int valid = 0;
  for (int i = tid; i < nq; i += 1024) {
    const int r = rank[i];
    if (r > 0) { s += 1.0 / (double)r; ++valid; }
  }
  s = wave_sum(s); valid = wave_sum(valid);
  if (lane == 0) { s_sum[wave] = s; s_cnt[wave] = valid; }
  __syncthreads();
  if (tid == 0) {
    double ts = 0.0; int tv = 0;
    for (int w = 0; w < 16; ++w) { ts += s_sum[w]; tv += s_cnt[w]; }
    *sum_inv_rank = ts; *n_valid = tv;
  }
  for (int j = 0; j < nk; ++j) {
    const int k = ks[j];
    int c = 0;
    for (int i = tid; i < nq; i += 1024) { const int r = rank[i]; c += (r > 0 && r <= k) ? 1 : 0; }
    c = wave_sum(c);
    __syncthreads();                                       // s_cnt of the previous round has been read
    if (lane == 0) s_cnt[wave] = c;
    __syncthreads();
    if (tid == 0) {
      int tc = 0;
      for (int w = 0; w < 16; ++w) tc += s_cnt[w];
      hits[j] = tc;
    }
  }
}

}  // namespace embnet

using namespace embnet;

struct RetrievalWorkspace {
  unsigned long long* key; int32_t* count; float* qn; float* xn; unsigned* qbloom; unsigned* xbloom;
  size_t bytes;
  RetrievalWorkspace(void* base, int nq, int n) {
    Bump b{(char*)base};
    key = b.take<unsigned long long>(nq); count = b.take<int32_t>(nq);
    qn = b.take<float>(nq); xn = b.take<float>(n);
    qbloom = b.take_bloom(nq); xbloom = b.take_bloom(n);
    bytes = b.used;
  }
};
extern "C" size_t embnet_retrieval_workspace_bytes(int nq, int n) {
  return nq <= 0 || n <= 0 ? 0 : RetrievalWorkspace(nullptr, nq, n).bytes;
}

// What the two entry points share in front of their walks: the plan, the loader, the grid, the label filters (launched here).
// ws: the entry point's workspace, for its norms and filters.
template <class W>
static WalkSetup walk_setup(const float* q, const int32_t* q_labels, int nq, const float* x, const int32_t* x_labels, int n, int e,
                            int self_exclude, const W& ws, hipStream_t s) {
  WalkSetup su{{q, x, ws.qn, ws.xn, q_labels, x_labels, ws.qbloom, ws.xbloom, nq, n, e, self_exclude ? 1 : 0, 0}};
  int splits;
  retrieval_plan(nq, n, su.big, splits, su.w.tiles_per_split);
  const int tile_rows = su.big ? 128 : 64, q_tiles = cdiv(nq, tile_rows);
  su.vec = (e & 3) == 0 && ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(x)) & 15) == 0;
  su.grid = dim3(q_tiles, splits);
  EMBNET_TRACE("embnet::retrieval_bloom_kernel", TRACE_BYTES, 4.0 * ((double)nq + n), s);
  retrieval_bloom_kernel<<<q_tiles + cdiv(n, tile_rows), 256, 0, s>>>(q_labels, nq, x_labels, n, tile_rows, q_tiles, ws.qbloom, ws.xbloom);
  return su;
}

extern "C" int embnet_retrieval_first_positive(const float* q, const int32_t* q_labels, int nq,
                                               const float* x, const int32_t* x_labels, int n, int e, int self_exclude,
                                               int32_t* rank, int32_t* pos_index, float* pos_d2,
                                               void* workspace, size_t workspace_bytes, void* stream) {
  EMBNET_CHECK_ARG(q && q_labels && x && x_labels && rank && pos_index && pos_d2 && workspace, "retrieval: null pointer");
  EMBNET_CHECK_ARG(nq > 0 && n > 0 && e > 0, "retrieval: nq=%d n=%d e=%d must be positive", nq, n, e);
  EMBNET_CHECK_ARG(!self_exclude || nq == n, "retrieval: self_exclude needs nq == n (nq=%d n=%d)", nq, n);
  EMBNET_CHECK_ARG((size_t)nq * e * 4 <= MAX_OPERAND_BYTES && (size_t)n * e * 4 <= MAX_OPERAND_BYTES,
                   "retrieval: an embedding block exceeds 2 GiB");
  EMBNET_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "retrieval: workspace must be 16-byte aligned");
  const RetrievalWorkspace w(workspace, nq, n);
  if (workspace_bytes < w.bytes) return fail(EMBNET_EWORKSPACE, "retrieval: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream;
  {
    EMBNET_TRACE("embnet::retrieval_prep_kernel", TRACE_BYTES, 4.0 * ((double)nq * e + (double)n * e), s);
    retrieval_prep_kernel<<<cdiv(nq > n ? nq : n, 4), 256, 0, s>>>(q, nq, x, n, e, w.qn, w.xn, w.key, w.count);
  }
  const WalkSetup su = walk_setup(q, q_labels, nq, x, x_labels, n, e, self_exclude, w, s);
  const RetrievalParams p{su.w, w.key, w.count};
  auto launch = [&](auto g, auto vec, auto pass) {
    retrieval_walk_kernel<decltype(g), decltype(vec)::value, decltype(pass)::value><<<su.grid, 256, 0, s>>>(p);
  };
  const double extra = 16.0 * nq + 8.0 * n;
  walk_dispatch(su, 1, "embnet::retrieval_walk_kernel<1>", extra, s, launch);
  walk_dispatch(su, 2, "embnet::retrieval_walk_kernel<2>", extra, s, launch);
  {
    EMBNET_TRACE("embnet::retrieval_finish_kernel", TRACE_BYTES, 24.0 * nq, s);
    retrieval_finish_kernel<<<cdiv(nq, 256), 256, 0, s>>>(w.key, w.count, nq, rank, pos_index, pos_d2);
  }
  return check_launch("retrieval_first_positive");
}

// ks is device memory: the caller guarantees ks[i] >= 1 (embeddingnet_amd/ops.py refuses anything else before the call)
extern "C" int embnet_retrieval_reduce(const int32_t* rank, int nq, const int32_t* ks, int nk,
                                       int32_t* hits, int32_t* n_valid, double* sum_inv_rank, void* stream) {
  EMBNET_CHECK_ARG(rank && ks && hits && n_valid && sum_inv_rank, "retrieval_reduce: null pointer");
  EMBNET_CHECK_ARG(nq > 0 && nk > 0, "retrieval_reduce: nq=%d nk=%d must be positive", nq, nk);
  EMBNET_CHECK_ARG((reinterpret_cast<uintptr_t>(sum_inv_rank) & 7) == 0, "retrieval_reduce: sum_inv_rank must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  EMBNET_TRACE("embnet::retrieval_reduce_kernel", TRACE_BYTES, 4.0 * nq * (1 + nk), s);
  retrieval_reduce_kernel<<<1, 1024, 0, s>>>(rank, nq, ks, nk, hits, n_valid, sum_inv_rank);
  return check_launch("retrieval_reduce");
}

// ---------------------------------------------------------------------------------------------------------------------------
// MAP@R / R-precision: the position of EVERY positive of a query, not only the first (include/embnet.h, "positive ranks").
// retrieval_walk again: the distance, order, exclusion and label filters are the ones above; what changes is the epilogue:
//   prep:   norms; class sizes by integer atomicAdd, x_slot[c] = the value that add returned (any bijection of a class onto
//           0..count-1 will do: keys carry the gallery index, and the sort below removes the assignment from the result);
//           R[r] = size of the query's class (- 1 with self-exclusion), offset = exclusive scan of R
//   pass 1: every positive's key goes to keys[offset[r] + slot] — each address written once, plain 8-byte stores
//   sort:   each query's segment ascending (a wave with shuffles up to 64 keys, the workgroup in LDS up to R_MAX)
//   pass 2: a negative below the LARGEST positive key counts into between[offset[r] + j], j = the number of the row's positive
//           keys below it (below the smallest one: j = 0, kept in registers as the counting pass above does; otherwise a
//           binary search of the sorted segment and one integer atomicAdd)
//   finish: pos_rank[offset[r] + j] = j + 1 + between[offset[r] + 0..j], pos_index from the key's low word
// Integers only, so the atomics leave the result bitwise reproducible.  Counters, histogram and status are zeroed by a kernel.
// Whatever depends on label contents (capacity, R_MAX, label range) raises `status`; the kernels behind it then exit, and
// every offset-derived address is guarded (slot < R, offset + R <= capacity) whatever the status.
// Roofline: MFMA f32, (1 + visited share) x 2*nq*n*e FLOP as above; on top of it pass 2 pays, per negative between a
// query's first and last positive, ceil(log2 R) dependent 8-byte loads (L2) and one L2 atomic.
namespace embnet {

constexpr int R_MAX = EMBNET_RETRIEVAL_R_MAX;
enum : int { MAP_OK = 0, MAP_CAPACITY = 1, MAP_RMAX = 2, MAP_LABEL = 3 };

__global__ __launch_bounds__(256) void map_zero_kernel(int32_t* __restrict__ class_count, int num_classes,
                                                       int32_t* __restrict__ between, long capacity, int32_t* __restrict__ status) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < num_classes) class_count[i] = 0;
  if (i < capacity) between[i] = 0;
  if (i == 0) *status = MAP_OK;
}

// one wave per row: norms as retrieval_prep_kernel; the gallery row also takes its slot in its class
__global__ __launch_bounds__(256) void map_prep_kernel(const float* __restrict__ q, const int32_t* __restrict__ ql, int nq,
                                                       const float* __restrict__ x, const int32_t* __restrict__ xl, int n, int e,
                                                       int num_classes, float* __restrict__ qn, float* __restrict__ xn,
                                                       int32_t* __restrict__ class_count, int32_t* __restrict__ x_slot,
                                                       int32_t* __restrict__ status) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row < nq) {
    const float s = row_sqnorm(q + (long)row * e, e);
    if (lane == 0) {
      qn[row] = s;
      if ((unsigned)ql[row] >= (unsigned)num_classes) atomicMax(status, (int)MAP_LABEL);
    }
  }
  if (row < n) {
    const float s = row_sqnorm(x + (long)row * e, e);
    if (lane == 0) {
      xn[row] = s;
      const int c = xl[row];
      if ((unsigned)c < (unsigned)num_classes) x_slot[row] = atomicAdd(&class_count[c], 1);
      else { x_slot[row] = 0; atomicMax(status, (int)MAP_LABEL); }
    }
  }
}

__device__ __forceinline__ int map_row_positives(const int32_t* ql, const int32_t* class_count, int num_classes, int self_exclude,
                                                 int row) {
  const int c = ql[row];
  if ((unsigned)c >= (unsigned)num_classes) return 0;
  const int r = class_count[c] - (self_exclude ? 1 : 0);
  return r > 0 ? r : 0;
}

// offset = exclusive scan of R over the queries, one workgroup: thread t owns a contiguous run of queries
__global__ __launch_bounds__(1024) void map_scan_kernel(const int32_t* __restrict__ ql, int nq,
                                                        const int32_t* __restrict__ class_count, int num_classes, int self_exclude,
                                                        long capacity, long long* __restrict__ offset, int32_t* __restrict__ status) {
  __shared__ long long s_wave[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int run = (nq + 1023) / 1024;
  const int i0 = min((long)tid * run, (long)nq), i1 = min((long)i0 + run, (long)nq);
  long long sum = 0; int worst = 0;
  for (int i = i0; i < i1; ++i) {
    const int r = map_row_positives(ql, class_count, num_classes, self_exclude, i);
    sum += r; worst = max(worst, r);
  }
  long long incl = sum;                                    // inclusive scan over the wave, then over the 16 waves
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  long long base = 0, total = 0;
  for (int w = 0; w < 16; ++w) { if (w < wave) base += s_wave[w]; total += s_wave[w]; }
  long long at = base + incl - sum;
  for (int i = i0; i < i1; ++i) {
    offset[i] = at;
    at += map_row_positives(ql, class_count, num_classes, self_exclude, i);
  }
  if (tid == 0) {
    offset[nq] = total;
    if (total > capacity) atomicMax(status, (int)MAP_CAPACITY);
  }
  if (worst > R_MAX) atomicMax(status, (int)MAP_RMAX);
}

struct MapParams {
  WalkParams w;
  const long long* offset; const int32_t* x_slot; const int32_t* status;
  unsigned long long* keys; int32_t* between;
  long capacity;
};

// pass 1 of MAP@R: every positive's key goes to its slot of the row's segment.  s_R, s_off: the rows' segments; s_own: the
// slot of the query's own column (the slots behind it move up by one), past every slot without self-exclusion.
struct StorePositives : WalkEpilogue {
  static constexpr bool FILTER = true;
  const int32_t* x_slot; unsigned long long* keys;
  const int* s_R; const long long* s_off; const int* s_own;
  __device__ __forceinline__ int column(int col) const { return x_slot[col]; }
  __device__ __forceinline__ int row(int rt) const { return s_R[rt]; }
  __device__ __forceinline__ int visit(int, int rt, int R, int cs, unsigned long long k, bool live, bool same) const {
    if (live && same) {
      const int slot = cs - (cs > s_own[rt] ? 1 : 0);
      if ((unsigned)slot < (unsigned)R) keys[s_off[rt] + slot] = k;
    }
    return 0;                                              // nothing to keep per row
  }
};

// pass 2 of MAP@R: a negative counts by the number of the row's positives in front of it.  Below the first positive
// (s_first): in the row's slot, as NegativesBelow; between the first and the last (s_last): a binary search of the sorted
// segment and one atomic.
struct CountByPosition : WalkEpilogue {
  struct Row { unsigned long long first, last; int R; };
  const unsigned long long* keys; int32_t* between;
  const int* s_R; const long long* s_off; const unsigned long long* s_first; const unsigned long long* s_last;
  __device__ __forceinline__ Row row(int rt) const { return {s_first[rt], s_last[rt], s_R[rt]}; }
  __device__ __forceinline__ int visit(int cnt, int rt, Row w, int, unsigned long long k, bool live, bool same) const {
    const bool neg = live && !same;
    cnt += (neg && k < w.first) ? 1 : 0;
    if (neg && k > w.first && k < w.last) {                // between two positives: how many are in front of it
      const unsigned long long* seg = keys + s_off[rt];
      int lo = 1, hi = w.R - 1;                            // keys[0] < k < keys[R - 1]: the answer lies in 1 .. R - 1
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (seg[mid] < k) lo = mid + 1; else hi = mid;
      }
      atomicAdd(&between[s_off[rt] + lo], 1);
    }
    return cnt;
  }
  __device__ __forceinline__ void commit(int rt, int c) const { if (c != 0 && s_R[rt] > 0) atomicAdd(&between[s_off[rt]], c); }
};

// PASS 1 stores the positives' keys, PASS 2 counts the negatives by the number of positives in front of them.  A row whose
// segment does not fit (or a row past nq) gets R = 0: nothing is stored or counted for it.
template <class G, bool VEC, int PASS>
__global__ __launch_bounds__(256, VEC ? 2 : 1) void map_walk_kernel(MapParams p) {
  __shared__ int s_R[G::BM];
  __shared__ long long s_off[G::BM];
  __shared__ int s_own[PASS == 1 ? G::BM : 1];
  __shared__ unsigned long long s_first[PASS == 2 ? G::BM : 1];
  __shared__ unsigned long long s_last[PASS == 2 ? G::BM : 1];
  if (*p.status != MAP_OK) return;                         // the same answer in every thread
  prio_hi();
  const int m0 = blockIdx.x * G::BM;
  for (int i = threadIdx.x; i < G::BM; i += NTHREADS) {
    const int row = min(m0 + i, p.w.nq - 1);
    const long long off = p.offset[row], R = p.offset[row + 1] - off;
    const bool fits = m0 + i < p.w.nq && off >= 0 && R > 0 && R <= R_MAX && off + R <= p.capacity;
    s_off[i] = off; s_R[i] = fits ? (int)R : 0;
    if (PASS == 1) s_own[i] = p.w.self_exclude ? p.x_slot[row] : 0x7fffffff;
    if (PASS == 2) { s_first[i] = fits ? p.keys[off] : 0ull; s_last[i] = fits ? p.keys[off + R - 1] : 0ull; }
  }
  if constexpr (PASS == 1) retrieval_walk<G, VEC>(p.w, StorePositives{{}, p.x_slot, p.keys, s_R, s_off, s_own});
  else retrieval_walk<G, VEC>(p.w, CountByPosition{{}, p.keys, p.between, s_R, s_off, s_first, s_last});
}

// a query's segment, or -1 when there is nothing to do for it (no positive, or a segment that does not fit)
__device__ __forceinline__ int map_segment(const long long* offset, long capacity, int row, long long& off) {
  off = offset[row];
  const long long R = offset[row + 1] - off;
  return (off >= 0 && R > 0 && R <= R_MAX && off + R <= capacity) ? (int)R : -1;
}

// four queries per workgroup.  R <= 64: the query's wave sorts in registers (bitonic over the lanes, NO_KEY padding);
// above: the workgroup sorts the segment in LDS, one such query after the other.
__global__ __launch_bounds__(256) void map_sort_kernel(const long long* __restrict__ offset, int nq, long capacity,
                                                       const int32_t* __restrict__ status, unsigned long long* __restrict__ keys) {
  __shared__ unsigned long long s[R_MAX];
  if (*status != MAP_OK) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  {
    const int row = blockIdx.x * 4 + wave;
    long long off = 0;
    const int R = row < nq ? map_segment(offset, capacity, row, off) : -1;
    if (R > 1 && R <= 64) {
      unsigned long long v = lane < R ? keys[off + lane] : NO_KEY;
#pragma unroll
      for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
          const unsigned long long o = __shfl_xor(v, j, 64);
          const bool keep_min = ((lane & j) == 0) == ((lane & k) == 0);
          v = (keep_min ? o < v : o > v) ? o : v;
        }
      if (lane < R) keys[off + lane] = v;
    }
  }
  for (int w = 0; w < 4; ++w) {                            // the same rows in every thread: the barriers are uniform
    const int row = blockIdx.x * 4 + w;
    long long off = 0;
    const int R = row < nq ? map_segment(offset, capacity, row, off) : -1;
    if (R <= 64) continue;
    int P = 128;
    while (P < R) P <<= 1;
    __syncthreads();                                       // the previous segment has left LDS
    for (int i = tid; i < P; i += 256) s[i] = i < R ? keys[off + i] : NO_KEY;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < P; i += 256) {
          const int o = i ^ j;
          if (o > i) {
            const unsigned long long a = s[i], b = s[o];
            if (((i & k) == 0) == (a > b)) { s[i] = b; s[o] = a; }
          }
        }
        __syncthreads();
      }
    for (int i = tid; i < R; i += 256) keys[off + i] = s[i];
  }
}

// one wave per query: the running sum of `between` over the segment, 64 positives at a time
__global__ __launch_bounds__(256) void map_finish_kernel(const long long* __restrict__ offset, int nq, long capacity,
                                                         const int32_t* __restrict__ status,
                                                         const unsigned long long* __restrict__ keys,
                                                         const int32_t* __restrict__ between, int32_t* __restrict__ pos_index,
                                                         int32_t* __restrict__ pos_rank) {
  if (*status != MAP_OK) return;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= nq) return;
  long long off = 0;
  const int R = map_segment(offset, capacity, row, off);
  int carry = 0;
  for (int j0 = 0; j0 < R; j0 += 64) {
    const int j = j0 + lane;
    int incl = j < R ? between[off + j] : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    if (j < R) {
      pos_rank[off + j] = j + 1 + carry + incl;
      pos_index[off + j] = (int32_t)(unsigned)(keys[off + j] & 0xffffffffull);
    }
    carry += __shfl(incl, 63, 64);
  }
}

// one wave per query: ap@r, r_precision, ap in f64 (lane-strided partial sums, folded in the fixed order of wave_sum)
__global__ __launch_bounds__(256) void map_query_kernel(const long long* __restrict__ offset, const int32_t* __restrict__ pos_rank,
                                                        int nq, double* __restrict__ ap_at_r, double* __restrict__ r_precision,
                                                        double* __restrict__ ap) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= nq) return;
  const long long off = offset[row], R = offset[row + 1] - off;
  double s_in = 0.0, s_all = 0.0; int hits = 0;
  for (long long j = lane; j < R; j += 64) {
    const int pos = pos_rank[off + j];
    const double term = (double)(j + 1) / (double)pos;
    s_all += term;
    if (pos <= R) { s_in += term; ++hits; }
  }
  s_in = wave_sum(s_in); s_all = wave_sum(s_all); hits = wave_sum(hits);
  if (lane == 0) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    ap_at_r[row] = R > 0 ? s_in / (double)R : nan;
    r_precision[row] = R > 0 ? (double)hits / (double)R : nan;
    ap[row] = R > 0 ? s_all / (double)R : nan;
  }
}

// sums[0..2] = the sums of ap_at_r, r_precision, ap over the queries with a positive, *n_valid their number: one workgroup,
// strided partial sums folded in a fixed order as retrieval_reduce_kernel does
__global__ __launch_bounds__(1024) void map_total_kernel(const long long* __restrict__ offset, int nq,
                                                         const double* __restrict__ ap_at_r, const double* __restrict__ r_precision,
                                                         const double* __restrict__ ap, double* __restrict__ sums,
                                                         int32_t* __restrict__ n_valid) {
  __shared__ double s_sum[3][16];
  __shared__ int s_cnt[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double a = 0.0, b = 0.0, c = 0.0; int valid = 0;
  for (int i = tid; i < nq; i += 1024)
    if (offset[i + 1] > offset[i]) { a += ap_at_r[i]; b += r_precision[i]; c += ap[i]; ++valid; }
  a = wave_sum(a); b = wave_sum(b); c = wave_sum(c); valid = wave_sum(valid);
  if (lane == 0) { s_sum[0][wave] = a; s_sum[1][wave] = b; s_sum[2][wave] = c; s_cnt[wave] = valid; }
  __syncthreads();
  if (tid < 3) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t += s_sum[tid][w];
    sums[tid] = t;
  }
  if (tid == 0) {
    int tv = 0;
    for (int w = 0; w < 16; ++w) tv += s_cnt[w];
    *n_valid = tv;
  }
}

}  // namespace embnet

struct MapWorkspace {
  float* qn; float* xn; unsigned* qbloom; unsigned* xbloom; int32_t* class_count; int32_t* x_slot;
  unsigned long long* keys; int32_t* between;
  size_t bytes;
  MapWorkspace(void* base, int nq, int n, int num_classes, long capacity) {
    Bump b{(char*)base};
    qn = b.take<float>(nq); xn = b.take<float>(n);
    qbloom = b.take_bloom(nq); xbloom = b.take_bloom(n);
    class_count = b.take<int32_t>(num_classes); x_slot = b.take<int32_t>(n);
    keys = b.take<unsigned long long>(capacity); between = b.take<int32_t>(capacity);
    bytes = b.used;
  }
};
extern "C" size_t embnet_retrieval_positive_ranks_workspace_bytes(int nq, int n, int num_classes, long capacity) {
  return nq <= 0 || n <= 0 || num_classes <= 0 || capacity <= 0 ? 0 : MapWorkspace(nullptr, nq, n, num_classes, capacity).bytes;
}

extern "C" int embnet_retrieval_positive_ranks(const float* q, const int32_t* q_labels, int nq,
                                               const float* x, const int32_t* x_labels, int n, int e, int self_exclude,
                                               int num_classes, long capacity, long long* offset, int32_t* pos_index,
                                               int32_t* pos_rank, int32_t* status,
                                               void* workspace, size_t workspace_bytes, void* stream) {
  EMBNET_CHECK_ARG(q && q_labels && x && x_labels && offset && pos_index && pos_rank && status && workspace,
                   "retrieval_positive_ranks: null pointer");
  EMBNET_CHECK_ARG(nq > 0 && n > 0 && e > 0 && num_classes > 0 && capacity > 0,
                   "retrieval_positive_ranks: nq=%d n=%d e=%d num_classes=%d capacity=%ld must be positive", nq, n, e, num_classes,
                   capacity);
  EMBNET_CHECK_ARG(!self_exclude || nq == n, "retrieval_positive_ranks: self_exclude needs nq == n (nq=%d n=%d)", nq, n);
  EMBNET_CHECK_ARG((size_t)nq * e * 4 <= MAX_OPERAND_BYTES && (size_t)n * e * 4 <= MAX_OPERAND_BYTES,
                   "retrieval_positive_ranks: an embedding block exceeds 2 GiB");
  EMBNET_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "retrieval_positive_ranks: workspace must be 16-byte aligned");
  EMBNET_CHECK_ARG((reinterpret_cast<uintptr_t>(offset) & 7) == 0, "retrieval_positive_ranks: offset must be 8-byte aligned");
  const MapWorkspace w(workspace, nq, n, num_classes, capacity);
  if (workspace_bytes < w.bytes)
    return fail(EMBNET_EWORKSPACE, "retrieval_positive_ranks: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream;
  {
    EMBNET_TRACE("embnet::map_zero_kernel", TRACE_BYTES, 4.0 * ((double)num_classes + (double)capacity), s);
    const long cells = capacity > num_classes ? capacity : num_classes;
    map_zero_kernel<<<cdiv(cells, 256), 256, 0, s>>>(w.class_count, num_classes, w.between, capacity, status);
  }
  {
    EMBNET_TRACE("embnet::map_prep_kernel", TRACE_BYTES, 4.0 * ((double)nq * e + (double)n * e), s);
    map_prep_kernel<<<cdiv(nq > n ? nq : n, 4), 256, 0, s>>>(q, q_labels, nq, x, x_labels, n, e, num_classes, w.qn, w.xn,
                                                             w.class_count, w.x_slot, status);
  }
  const WalkSetup su = walk_setup(q, q_labels, nq, x, x_labels, n, e, self_exclude, w, s);
  {
    EMBNET_TRACE("embnet::map_scan_kernel", TRACE_BYTES, 16.0 * nq, s);
    map_scan_kernel<<<1, 1024, 0, s>>>(q_labels, nq, w.class_count, num_classes, self_exclude ? 1 : 0, capacity, offset, status);
  }
  const MapParams p{su.w, offset, w.x_slot, status, w.keys, w.between, capacity};
  auto launch = [&](auto g, auto vec, auto pass) {
    map_walk_kernel<decltype(g), decltype(vec)::value, decltype(pass)::value><<<su.grid, 256, 0, s>>>(p);
  };
  const double extra = 16.0 * nq + 12.0 * n + 12.0 * capacity;
  walk_dispatch(su, 1, "embnet::map_walk_kernel<1>", extra, s, launch);
  {
    EMBNET_TRACE("embnet::map_sort_kernel", TRACE_BYTES, 16.0 * capacity, s);
    map_sort_kernel<<<cdiv(nq, 4), 256, 0, s>>>(offset, nq, capacity, status, w.keys);
  }
  walk_dispatch(su, 2, "embnet::map_walk_kernel<2>", extra, s, launch);
  {
    EMBNET_TRACE("embnet::map_finish_kernel", TRACE_BYTES, 20.0 * capacity, s);
    map_finish_kernel<<<cdiv(nq, 4), 256, 0, s>>>(offset, nq, capacity, status, w.keys, w.between, pos_index, pos_rank);
  }
  return check_launch("retrieval_positive_ranks");
}

extern "C" int embnet_retrieval_map_reduce(const long long* offset, const int32_t* pos_rank, int nq,
                                           double* ap_at_r, double* r_precision, double* ap, double* sums, int32_t* n_valid,
                                           void* stream) {
  EMBNET_CHECK_ARG(offset && pos_rank && ap_at_r && r_precision && ap && sums && n_valid, "retrieval_map_reduce: null pointer");
  EMBNET_CHECK_ARG(nq > 0, "retrieval_map_reduce: nq=%d must be positive", nq);
  EMBNET_CHECK_ARG(((reinterpret_cast<uintptr_t>(offset) | reinterpret_cast<uintptr_t>(ap_at_r) | reinterpret_cast<uintptr_t>(r_precision) |
                     reinterpret_cast<uintptr_t>(ap) | reinterpret_cast<uintptr_t>(sums)) & 7) == 0,
                   "retrieval_map_reduce: 64-bit arrays must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  {
    EMBNET_TRACE("embnet::map_query_kernel", TRACE_BYTES, 32.0 * nq, s);
    map_query_kernel<<<cdiv(nq, 4), 256, 0, s>>>(offset, pos_rank, nq, ap_at_r, r_precision, ap);
  }
  {
    EMBNET_TRACE("embnet::map_total_kernel", TRACE_BYTES, 40.0 * nq, s);
    map_total_kernel<<<1, 1024, 0, s>>>(offset, nq, ap_at_r, r_precision, ap, sums, n_valid);
  }
  return check_launch("retrieval_map_reduce");
}
