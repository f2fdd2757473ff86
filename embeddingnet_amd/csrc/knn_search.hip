// k-nearest-neighbour search without the distance matrix: the k smallest keys of every query (include/embnet.h, "k-nearest-
// neighbour search").
//
// ONE walk of retrieval_walk (retrieval_walk.h): the distance, the NaN rule, the key (bits of d2) << 32 | column, the exclusion of
// the query's own column and the loaders are embnet_retrieval_first_positive's.  Its epilogue KeepNearest keeps, for each of the 64
// rows of the workgroup's tile, in dynamic LDS
//   thr   the row's threshold key, NO_KEY until the row has k candidates
//   cnt   the number of candidates in the row's buffer
//   buf   k + BN eight-byte keys: the k kept ones and the room for one more gallery tile
// visit: an eligible key below the row's threshold takes a slot with an LDS atomic on cnt and is stored there.  tile_done (the
// walk runs without FILTER, so it may hold barriers): a row with more than k candidates could not take another BN keys and is
// COMPACTED by one wave — the new keys merged into the sorted k of the last cut by counting (wave_merge_in; keys are unique), the
// keys whose place is below k stored at their place, so the k kept keys come out sorted — and its threshold becomes the k-th key.  A tile adds at most BN keys to a
// row, so cnt <= k + BN always; the store is guarded all the same.  After the warm-up almost nothing passes the threshold and
// compaction is rare; a gallery that comes sorted by descending distance compacts every row after every tile and stays correct.
// Behind the walk every row is compacted once more and its sorted keys, padded with NO_KEY, go to part[split][row][k] in the
// workspace.  knn_merge_kernel, one wave per query, folds the `splits` sorted lists into the final k with the same filter-and-
// compact scheme (a 512-key LDS buffer per wave, appended to by ballot prefix) and writes idx, d2 and found.
// Reproducibility: the keys of a row are unique, so the k smallest of a set do not depend on the order in which the LDS atomics
// hand out slots, nor on when a row is compacted (a stale threshold only admits more candidates).  The outputs are bitwise
// reproducible across runs, streams and graph replay.  Thresholds and counters are initialised by the walk kernel itself.
// Geometry: 64x64 tiles only.  With k = 128 the buffers take 64 x 192 x 8 B = 96 KiB (+ 768 B of thresholds and counters) beside the
// walk's static 18.5 KiB: 115 KiB, one workgroup per CU, every launch through allow_big_lds (common.h).  k <= 57 leaves two
// workgroups per CU (2 x (61.5 + 18.5) KiB).  The 128x128 geometry is NOT instantiated: its buffers (128 x 192 x 8 B = 192 KiB at
// k = 128, 138 KiB beside 37 KiB of static LDS at k = 10) do not fit a CU's 160 KiB.  The splits come from
// retrieval_plan's rule for 64-row tiles (plan_splits).
// Roofline: MFMA f32, 2*nq*n*e FLOP; one LDS read per row per tile for the threshold, one LDS atomic per admitted key.
#include "retrieval_walk.h"
#include <math.h>

namespace embnet {

constexpr int KNN_K_MAX = EMBNET_KNN_K_MAX;
constexpr int KNN_MERGE_CAP = 512;                         // keys of one wave's merge buffer: room for 4 lists of K_MAX keys
using KnnGeom = Geom<64, 64, 2, 2>;

// lane i's key, in every lane (i the same in every lane)
__device__ __forceinline__ unsigned long long wave_key(unsigned long long v, int i) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, i);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), i);
  return ((unsigned long long)hi << 32) | lo;
}

// The calling wave (all 64 lanes) merges the unsorted keys buf[s .. c) into the sorted prefix buf[0 .. s), s <= k <= 64 PER:
// afterwards buf[0 .. min(c, k)) holds the smallest of all of them, ascending; returns that count.  The keys are unique.
// 64 new keys at a time, one per lane; a lane also holds PER keys of the prefix.  Each new key in turn goes round the wave
// (readlane): a new key's place = the new keys below it + the prefix keys below it (a ballot's population count), a prefix
// key moves up by the number of new keys below it.  Places below k are stored; all reads of a round are issued before its first
// store, a wave's LDS operations execute in order, and a round's stores end below the keys of the next round.  The cost follows
// the number of NEW keys, not the buffer's size.
template <int PER>
__device__ __forceinline__ int wave_merge_in(unsigned long long* buf, int s, int c, int k) {
  const int lane = threadIdx.x & 63;
  for (int base = s; base < c; base += 64) {
    const int m = c - base < 64 ? c - base : 64;
    const unsigned long long mine = lane < m ? buf[base + lane] : NO_KEY;
    unsigned long long old[PER]; int up[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) { old[j] = lane + 64 * j < s ? buf[lane + 64 * j] : NO_KEY; up[j] = 0; }
    int place = 0;
    for (int i = 0; i < m; ++i) {
      const unsigned long long v = wave_key(mine, i);
      int below = 0;                                       // prefix keys below v: those that v is not below (padding is above v)
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        const bool b = v < old[j];
        up[j] += b ? 1 : 0;
        below += 64 - __popcll(__ballot(b));
      }
      place += (v < mine ? 1 : 0) + (lane == i ? below : 0);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < m && place < k) buf[place] = mine;          // place < k <= the buffer's size
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int p = lane + 64 * j;
      if (p < s && p + up[j] < k) buf[p + up[j]] = old[j];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    s = s + m < k ? s + m : k;
  }
  return s;
}

struct KeepNearest : WalkEpilogue {
  unsigned long long* s_thr; unsigned long long* s_buf; int* s_cnt;
  int k, cap, select, rows;                                // cap = k + BN; rows: the tile's rows below nq (the walk visits the padding rows too)
  __device__ __forceinline__ unsigned long long row(int rt) const { return s_thr[rt]; }
  __device__ __forceinline__ int visit(int c, int rt, unsigned long long thr, int, unsigned long long key, bool live, bool same) const {
    const bool eligible = live && rt < rows && (select == 0 || (select == 1) == same);
    if (__builtin_expect(eligible && key < thr, 0)) {      // rare behind the warm-up
      const int slot = atomicAdd(&s_cnt[rt], 1);
      if ((unsigned)slot < (unsigned)cap) s_buf[rt * cap + slot] = key;
    }
    return c;
  }
  __device__ static __forceinline__ int half_wave(int c) { return c; }      // nothing is kept in registers
  // every row that could not take another tile's keys is cut back to its k best; wave w owns rows 16 w .. 16 w + 15
  __device__ __forceinline__ void tile_done(int) const {
    __syncthreads();                                       // every wave's keys of this tile are in
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = 0; i < KnnGeom::BM / 4; ++i) {
      const int rt = wave * (KnnGeom::BM / 4) + i;
      const int c = __builtin_amdgcn_readfirstlane(min(s_cnt[rt], cap));
      if (c > k) {                                         // a threshold stands: the first k keys are the sorted result of a cut
        const int sorted = __builtin_amdgcn_readfirstlane(s_thr[rt] != NO_KEY ? k : 0);
        wave_merge_in<KNN_K_MAX / 64>(s_buf + rt * cap, sorted, c, k);
        if (lane == 0) { s_cnt[rt] = k; s_thr[rt] = s_buf[rt * cap + k - 1]; }
      }
    }
    __syncthreads();                                       // thresholds and counters stand before the next tile's visits
  }
};

struct KnnParams {
  WalkParams w;
  unsigned long long* part;                                // [splits][nq][k]
  int k, select;
};

// one wave per row: the squared norms of queries and gallery (row_sqnorm, as retrieval_prep_kernel)
__global__ __launch_bounds__(256) void knn_prep_kernel(const float* __restrict__ q, int nq, const float* __restrict__ x, int n, int e,
                                                       float* __restrict__ qn, float* __restrict__ xn) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row < nq) {
    const float s = row_sqnorm(q + (long)row * e, e);
    if (lane == 0) qn[row] = s;
  }
  if (row < n) {
    const float s = row_sqnorm(x + (long)row * e, e);
    if (lane == 0) xn[row] = s;
  }
}

// grid = (query tiles, gallery splits).  Dynamic LDS: BM thresholds, BM x (k + BN) keys, BM counters.
template <bool VEC>
__global__ __launch_bounds__(256, VEC ? 2 : 1) void knn_walk_kernel(KnnParams p) {
  using G = KnnGeom;
  extern __shared__ unsigned long long s_knn[];
  const int cap = p.k + G::BN;
  unsigned long long* s_thr = s_knn;
  unsigned long long* s_buf = s_knn + G::BM;
  int* s_cnt = (int*)(s_buf + G::BM * cap);
  prio_hi();
  for (int i = threadIdx.x; i < G::BM; i += NTHREADS) { s_thr[i] = NO_KEY; s_cnt[i] = 0; }   // published by the walk's first barrier
  const int m0 = blockIdx.x * G::BM;
  retrieval_walk<G, VEC>(p.w, KeepNearest{{}, s_thr, s_buf, s_cnt, p.k, cap, p.select, p.w.nq - m0});
  // the walk's last tile_done ended on a barrier: every row is complete, and each wave finishes its own rows
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int i = 0; i < G::BM / 4; ++i) {
    const int rt = wave * (G::BM / 4) + i;
    if (m0 + rt >= p.w.nq) break;
    const int c = __builtin_amdgcn_readfirstlane(min(s_cnt[rt], cap));
    const int sorted = __builtin_amdgcn_readfirstlane(s_thr[rt] != NO_KEY ? p.k : 0);
    const int kept = wave_merge_in<KNN_K_MAX / 64>(s_buf + rt * cap, sorted, c, p.k);
    unsigned long long* out = p.part + ((size_t)blockIdx.y * p.w.nq + m0 + rt) * p.k;
    for (int j = lane; j < p.k; j += 64) out[j] = j < kept ? s_buf[rt * cap + j] : NO_KEY;
  }
}

// one wave per query: the k smallest of its `splits` lists (each sorted, padded with NO_KEY), then idx, d2, found
__global__ __launch_bounds__(256) void knn_merge_kernel(const unsigned long long* __restrict__ part, int splits, int nq, int k,
                                                        int32_t* __restrict__ idx, float* __restrict__ d2, int32_t* __restrict__ found) {
  __shared__ unsigned long long s_all[4][KNN_MERGE_CAP];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= nq) return;                                   // no barrier below
  unsigned long long* buf = s_all[wave];
  int cnt = 0, sorted = 0;                                 // buf[0 .. sorted): the result of the last cut
  unsigned long long thr = NO_KEY;
  for (int sp = 0; sp < splits; ++sp) {
    if (cnt + k > KNN_MERGE_CAP) {                         // no room for another list: cut back to the k best
      cnt = sorted = wave_merge_in<KNN_K_MAX / 64>(buf, sorted, cnt, k);
      thr = cnt == k ? buf[k - 1] : NO_KEY;
    }
    const unsigned long long* list = part + ((size_t)sp * nq + row) * k;
    for (int j0 = 0; j0 < k; j0 += 64) {
      const unsigned long long key = j0 + lane < k ? list[j0 + lane] : NO_KEY;
      const bool pass = key < thr;                         // NO_KEY never passes
      const unsigned long long m = __ballot(pass);
      const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
      if (pass && pos < KNN_MERGE_CAP) buf[pos] = key;
      cnt += __popcll(m);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
  cnt = wave_merge_in<KNN_K_MAX / 64>(buf, sorted, cnt < KNN_MERGE_CAP ? cnt : KNN_MERGE_CAP, k);
  for (int j = lane; j < k; j += 64) {
    const unsigned long long key = j < cnt ? buf[j] : NO_KEY;
    idx[(size_t)row * k + j] = j < cnt ? (int32_t)(unsigned)(key & 0xffffffffull) : -1;
    d2[(size_t)row * k + j] = j < cnt ? __uint_as_float((unsigned)(key >> 32)) : INFINITY;
  }
  if (lane == 0) found[row] = cnt;
}

}  // namespace embnet

using namespace embnet;

struct KnnWorkspace {
  float* qn; float* xn; unsigned long long* part; int splits, tiles_per_split;
  size_t bytes;
  KnnWorkspace(void* base, int nq, int n, int k) {
    Bump b{(char*)base};
    plan_splits(nq, n, KnnGeom::BM, splits, tiles_per_split);
    qn = b.take<float>(nq); xn = b.take<float>(n);
    part = b.take<unsigned long long>((size_t)splits * nq * k);
    bytes = b.used;
  }
};
extern "C" size_t embnet_knn_search_workspace_bytes(int nq, int n, int k) {
  return nq <= 0 || n <= 0 || k < 1 || k > KNN_K_MAX ? 0 : KnnWorkspace(nullptr, nq, n, k).bytes;
}

extern "C" int embnet_knn_search(const float* q, const int32_t* q_labels, int nq, const float* x, const int32_t* x_labels, int n,
                                 int e, int self_exclude, int select, int k, int32_t* idx, float* d2, int32_t* found,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  EMBNET_CHECK_ARG(q && x && idx && d2 && found && workspace, "knn_search: null pointer");
  EMBNET_CHECK_ARG(nq > 0 && n > 0 && e > 0, "knn_search: nq=%d n=%d e=%d must be positive", nq, n, e);
  EMBNET_CHECK_ARG(k >= 1 && k <= KNN_K_MAX, "knn_search: k=%d must be in [1, %d]", k, KNN_K_MAX);
  EMBNET_CHECK_ARG(select >= 0 && select <= 2, "knn_search: select=%d must be 0 (all), 1 (same label) or 2 (other label)", select);
  EMBNET_CHECK_ARG(select == 0 || (q_labels && x_labels), "knn_search: select=%d needs q_labels and x_labels", select);
  EMBNET_CHECK_ARG(!self_exclude || nq == n, "knn_search: self_exclude needs nq == n (nq=%d n=%d)", nq, n);
  EMBNET_CHECK_ARG((size_t)nq * e * 4 <= MAX_OPERAND_BYTES && (size_t)n * e * 4 <= MAX_OPERAND_BYTES,
                   "knn_search: an embedding block exceeds 2 GiB");
  EMBNET_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "knn_search: workspace must be 16-byte aligned");
  const KnnWorkspace w(workspace, nq, n, k);
  if (workspace_bytes < w.bytes) return fail(EMBNET_EWORKSPACE, "knn_search: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream;
  {
    EMBNET_TRACE("embnet::knn_prep_kernel", TRACE_BYTES, 4.0 * ((double)nq * e + (double)n * e), s);
    knn_prep_kernel<<<cdiv(nq > n ? nq : n, 4), 256, 0, s>>>(q, nq, x, n, e, w.qn, w.xn);
  }
  // select == 0 reads no label: without label arrays the walk is handed the norms to read in their place (as many words)
  const int32_t* ql = select == 0 ? (const int32_t*)w.qn : q_labels;
  const int32_t* xl = select == 0 ? (const int32_t*)w.xn : x_labels;
  const KnnParams p{{q, x, w.qn, w.xn, ql, xl, nullptr, nullptr, nq, n, e, self_exclude ? 1 : 0, w.tiles_per_split}, w.part, k, select};
  const bool vec = (e & 3) == 0 && ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(x)) & 15) == 0;
  const dim3 grid(cdiv(nq, KnnGeom::BM), w.splits);
  const size_t lds = (size_t)KnnGeom::BM * (8 + (size_t)(k + KnnGeom::BN) * 8 + 4);
  {
    EMBNET_TRACE_FLOP("embnet::knn_walk_kernel", 2.0 * nq * n * e, 4.0 * ((double)nq + n) * e + 8.0 * ((double)nq + n) + 8.0 * w.splits * nq * k, s);
    // the walk's own LDS (operand tiles, the rows' norms and labels) is static: the opt-in covers the dynamic rest of the CU's
    constexpr int STATIC_BYTES = (MAIN_FLOATS<TileKC<KnnGeom::BM>, TileKC<KnnGeom::BN>> + 2 * KnnGeom::BM) * 4;
    if (vec) {
      allow_big_lds<knn_walk_kernel<true>, STATIC_BYTES>();
      knn_walk_kernel<true><<<grid, 256, lds, s>>>(p);
    } else {
      allow_big_lds<knn_walk_kernel<false>, STATIC_BYTES>();
      knn_walk_kernel<false><<<grid, 256, lds, s>>>(p);
    }
  }
  {
    EMBNET_TRACE("embnet::knn_merge_kernel", TRACE_BYTES, 8.0 * w.splits * nq * k + 8.0 * nq * k + 4.0 * nq, s);
    knn_merge_kernel<<<cdiv(nq, 4), 256, 0, s>>>(w.part, w.splits, nq, k, idx, d2, found);
  }
  return check_launch("knn_search");
}
