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
// in random order nothing is skipped and the cost is two full passes — the result is the same either way.  A workgroup takes one tile of queries and WALKS a range of gallery tiles, keeping the minima / counts of
// its rows in registers; it meets global memory with one atomic per row per wave at the end of the walk, so a row sees
// (gallery splits) x (waves across the tile) atomics per pass, not one per gallery tile.
// Roofline: MFMA f32, 2 passes x 2*nq*n*e FLOP; HBM traffic O((nq + n) e), workspace O(nq + n).
#include "gemm_engine.h"
#include "../../include/embnet.h"

namespace embnet {

constexpr unsigned long long NO_KEY = ~0ull;               // above every key: (+inf, any index) < NO_KEY

// one wave per row: the squared norms of queries and gallery (row_sqnorm_kernel's chain), and the reset of the row's
// key and counter — by this kernel, not a memset node, so a replayed graph starts from a clean state
__global__ __launch_bounds__(256) void retrieval_prep_kernel(const float* __restrict__ q, int nq, const float* __restrict__ x,
                                                             int n, int e, float* __restrict__ qn, float* __restrict__ xn,
                                                             unsigned long long* __restrict__ key, int32_t* __restrict__ count) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row < nq) {
    const float* r = q + (long)row * e;
    float s = 0.f;
    for (int k = lane; k < e; k += 64) s = fmaf(r[k], r[k], s);
    s = wave_sum(s);
    if (lane == 0) { qn[row] = s; key[row] = NO_KEY; count[row] = 0; }
  }
  if (row < n) {
    const float* r = x + (long)row * e;
    float s = 0.f;
    for (int k = lane; k < e; k += 64) s = fmaf(r[k], r[k], s);
    s = wave_sum(s);
    if (lane == 0) xn[row] = s;
  }
}

// The labels of one tile of rows as a Bloom filter of BLOOM_WORDS x 32 bits, one bit per label (multiplicative hash, top bits).
// No common bit between a query tile's and a gallery tile's filter: no positive in that tile pair.
constexpr int BLOOM_WORDS = 32;
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

struct RetrievalParams {
  const float* q; const float* x; const float* qn; const float* xn;
  const int32_t* ql; const int32_t* xl;
  unsigned long long* key; int32_t* count;
  const unsigned* qbloom; const unsigned* xbloom;
  int nq, n, e, self_exclude, tiles_per_split;
};

// PASS 1: nearest positive per row; PASS 2: negatives in front of it.  grid = (query tiles, gallery splits).
// (two workgroups per CU asked for with the 16-byte loader, where the registers allow it without scratch; the scalar loader of
// unaligned or ragged operands keeps 12 more address registers and runs one workgroup per SIMD at 128x128)
template <class G, bool VEC, int PASS>
__global__ __launch_bounds__(256, VEC ? 2 : 1) void retrieval_walk_kernel(RetrievalParams p) {
  using TA = TileKC<G::BM>;
  using TB = TileKC<G::BN>;
  constexpr int SLOTS = G::TM * 16;                        // rows of the tile this lane holds an element of
  __shared__ __attribute__((aligned(16))) float smem[MAIN_FLOATS<TA, TB>];
  __shared__ float s_qn[G::BM];
  __shared__ int s_ql[G::BM];
  __shared__ unsigned long long s_thr[PASS == 2 ? G::BM : 1];
  prio_hi();
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave / G::WAVES_N) * G::WTM, wn = (wave % G::WAVES_N) * G::WTN;
  const int m0 = blockIdx.x * G::BM;
  const int tiles_n = (p.n + G::BN - 1) / G::BN;
  const int t0 = blockIdx.y * p.tiles_per_split, t1 = min(t0 + p.tiles_per_split, tiles_n);
  const int kt_total = (p.e + BK - 1) / BK;

  for (int i = tid; i < G::BM; i += NTHREADS) {            // the tile's rows: norm, label, pass-1 key
    const int row = min(m0 + i, p.nq - 1);
    s_qn[i] = p.qn[row]; s_ql[i] = p.ql[row];
    if (PASS == 2) s_thr[i] = p.key[row];
  }
  __syncthreads();

  LoadRowsKC<G::BM, VEC> la; la.init(p.q, p.e, p.nq, p.e, m0, tid);
  unsigned qb = 0u;                                        // this lane's word of the query tile's label filter
  if (PASS == 1) qb = p.qbloom[(long)blockIdx.x * BLOOM_WORDS + (lane & 31)];
  unsigned long long best[SLOTS];
  int cnt[SLOTS];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) { best[s] = NO_KEY; cnt[s] = 0; }

  for (int t = t0; t < t1; ++t) {
    const int n0 = t * G::BN;
    if (PASS == 1) {                                       // no label in common: no positive here (the same answer in every wave)
      const unsigned w = qb & p.xbloom[(long)t * BLOOM_WORDS + (lane & 31)];
      if (__ballot(w != 0u) == 0ull) continue;
    }
    LoadRowsKC<G::BN, VEC> lb; lb.init(p.x, p.e, p.n, p.e, n0, tid);
    // the lane's columns: norm and label, requested in front of the main loop that hides them
    float cn[G::TN]; int cl[G::TN]; int cc[G::TN];
#pragma unroll
    for (int in = 0; in < G::TN; ++in) {
      const int col = n0 + wn + 32 * in + (lane & 31);
      cc[in] = col < p.n ? col : -1;                       // -1: past the gallery, never a positive and never counted
      cn[in] = p.xn[min(col, p.n - 1)]; cl[in] = p.xl[min(col, p.n - 1)];
    }
    f32x16 acc[G::TM][G::TN];
    gemm_mainloop<G, TA, TB>(la, lb, 0, kt_total, smem, acc);
#pragma unroll
    for (int im = 0; im < G::TM; ++im)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rt = wm + 32 * im + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const float rn = s_qn[rt]; const int rl = s_ql[rt];
        const int skip = p.self_exclude ? m0 + rt : -1;    // the query's own column
        unsigned long long thr = 0;
        if (PASS == 2) thr = s_thr[rt];
#pragma unroll
        for (int in = 0; in < G::TN; ++in) {
          const float v = rn + cn[in] - 2.f * acc[im][in][r];
          const float d2 = v != v ? INFINITY : fmaxf(v, 0.f);
          const unsigned long long k = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)cc[in];
          const bool live = cc[in] >= 0 && cc[in] != skip;
          if (PASS == 1) {
            if (live && cl[in] == rl && k < best[im * 16 + r]) best[im * 16 + r] = k;
          } else {
            cnt[im * 16 + r] += (live && cl[in] != rl && k < thr) ? 1 : 0;
          }
        }
      }
  }

  // the 32 lanes of a half wave hold the columns of the same rows
#pragma unroll
  for (int im = 0; im < G::TM; ++im)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = m0 + wm + 32 * im + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (PASS == 1) {
        unsigned long long k = best[im * 16 + r];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
          const unsigned long long ok = __shfl_xor(k, o, 64);
          k = ok < k ? ok : k;
        }
        if ((lane & 31) == 0 && row < p.nq && k != NO_KEY) atomicMin(&p.key[row], k);
      } else {
        int c = cnt[im * 16 + r];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if ((lane & 31) == 0 && row < p.nq && c != 0) atomicAdd(&p.count[row], c);
      }
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

// Tile and split choice.  128x128 tiles where they alone put >= 384 workgroups' worth of work on the chip (cross_dist's
// rule), 64x64 below.  The gallery is cut into `splits` ranges of whole tiles so that (query tiles) x splits reaches ~512
// workgroups on the 256 CUs; with many query tiles splits = 1 and a row sees one atomic per wave column per pass.
static void retrieval_plan(int nq, int n, bool& big, int& splits, int& tiles_per_split) {
  big = (long)cdiv(nq, 128) * cdiv(n, 128) >= 384;
  const int b = big ? 128 : 64;
  const int tiles_m = cdiv(nq, b), tiles_n = cdiv(n, b);
  int want = cdiv(512, tiles_m);
  if (want > tiles_n) want = tiles_n;
  tiles_per_split = cdiv(tiles_n, want);
  splits = cdiv(tiles_n, tiles_per_split);
}

static size_t round16(size_t v) { return (v + 15) / 16 * 16; }

// keys u64[nq] | counters i32[nq] | query norms f32[nq] | gallery norms f32[n] | label filters of the query tiles | of the
// gallery tiles (sized for 64-row tiles: 2 bytes per row)
static size_t bloom_bytes(int rows) { return (size_t)cdiv(rows, 64) * BLOOM_WORDS * sizeof(unsigned); }
extern "C" size_t embnet_retrieval_workspace_bytes(int nq, int n) {
  if (nq <= 0 || n <= 0) return 0;
  return round16((size_t)nq * 8) + round16((size_t)nq * 4) + round16((size_t)nq * 4) + round16((size_t)n * 4) +
         bloom_bytes(nq) + bloom_bytes(n);
}

template <class G>
static void retrieval_launch(const RetrievalParams& p, bool vec, int pass, dim3 grid, hipStream_t s) {
  if (pass == 1) {
    if (vec) retrieval_walk_kernel<G, true, 1><<<grid, 256, 0, s>>>(p); else retrieval_walk_kernel<G, false, 1><<<grid, 256, 0, s>>>(p);
  } else {
    if (vec) retrieval_walk_kernel<G, true, 2><<<grid, 256, 0, s>>>(p); else retrieval_walk_kernel<G, false, 2><<<grid, 256, 0, s>>>(p);
  }
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
  if (workspace_bytes < embnet_retrieval_workspace_bytes(nq, n))
    return fail(EMBNET_EWORKSPACE, "retrieval: workspace %zu < %zu bytes", workspace_bytes, embnet_retrieval_workspace_bytes(nq, n));
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)workspace;
  unsigned long long* key = (unsigned long long*)w;  w += round16((size_t)nq * 8);
  int32_t* count = (int32_t*)w;                      w += round16((size_t)nq * 4);
  float* qn = (float*)w;                             w += round16((size_t)nq * 4);
  float* xn = (float*)w;                             w += round16((size_t)n * 4);
  unsigned* qbloom = (unsigned*)w;                   w += bloom_bytes(nq);
  unsigned* xbloom = (unsigned*)w;
  {
    EMBNET_TRACE("embnet::retrieval_prep_kernel", TRACE_BYTES, 4.0 * ((double)nq * e + (double)n * e), s);
    retrieval_prep_kernel<<<cdiv(nq > n ? nq : n, 4), 256, 0, s>>>(q, nq, x, n, e, qn, xn, key, count);
  }
  bool big; int splits, tps; retrieval_plan(nq, n, big, splits, tps);
  const int tile_rows = big ? 128 : 64;
  {
    EMBNET_TRACE("embnet::retrieval_bloom_kernel", TRACE_BYTES, 4.0 * ((double)nq + n), s);
    const int q_tiles = cdiv(nq, tile_rows);
    retrieval_bloom_kernel<<<q_tiles + cdiv(n, tile_rows), 256, 0, s>>>(q_labels, nq, x_labels, n, tile_rows, q_tiles, qbloom, xbloom);
  }
  RetrievalParams p{q, x, qn, xn, q_labels, x_labels, key, count, qbloom, xbloom, nq, n, e, self_exclude ? 1 : 0, tps};
  const bool vec = (e & 3) == 0 && ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(x)) & 15) == 0;
  const dim3 grid(cdiv(nq, tile_rows), splits);
  const double flop = 2.0 * nq * n * e, bytes = 4.0 * ((double)nq * e + (double)n * e) + 16.0 * nq + 8.0 * n;
  using GS = Geom<64, 64, 2, 2>;
  using GL = Geom<128, 128, 2, 2>;
  {
    EMBNET_TRACE_FLOP("embnet::retrieval_walk_kernel<1>", flop, bytes, s);
    if (big) retrieval_launch<GL>(p, vec, 1, grid, s); else retrieval_launch<GS>(p, vec, 1, grid, s);
  }
  {
    EMBNET_TRACE_FLOP("embnet::retrieval_walk_kernel<2>", flop, bytes, s);
    if (big) retrieval_launch<GL>(p, vec, 2, grid, s); else retrieval_launch<GS>(p, vec, 2, grid, s);
  }
  {
    EMBNET_TRACE("embnet::retrieval_finish_kernel", TRACE_BYTES, 24.0 * nq, s);
    retrieval_finish_kernel<<<cdiv(nq, 256), 256, 0, s>>>(key, count, nq, rank, pos_index, pos_d2);
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
