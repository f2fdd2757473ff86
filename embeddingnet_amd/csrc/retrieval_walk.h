// What every walk of the streaming distance GEMM shares (retrieval.hip: Recall@K, MAP@R; kmeans.hip: nearest centre; verification.hip: pair histograms; knn_search.hip: top-k): the key,
// the walk and its epilogue contract, the tile and split plan, the workspace carver and the traced dispatch.
#pragma once
#include "gemm_engine.h"
#include "../../include/embnet.h"

namespace embnet {

constexpr unsigned long long NO_KEY = ~0ull;               // above every key: (+inf, any index) < NO_KEY

// The label filter of one tile of rows: BLOOM_WORDS x 32 bits (retrieval_bloom_kernel, retrieval.hip).
constexpr int BLOOM_WORDS = 32;

// What every walk reads; the kernels' parameter structs embed it.
struct WalkParams {
  const float* q; const float* x; const float* qn; const float* xn;
  const int32_t* ql; const int32_t* xl;
  const unsigned* qbloom; const unsigned* xbloom;
  int nq, n, e, self_exclude, tiles_per_split;
};

// The row of the workgroup's tile of element r of this lane's accumulator block im (C/D map of the 32x32 MFMA: col = lane & 31,
// row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)).  The 32 lanes of a half wave hold the columns of the same rows.
template <class G>
__device__ __forceinline__ int walk_row(int im, int r) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  return (wave / G::WAVES_N) * G::WTM + 32 * im + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
}
__device__ __forceinline__ unsigned long long half_wave_min(unsigned long long k) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) {
    const unsigned long long ok = __shfl_xor(k, o, 64);
    k = ok < k ? ok : k;
  }
  return k;
}
__device__ __forceinline__ int half_wave_sum(int c) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  return c;
}

// The walk: the workgroup's tile of queries (blockIdx.x) against its range of gallery tiles (blockIdx.y).  For every element
// of every tile it hands the epilogue E the key (bits of d2) << 32 | column, `live` (a gallery column that is not the query's
// own) and `same` (the labels agree), and keeps one Slot per row of the lane for it.  E has
//   FILTER, Slot, INIT    FILTER: only positives matter: skip gallery tiles whose label filter shares no bit with the query tile's
//   column(col)           what E needs per gallery column, fetched in front of the main loop that hides the load
//   row(rt)               what E needs per row (rt = walk_row, the row in the tile), handed back to every visit of that row
//   visit(slot value, rt, row value, column value, key, live, same) -> the new slot value
//   half_wave(v), commit(rt, v)   the reduction over the row's lanes; what their first lane does with it for a row below nq
//   tile_done(count)      called by every thread behind the visits of a gallery tile, count = the visited tiles of this walk so
//                         far; without FILTER every wave gets here for every tile, so E may put a barrier in it
// The barrier behind the row prologue also publishes the LDS rows the calling kernel filled for E before the call.
template <class G, bool VEC, class E>
__device__ __forceinline__ void retrieval_walk(const WalkParams& p, const E ep) {
  using TA = TileKC<G::BM>;
  using TB = TileKC<G::BN>;
  __shared__ __attribute__((aligned(16))) float smem[MAIN_FLOATS<TA, TB>];
  __shared__ float s_qn[G::BM];
  __shared__ int s_ql[G::BM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = (wave % G::WAVES_N) * G::WTN;
  const int m0 = blockIdx.x * G::BM;
  const int tiles_n = (p.n + G::BN - 1) / G::BN;
  const int t0 = blockIdx.y * p.tiles_per_split, t1 = min(t0 + p.tiles_per_split, tiles_n);
  const int kt_total = (p.e + BK - 1) / BK;

  for (int i = tid; i < G::BM; i += NTHREADS) {            // the tile's rows: norm and label
    const int row = min(m0 + i, p.nq - 1);
    s_qn[i] = p.qn[row]; s_ql[i] = p.ql[row];
  }
  __syncthreads();

  LoadRowsKC<G::BM, VEC> la; la.init(p.q, p.e, p.nq, p.e, m0, tid);
  unsigned qb = 0u;                                        // this lane's word of the query tile's label filter
  if (E::FILTER) qb = p.qbloom[(long)blockIdx.x * BLOOM_WORDS + (lane & 31)];
  // A plain local array that only this function touches, and visit() a pure function of its element: as a member of E, or
  // handed to E by reference, the 128x128 kernels carry it twice through the tile loop and spill.
  typename E::Slot out[G::TM * 16];
#pragma unroll
  for (int s = 0; s < G::TM * 16; ++s) out[s] = E::INIT;

  for (int t = t0; t < t1; ++t) {
    const int n0 = t * G::BN;
    if (E::FILTER) {                                       // no label in common: no positive here (the same answer in every wave)
      const unsigned w = qb & p.xbloom[(long)t * BLOOM_WORDS + (lane & 31)];
      if (__ballot(w != 0u) == 0ull) continue;
    }
    LoadRowsKC<G::BN, VEC> lb; lb.init(p.x, p.e, p.n, p.e, n0, tid);
    // the lane's columns: norm and label, requested in front of the main loop that hides them
    float cn[G::TN]; int cl[G::TN]; int cc[G::TN]; int cx[G::TN];
#pragma unroll
    for (int in = 0; in < G::TN; ++in) {
      const int col = n0 + wn + 32 * in + (lane & 31);
      cc[in] = col < p.n ? col : -1;                       // -1: past the gallery, never a positive and never counted
      cn[in] = p.xn[min(col, p.n - 1)]; cl[in] = p.xl[min(col, p.n - 1)];
      cx[in] = ep.column(min(col, p.n - 1));
    }
    f32x16 acc[G::TM][G::TN];
    gemm_mainloop<G, TA, TB>(la, lb, 0, kt_total, smem, acc);
#pragma unroll
    for (int im = 0; im < G::TM; ++im)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rt = walk_row<G>(im, r);
        const float rn = s_qn[rt]; const int rl = s_ql[rt];
        const int skip = p.self_exclude ? m0 + rt : -1;    // the query's own column
        const auto rv = ep.row(rt);
#pragma unroll
        for (int in = 0; in < G::TN; ++in) {
          const float v = rn + cn[in] - 2.f * acc[im][in][r];
          const float d2 = v != v ? INFINITY : fmaxf(v, 0.f);
          const unsigned long long k = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)cc[in];
          const bool live = cc[in] >= 0 && cc[in] != skip;
          out[im * 16 + r] = ep.visit(out[im * 16 + r], rt, rv, cx[in], k, live, cl[in] == rl);
        }
      }
    ep.tile_done(t - t0 + 1);
  }

#pragma unroll
  for (int im = 0; im < G::TM; ++im)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const auto v = E::half_wave(out[im * 16 + r]);
      const int rt = walk_row<G>(im, r);
      if ((lane & 31) == 0 && m0 + rt < p.nq) ep.commit(rt, v);
    }
}

// What an epilogue gets unless it says otherwise: an integer count per row, summed over the half wave; nothing to fetch per
// column or per row, nothing to commit.
struct WalkEpilogue {
  static constexpr bool FILTER = false;
  using Slot = int;
  static constexpr Slot INIT = 0;
  __device__ __forceinline__ int column(int) const { return 0; }
  __device__ __forceinline__ int row(int) const { return 0; }
  __device__ static __forceinline__ int half_wave(int c) { return half_wave_sum(c); }
  __device__ __forceinline__ void commit(int, int) const {}
  __device__ __forceinline__ void tile_done(int) const {}
};

// Tile and split choice.  128x128 tiles where they alone put >= 384 workgroups' worth of work on the chip (cross_dist's
// rule), 64x64 below.  The gallery is cut into `splits` ranges of whole tiles so that (query tiles) x splits reaches ~512
// workgroups on the 256 CUs; with many query tiles splits = 1 and a row sees one atomic per wave column per pass.
// (plan_splits: the split rule for b x b tiles, for a walk that has one geometry only — knn_search.hip)
static void plan_splits(int nq, int n, int b, int& splits, int& tiles_per_split) {
  const int tiles_m = cdiv(nq, b), tiles_n = cdiv(n, b);
  int want = cdiv(512, tiles_m);
  if (want > tiles_n) want = tiles_n;
  tiles_per_split = cdiv(tiles_n, want);
  splits = cdiv(tiles_n, tiles_per_split);
}
static void retrieval_plan(int nq, int n, bool& big, int& splits, int& tiles_per_split) {
  big = (long)cdiv(nq, 128) * cdiv(n, 128) >= 384;
  plan_splits(nq, n, big ? 128 : 64, splits, tiles_per_split);
}

// A workspace handed out from the front in 16-byte steps.  Without a base it only adds up, so the constructor that carves a
// workspace is also the one that sizes it.
struct Bump {
  char* base; size_t used = 0;
  template <class T> T* take(size_t count) {
    T* at = base ? (T*)(base + used) : nullptr;
    used += (count * sizeof(T) + 15) / 16 * 16;
    return at;
  }
  unsigned* take_bloom(int rows) { return take<unsigned>((size_t)cdiv(rows, 64) * BLOOM_WORDS); }   // sized for 64-row tiles
};

struct WalkSetup { WalkParams w; bool big, vec; dim3 grid; };

// One traced walk: launch(geometry, loader, pass), as types, for the instantiation that the setup and `pass` (1 or 2) select.
// `extra_bytes`: what the family moves on top of the two embedding blocks.
template <class F>
static void walk_dispatch(const WalkSetup& su, int pass, const char* trace_name, double extra_bytes, hipStream_t s, F launch) {
  const double rows = (double)su.w.nq + su.w.n;
  EMBNET_TRACE_FLOP(trace_name, 2.0 * su.w.nq * su.w.n * su.w.e, 4.0 * rows * su.w.e + extra_bytes, s);
  auto by_pass = [&](auto g, auto vec) {
    if (pass == 1) launch(g, vec, std::integral_constant<int, 1>{}); else launch(g, vec, std::integral_constant<int, 2>{});
  };
  auto by_loader = [&](auto g) { if (su.vec) by_pass(g, std::true_type{}); else by_pass(g, std::false_type{}); };
  if (su.big) by_loader(Geom<128, 128, 2, 2>{}); else by_loader(Geom<64, 64, 2, 2>{});
}

}  // namespace embnet
