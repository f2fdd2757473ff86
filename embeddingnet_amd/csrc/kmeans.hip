// Lloyd's k-means on encodings: nearest-centre assignment, centre update and k-means++ seeding (include/embnet.h, "k-means").
//
// ASSIGN is retrieval_walk (retrieval_walk.h) with the points as its queries and the centres as its gallery: the same d2 =
// fmaxf(|x|^2 + |c|^2 - 2 g, 0) from the fp32 MFMA chain, NaN as +inf, the same 64-bit key (bits of d2) << 32 | centre.  The
// epilogue NearestColumn keeps the smallest key over all live columns: an exact argmin with ties to the smaller centre index,
// merged across gallery splits by a 64-bit atomicMin — a minimum, so bitwise reproducible; no [n, k] matrix is formed.
//   prep:   point norms (once per fit) and centre norms (every pass), keys back to NO_KEY, the walk's label array to zero
//   walk:   key[i] = min over the centres
//   finish: labels / d2 from the key, the labels that differ from the previous pass (integer atomic), per-block f64 inertia
//   total:  the block partials folded by one workgroup in a fixed order
// UPDATE sums every cluster's rows in an order that depends on (n, e, k, labels) alone:
//   zero, hist:   count[j] by integer atomics
//   scan:         offset = exclusive scan of count; chunk_off = exclusive scan of ceil(count / CHUNK_ROWS)
//   scatter:      point indices into their cluster's segment through an atomic cursor — any order
//   order:        each segment ascending by index: up to SORT_MAX in LDS (a set of distinct integers: the sorted segment is unique);
//                 a larger cluster does not sort, it re-derives its list from the label array in index order (ballot ranks)
//   accumulate:   one workgroup per (chunk of CHUNK_ROWS segment rows, 64 columns): wave w adds rows w, w + 4, .. of the chunk
//                 in f64 in that order, the four waves are folded 0..3 -> partial[chunk][column]
//   finalize:     one workgroup per cluster: its chunks' partials in chunk order, / count, rounded to f32 once; an empty cluster
//                 keeps its centre's bits; the cluster's |new - old|^2 in f64
//   total:        shift and n_empty folded by one workgroup in a fixed order
// No float atomics anywhere.  A cluster of any size is cut into chunks, so one huge cluster is as parallel as many small ones.
// SEEDING (k-means++, plain D^2 sampling): pp_update streams x once per chosen row; pp_pick is one workgroup: the f64 prefix
// sums of the weights in a fixed two-level order and the first positive-weight index whose prefix exceeds u * total.
// Roofline: assign 2*n*k*e FLOP on the fp32 MFMA, O((n + k) e) bytes; update one read of x (4 n e bytes) plus O(n + k e).
#include "retrieval_walk.h"

namespace embnet {

constexpr int CHUNK_ROWS = 512;                            // segment rows per accumulate workgroup
constexpr int SORT_MAX = 2048;                             // the largest segment sorted in LDS (2048 x 4 B)
constexpr int COL_BLOCK = 64;                              // columns per accumulate workgroup: one per lane

// one wave per row, in retrieval_prep_kernel's idiom.  zero_labels: what the walk reads as ql / xl (max(n, k) entries)
__global__ __launch_bounds__(256) void kmeans_prep_kernel(const float* __restrict__ x, int n, const float* __restrict__ c, int k,
                                                          int e, int point_norms, float* __restrict__ xn, float* __restrict__ cn,
                                                          unsigned long long* __restrict__ key, int32_t* __restrict__ zero_labels,
                                                          int32_t* __restrict__ changed) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row == 0 && lane == 0) *changed = 0;
  if (row < n) {
    if (point_norms) {
      const float s = row_sqnorm(x + (long)row * e, e);
      if (lane == 0) xn[row] = s;
    }
    if (lane == 0) { key[row] = NO_KEY; zero_labels[row] = 0; }
  }
  if (row < k) {
    const float s = row_sqnorm(c + (long)row * e, e);
    if (lane == 0) { cn[row] = s; zero_labels[row] = 0; }
  }
}

// the smallest key over all live columns of the row (key: of the tile's first row); the labels play no part
struct NearestColumn : WalkEpilogue {
  using Slot = unsigned long long;
  static constexpr Slot INIT = NO_KEY;
  unsigned long long* key;
  __device__ __forceinline__ Slot visit(Slot best, int, int, int, unsigned long long k, bool live, bool) const {
    return (live && k < best) ? k : best;
  }
  __device__ static __forceinline__ Slot half_wave(Slot k) { return half_wave_min(k); }
  __device__ __forceinline__ void commit(int rt, Slot k) const { if (k != NO_KEY) atomicMin(&key[rt], k); }
};

struct AssignParams {
  WalkParams w;
  unsigned long long* key;
};

// grid = (point tiles, centre splits).  One workgroup per CU behind the scalar loader, as retrieval_walk_kernel's pass 1, which
// carries the same 64-bit slots.
template <class G, bool VEC>
__global__ __launch_bounds__(256, VEC ? 2 : 1) void kmeans_assign_kernel(AssignParams p) {
  prio_hi();
  retrieval_walk<G, VEC>(p.w, NearestColumn{{}, p.key + blockIdx.x * G::BM});
}

// 256 points per workgroup.  A point without a finite distance has the key (+inf, 0) or NO_KEY: label 0 either way.
__global__ __launch_bounds__(256) void kmeans_finish_kernel(const unsigned long long* __restrict__ key, int n, int k,
                                                            const int32_t* __restrict__ labels_prev, int32_t* __restrict__ labels,
                                                            float* __restrict__ d2, int32_t* __restrict__ changed,
                                                            double* __restrict__ part) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  double d = 0.0; int diff = 0;
  if (i < n) {
    const unsigned long long kk = key[i];
    const unsigned col = (unsigned)(kk & 0xffffffffull);
    const int label = (kk == NO_KEY || col >= (unsigned)k) ? 0 : (int)col;
    const float dist = kk == NO_KEY ? INFINITY : __uint_as_float((unsigned)(kk >> 32));
    labels[i] = label; d2[i] = dist;
    d = (double)dist;
    diff = labels_prev ? (labels_prev[i] != label ? 1 : 0) : 1;
  }
  diff = wave_sum(diff);
  if ((threadIdx.x & 63) == 0 && diff != 0) atomicAdd(changed, diff);
  d = block_sum256(d);
  if (threadIdx.x == 0) part[blockIdx.x] = d;
}

// *out = the sum of part[0 .. count) : one workgroup, strided partial sums folded in a fixed order (retrieval_reduce_kernel's)
__global__ __launch_bounds__(1024) void kmeans_total_kernel(const double* __restrict__ part, int count, double* __restrict__ out) {
  __shared__ double s_sum[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double s = 0.0;
  for (int i = tid; i < count; i += 1024) s += part[i];
  s = wave_sum(s);
  if (lane == 0) s_sum[wave] = s;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t += s_sum[w];
    *out = t;
  }
}

// ---- update ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kmeans_zero_kernel(int32_t* __restrict__ count, int32_t* __restrict__ cursor, int k) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < k) { count[i] = 0; cursor[i] = 0; }
}

// a label outside [0, k) belongs to no cluster: it is left out here and in the scatter, so nothing is addressed through it
__global__ __launch_bounds__(256) void kmeans_hist_kernel(const int32_t* __restrict__ labels, int n, int k, int32_t* __restrict__ count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const int l = labels[i];
    if ((unsigned)l < (unsigned)k) atomicAdd(&count[l], 1);
  }
}

// offset[j] = exclusive scan of count, chunk_off[j] = exclusive scan of ceil(count / CHUNK_ROWS); one workgroup, thread t owns a
// contiguous run of clusters (map_scan_kernel's shape)
__global__ __launch_bounds__(1024) void kmeans_scan_kernel(const int32_t* __restrict__ count, int k, int32_t* __restrict__ offset,
                                                           int32_t* __restrict__ chunk_off) {
  __shared__ int s_a[16], s_b[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int run = (k + 1023) / 1024;
  const int j0 = min((long)tid * run, (long)k), j1 = min((long)j0 + run, (long)k);
  int sa = 0, sb = 0;
  for (int j = j0; j < j1; ++j) { const int c = count[j]; sa += c; sb += (c + CHUNK_ROWS - 1) / CHUNK_ROWS; }
  int ia = sa, ib = sb;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int ua = __shfl_up(ia, o, 64), ub = __shfl_up(ib, o, 64);
    if (lane >= o) { ia += ua; ib += ub; }
  }
  if (lane == 63) { s_a[wave] = ia; s_b[wave] = ib; }
  __syncthreads();
  int ba = 0, bb = 0, ta = 0, tb = 0;
  for (int w = 0; w < 16; ++w) { if (w < wave) { ba += s_a[w]; bb += s_b[w]; } ta += s_a[w]; tb += s_b[w]; }
  int a = ba + ia - sa, b = bb + ib - sb;
  for (int j = j0; j < j1; ++j) {
    offset[j] = a; chunk_off[j] = b;
    const int c = count[j];
    a += c; b += (c + CHUNK_ROWS - 1) / CHUNK_ROWS;
  }
  if (tid == 0) { offset[k] = ta; chunk_off[k] = tb; }
}

// clusters above SORT_MAX are placed by kmeans_order_kernel from the labels themselves
__global__ __launch_bounds__(256) void kmeans_scatter_kernel(const int32_t* __restrict__ labels, int n, int k,
                                                             const int32_t* __restrict__ count, const int32_t* __restrict__ offset,
                                                             int32_t* __restrict__ cursor, int32_t* __restrict__ perm) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int l = labels[i];
  if ((unsigned)l >= (unsigned)k) return;
  const int c = count[l];
  if (c > SORT_MAX) return;
  const int slot = atomicAdd(&cursor[l], 1);
  if (slot < c) perm[offset[l] + slot] = i;                // slot < c always; the guard keeps the address inside the segment
}

// one workgroup per cluster: its segment of perm ascending by point index
__global__ __launch_bounds__(256) void kmeans_order_kernel(const int32_t* __restrict__ labels, int n,
                                                           const int32_t* __restrict__ count, const int32_t* __restrict__ offset,
                                                           int32_t* __restrict__ perm) {
  __shared__ int s[SORT_MAX];
  __shared__ int s_wave[4];
  const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = count[j], off = offset[j];                 // the same in every thread: the barriers below are uniform
  if (c <= 1 || off < 0 || (long)off + c > n) return;
  if (c <= SORT_MAX) {
    int P = 2;
    while (P < c) P <<= 1;
    for (int i = tid; i < P; i += 256) s[i] = i < c ? perm[off + i] : 0x7fffffff;
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1)
      for (int jj = kk >> 1; jj > 0; jj >>= 1) {
        for (int i = tid; i < P; i += 256) {
          const int o = i ^ jj;
          if (o > i) {
            const int a = s[i], b = s[o];
            if (((i & kk) == 0) == (a > b)) { s[i] = b; s[o] = a; }
          }
        }
        __syncthreads();
      }
    for (int i = tid; i < c; i += 256) perm[off + i] = s[i];
    return;
  }
  int base = 0;                                            // members of the cluster in front of this round's 256 points
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + tid;
    const bool mine = i < n && labels[i] == j;
    const unsigned long long m = __ballot(mine);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int before = __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    const int round = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    if (mine && base + before < c) perm[off + base + before] = i;
    base += round;
    __syncthreads();                                       // s_wave has been read
  }
}

// the cluster of chunk `chunk`: the last j with chunk_off[j] <= chunk (empty clusters share their successor's value)
__device__ __forceinline__ int kmeans_chunk_cluster(const int32_t* chunk_off, int k, int chunk) {
  int lo = 0, hi = k - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (chunk_off[mid] <= chunk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// grid = (chunks, column blocks), chunks the upper bound ceil(n / CHUNK_ROWS) + min(n, k): a workgroup past the real number leaves.
// Wave w sums rows w, w + 4, .. of the chunk in that order (four loads in flight, added in row order); lane = column.
__global__ __launch_bounds__(256) void kmeans_accumulate_kernel(const float* __restrict__ x, int n, int e, int k,
                                                                const int32_t* __restrict__ count, const int32_t* __restrict__ offset,
                                                                const int32_t* __restrict__ chunk_off,
                                                                const int32_t* __restrict__ perm, double* __restrict__ partial) {
  __shared__ double s_part[4][COL_BLOCK];
  const int chunk = blockIdx.x;
  if (chunk >= chunk_off[k]) return;
  const int j = kmeans_chunk_cluster(chunk_off, k, chunk);
  const int r0 = (chunk - chunk_off[j]) * CHUNK_ROWS;
  const int rows = min(count[j] - r0, CHUNK_ROWS);
  const int32_t* seg = perm + offset[j] + r0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = blockIdx.y * COL_BLOCK + lane;
  const bool in = col < e;
  double s = 0.0;
  int r = wave;
  for (; r + 12 < rows; r += 16) {
    const int i0 = seg[r], i1 = seg[r + 4], i2 = seg[r + 8], i3 = seg[r + 12];
    const bool ok = (unsigned)i0 < (unsigned)n && (unsigned)i1 < (unsigned)n && (unsigned)i2 < (unsigned)n && (unsigned)i3 < (unsigned)n;
    if (in && ok) {
      const float v0 = x[(long)i0 * e + col], v1 = x[(long)i1 * e + col], v2 = x[(long)i2 * e + col], v3 = x[(long)i3 * e + col];
      s += (double)v0; s += (double)v1; s += (double)v2; s += (double)v3;
    }
  }
  for (; r < rows; r += 4) {
    const int i0 = seg[r];
    if (in && (unsigned)i0 < (unsigned)n) s += (double)x[(long)i0 * e + col];
  }
  s_part[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && in) partial[(long)chunk * e + col] = ((s_part[0][lane] + s_part[1][lane]) + s_part[2][lane]) + s_part[3][lane];
}

// one workgroup per cluster.  centres_out may be centres: a thread reads the element it writes.
__global__ __launch_bounds__(256) void kmeans_finalize_kernel(const float* __restrict__ centres, int k, int e,
                                                              const int32_t* __restrict__ count, const int32_t* __restrict__ chunk_off,
                                                              const double* __restrict__ partial, float* centres_out,
                                                              double* __restrict__ shift_part) {
  const int j = blockIdx.x;
  const int c = count[j], ch0 = chunk_off[j], ch1 = chunk_off[j + 1];
  double d = 0.0;
  for (int col = threadIdx.x; col < e; col += 256) {
    const float old = centres[(long)j * e + col];
    float now = old;
    if (c > 0) {
      double s = 0.0;
      for (int ch = ch0; ch < ch1; ++ch) s += partial[(long)ch * e + col];
      now = (float)(s / (double)c);
    }
    centres_out[(long)j * e + col] = now;
    const double t = (double)now - (double)old;
    d = fma(t, t, d);
  }
  d = block_sum256(d);
  if (threadIdx.x == 0) shift_part[j] = c > 0 ? d : 0.0;
}

__global__ __launch_bounds__(1024) void kmeans_update_total_kernel(const double* __restrict__ shift_part, const int32_t* __restrict__ count,
                                                                   int k, double* __restrict__ shift, int32_t* __restrict__ n_empty) {
  __shared__ double s_sum[16];
  __shared__ int s_cnt[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double s = 0.0; int empty = 0;
  for (int j = tid; j < k; j += 1024) { s += shift_part[j]; empty += count[j] == 0 ? 1 : 0; }
  s = wave_sum(s); empty = wave_sum(empty);
  if (lane == 0) { s_sum[wave] = s; s_cnt[wave] = empty; }
  __syncthreads();
  if (tid == 0) {
    double t = 0.0; int te = 0;
    for (int w = 0; w < 16; ++w) { t += s_sum[w]; te += s_cnt[w]; }
    *shift = t; *n_empty = te;
  }
}

// ---- k-means++ seeding ----------------------------------------------------------------------------------------------------
// one wave per row: |x_i - x_c|^2 by row_sqnorm's chain on the difference (lane-strided fma, wave_sum); c = *index
__global__ __launch_bounds__(256) void kmeans_pp_update_kernel(const float* __restrict__ x, int n, int e,
                                                               const int32_t* __restrict__ index, int first,
                                                               float* __restrict__ mind2) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;
  const int c = min(max(*index, 0), n - 1);
  const float* a = x + (long)row * e;
  const float* b = x + (long)c * e;
  float s = 0.f;
  for (int kk = lane; kk < e; kk += 64) { const float t = a[kk] - b[kk]; s = fmaf(t, t, s); }
  s = wave_sum(s);
  if (lane == 0) mind2[row] = first ? s : fminf(mind2[row], s);
}

__device__ __forceinline__ double pp_weight(float m) { return (m > 0.f && m < INFINITY) ? (double)m : 0.0; }

// One workgroup.  draw 0: *index = rng_u32(seed, 0, 0) mod n, *u = 0.  draw j >= 1: u from 53 bits of two keyed words; thread t
// sums its contiguous run of weights (level 1), the run sums are scanned over the wave and the 16 waves (level 2); the prefix
// of row i is its run's exclusive prefix plus the running sum inside the run.  *index = the first row of positive weight
// whose prefix exceeds u * total (if rounding leaves none: the last row of positive weight); total == 0: floor(u * n).
__global__ __launch_bounds__(1024) void kmeans_pp_pick_kernel(const float* __restrict__ mind2, int n, uint64_t seed, int draw,
                                                              int32_t* __restrict__ index, double* __restrict__ u_out) {
  __shared__ double s_wave[16];
  __shared__ int s_first, s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (draw <= 0) {
    if (tid == 0) { *index = (int32_t)(rng_u32(seed, 0, 0) % (uint32_t)n); *u_out = 0.0; }
    return;
  }
  const uint64_t bits = ((uint64_t)rng_u32(seed, (uint64_t)draw, 0) << 32) | rng_u32(seed, (uint64_t)draw, 1);
  const double u = (double)(bits >> 11) * 0x1p-53;
  if (tid == 0) { s_first = n; s_last = -1; }
  const int run = (n + 1023) / 1024;
  const int i0 = min((long)tid * run, (long)n), i1 = min((long)i0 + run, (long)n);
  double sum = 0.0;
  for (int i = i0; i < i1; ++i) sum += pp_weight(mind2[i]);
  double incl = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  double excl = __shfl_up(incl, 1, 64);
  if (lane == 0) excl = 0.0;
  if (lane == 63) s_wave[wave] = incl;
  __syncthreads();
  double base = 0.0, total = 0.0;
  for (int w = 0; w < 16; ++w) { if (w < wave) base += s_wave[w]; total += s_wave[w]; }
  if (total > 0.0) {
    const double target = u * total;
    double cum = base + excl;
    int first = n, last = -1;
    for (int i = i0; i < i1; ++i) {
      const double w = pp_weight(mind2[i]);
      cum += w;
      if (w > 0.0) { last = i; if (first == n && cum > target) first = i; }
    }
    if (first < n) atomicMin(&s_first, first);
    if (last >= 0) atomicMax(&s_last, last);
  }
  __syncthreads();
  if (tid == 0) {
    int pick;
    if (total > 0.0) pick = s_first < n ? s_first : s_last;
    else pick = (int)(u * (double)n);
    *index = min(max(pick, 0), n - 1);
    *u_out = u;
  }
}

}  // namespace embnet

using namespace embnet;

static int kmeans_max_chunks(int n, int k) { return cdiv(n, CHUNK_ROWS) + (k < n ? k : n); }

struct KMeansWorkspace {
  unsigned long long* key; double* part; double* shift_part; double* partial;
  float* xn; float* cn; int32_t* zero_labels; int32_t* offset; int32_t* chunk_off; int32_t* cursor; int32_t* perm;
  size_t bytes;
  KMeansWorkspace(void* base, int n, int k, int e) {
    Bump b{(char*)base};
    key = b.take<unsigned long long>(n); part = b.take<double>(cdiv(n, 256)); shift_part = b.take<double>(k);
    partial = b.take<double>((size_t)kmeans_max_chunks(n, k) * e);
    xn = b.take<float>(n); cn = b.take<float>(k); zero_labels = b.take<int32_t>(n > k ? n : k);
    offset = b.take<int32_t>((size_t)k + 1); chunk_off = b.take<int32_t>((size_t)k + 1); cursor = b.take<int32_t>(k);
    perm = b.take<int32_t>(n);
    bytes = b.used;
  }
};
extern "C" size_t embnet_kmeans_workspace_bytes(int n, int k, int e) {
  return n <= 0 || k <= 0 || e <= 0 || k > n ? 0 : KMeansWorkspace(nullptr, n, k, e).bytes;
}

#define KMEANS_CHECK_SHAPE(who)                                                                                              \
  EMBNET_CHECK_ARG(n > 0 && k > 0 && e > 0, who ": n=%d k=%d e=%d must be positive", n, k, e);                               \
  EMBNET_CHECK_ARG(k <= n, who ": k=%d exceeds n=%d", k, n);                                                                 \
  EMBNET_CHECK_ARG((size_t)n * e * 4 <= MAX_OPERAND_BYTES && (size_t)k * e * 4 <= MAX_OPERAND_BYTES,                         \
                   who ": an embedding block exceeds 2 GiB");                                                                \
  EMBNET_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, who ": workspace must be 16-byte aligned")

extern "C" int embnet_kmeans_assign(const float* x, int n, const float* centres, int k, int e, int reuse_point_norms,
                                    const int32_t* labels_prev, int32_t* labels, float* d2, int32_t* changed, double* inertia,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  EMBNET_CHECK_ARG(x && centres && labels && d2 && changed && inertia && workspace, "kmeans_assign: null pointer");
  KMEANS_CHECK_SHAPE("kmeans_assign");
  EMBNET_CHECK_ARG((reinterpret_cast<uintptr_t>(inertia) & 7) == 0, "kmeans_assign: inertia must be 8-byte aligned");
  const KMeansWorkspace w(workspace, n, k, e);
  if (workspace_bytes < w.bytes) return fail(EMBNET_EWORKSPACE, "kmeans_assign: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream;
  {
    EMBNET_TRACE("embnet::kmeans_prep_kernel", TRACE_BYTES, 4.0 * ((reuse_point_norms ? 0.0 : (double)n * e) + (double)k * e) + 16.0 * n, s);
    kmeans_prep_kernel<<<cdiv(n, 4), 256, 0, s>>>(x, n, centres, k, e, reuse_point_norms ? 0 : 1, w.xn, w.cn, w.key, w.zero_labels,
                                                  changed);
  }
  WalkSetup su{{x, centres, w.xn, w.cn, w.zero_labels, w.zero_labels, nullptr, nullptr, n, k, e, 0, 0}};
  int splits;
  retrieval_plan(n, k, su.big, splits, su.w.tiles_per_split);
  su.vec = (e & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(centres)) & 15) == 0;
  su.grid = dim3(cdiv(n, su.big ? 128 : 64), splits);
  const AssignParams p{su.w, w.key};
  walk_dispatch(su, 1, "embnet::kmeans_assign_kernel", 12.0 * n + 4.0 * k, s, [&](auto g, auto vec, auto) {
    kmeans_assign_kernel<decltype(g), decltype(vec)::value><<<su.grid, 256, 0, s>>>(p);
  });
  const int blocks = cdiv(n, 256);
  {
    EMBNET_TRACE("embnet::kmeans_finish_kernel", TRACE_BYTES, (labels_prev ? 20.0 : 16.0) * n, s);
    kmeans_finish_kernel<<<blocks, 256, 0, s>>>(w.key, n, k, labels_prev, labels, d2, changed, w.part);
  }
  {
    EMBNET_TRACE("embnet::kmeans_total_kernel", TRACE_BYTES, 8.0 * blocks, s);
    kmeans_total_kernel<<<1, 1024, 0, s>>>(w.part, blocks, inertia);
  }
  return check_launch("kmeans_assign");
}

extern "C" int embnet_kmeans_update(const float* x, const int32_t* labels, int n, const float* centres, int k, int e,
                                    float* centres_out, int32_t* count, double* shift, int32_t* n_empty,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  EMBNET_CHECK_ARG(x && labels && centres && centres_out && count && shift && n_empty && workspace, "kmeans_update: null pointer");
  KMEANS_CHECK_SHAPE("kmeans_update");
  EMBNET_CHECK_ARG((reinterpret_cast<uintptr_t>(shift) & 7) == 0, "kmeans_update: shift must be 8-byte aligned");
  const KMeansWorkspace w(workspace, n, k, e);
  if (workspace_bytes < w.bytes) return fail(EMBNET_EWORKSPACE, "kmeans_update: workspace %zu < %zu bytes", workspace_bytes, w.bytes);
  hipStream_t s = (hipStream_t)stream;
  {
    EMBNET_TRACE("embnet::kmeans_zero_kernel", TRACE_BYTES, 8.0 * k, s);
    kmeans_zero_kernel<<<cdiv(k, 256), 256, 0, s>>>(count, w.cursor, k);
  }
  {
    EMBNET_TRACE("embnet::kmeans_hist_kernel", TRACE_BYTES, 8.0 * n, s);
    kmeans_hist_kernel<<<cdiv(n, 256), 256, 0, s>>>(labels, n, k, count);
  }
  {
    EMBNET_TRACE("embnet::kmeans_scan_kernel", TRACE_BYTES, 12.0 * k, s);
    kmeans_scan_kernel<<<1, 1024, 0, s>>>(count, k, w.offset, w.chunk_off);
  }
  {
    EMBNET_TRACE("embnet::kmeans_scatter_kernel", TRACE_BYTES, 16.0 * n, s);
    kmeans_scatter_kernel<<<cdiv(n, 256), 256, 0, s>>>(labels, n, k, count, w.offset, w.cursor, w.perm);
  }
  {
    EMBNET_TRACE("embnet::kmeans_order_kernel", TRACE_BYTES, 8.0 * n + 8.0 * k, s);
    kmeans_order_kernel<<<k, 256, 0, s>>>(labels, n, count, w.offset, w.perm);
  }
  {
    EMBNET_TRACE("embnet::kmeans_accumulate_kernel", TRACE_BYTES, 4.0 * n * e + 4.0 * n, s);
    kmeans_accumulate_kernel<<<dim3(kmeans_max_chunks(n, k), cdiv(e, COL_BLOCK)), 256, 0, s>>>(x, n, e, k, count, w.offset, w.chunk_off,
                                                                                             w.perm, w.partial);
  }
  {
    EMBNET_TRACE("embnet::kmeans_finalize_kernel", TRACE_BYTES, 8.0 * k * e + 8.0 * ((double)cdiv(n, CHUNK_ROWS) + k) * e, s);
    kmeans_finalize_kernel<<<k, 256, 0, s>>>(centres, k, e, count, w.chunk_off, w.partial, centres_out, w.shift_part);
  }
  {
    EMBNET_TRACE("embnet::kmeans_update_total_kernel", TRACE_BYTES, 12.0 * k, s);
    kmeans_update_total_kernel<<<1, 1024, 0, s>>>(w.shift_part, count, k, shift, n_empty);
  }
  return check_launch("kmeans_update");
}

extern "C" int embnet_kmeans_pp_update(const float* x, int n, int e, const int32_t* index, int first, float* mind2, void* stream) {
  EMBNET_CHECK_ARG(x && index && mind2, "kmeans_pp_update: null pointer");
  EMBNET_CHECK_ARG(n > 0 && e > 0, "kmeans_pp_update: n=%d e=%d must be positive", n, e);
  EMBNET_CHECK_ARG((size_t)n * e * 4 <= MAX_OPERAND_BYTES, "kmeans_pp_update: an embedding block exceeds 2 GiB");
  hipStream_t s = (hipStream_t)stream;
  EMBNET_TRACE("embnet::kmeans_pp_update_kernel", TRACE_BYTES, 4.0 * n * e + 8.0 * n, s);
  kmeans_pp_update_kernel<<<cdiv(n, 4), 256, 0, s>>>(x, n, e, index, first ? 1 : 0, mind2);
  return check_launch("kmeans_pp_update");
}

extern "C" int embnet_kmeans_pp_pick(const float* mind2, int n, uint64_t seed, int draw, int32_t* index, double* u, void* stream) {
  EMBNET_CHECK_ARG(index && u && (mind2 || draw == 0), "kmeans_pp_pick: null pointer");
  EMBNET_CHECK_ARG(n > 0 && draw >= 0, "kmeans_pp_pick: n=%d must be positive and draw=%d non-negative", n, draw);
  EMBNET_CHECK_ARG((reinterpret_cast<uintptr_t>(u) & 7) == 0, "kmeans_pp_pick: u must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  EMBNET_TRACE("embnet::kmeans_pp_pick_kernel", TRACE_BYTES, draw ? 8.0 * n : 12.0, s);
  kmeans_pp_pick_kernel<<<1, 1024, 0, s>>>(mind2, n, seed, draw, index, u);
  return check_launch("kmeans_pp_pick");
}
