// One launch updates every trainable tensor of a model with the update rule of the Keras optimizer the
// reference builds in /root/reference/embedding_net/utils.py:143-153 (SGD / Adam / RMSprop / keras_radam RAdam,
// library defaults, only `lr` passed).  Multi-tensor (multi_tensor.h) over a table of {w, g, slot1, slot2, n}
// descriptors, so the step is one kernel instead of ~10 framework launches per rule (ResNet18: 62 tensors,
// 11.3 M floats).  HBM-bound: 4 B/element x (w r+w, g r, slots r+w) = 12..28 B/element.
// The scalar coefficients (bias corrections, RAdam's rectifier) are computed on the host in double and passed in;
// the arithmetic per element is the rule's own order in fp32.
// l2x2 = 2*lambda of the tensor's kernel_regularizer=l2(lambda) (backbones.py:22-36; 0 for none): the regulariser's
// gradient 2*lambda*w is added to g here, which is what Keras' loss + regulariser differentiates to, so no separate
// 2*lambda*w tensors or accumulation launches exist.
#include "common.h"
#include "multi_tensor.h"
#include "../../include/embnet.h"

namespace embnet {

struct OptTensor { float* w; const float* g; float* s1; float* s2; long n; float l2x2; int group; };   // group: embnet_optimizer_step_groups only
static_assert(sizeof(OptTensor) == 48, "descriptor layout is part of the ABI (include/embnet.h)");

struct OptCoef { float lr, b1, b2, eps, c1, c2; };

template <int RULE>
__device__ __forceinline__ void opt_update(float& w, float g, float& s1, float& s2, const OptCoef& k) {
  if (RULE == EMBNET_OPT_SGD) {
    w -= k.lr * g;
  } else if (RULE == EMBNET_OPT_RMSPROP) {                 // rms <- rho rms + (1-rho) g^2; w -= lr g / (sqrt(rms) + eps)
    s1 = k.b1 * s1 + (1.f - k.b1) * g * g;
    w -= k.lr * g / (sqrtf(s1) + k.eps);
  } else {
    s1 = k.b1 * s1 + (1.f - k.b1) * g;                     // m
    s2 = k.b2 * s2 + (1.f - k.b2) * g * g;                 // v
    if (RULE == EMBNET_OPT_ADAM) w -= k.c1 * s1 / (sqrtf(s2) + k.eps);                    // c1 = lr sqrt(1-b2^t)/(1-b1^t)
    else if (RULE == EMBNET_OPT_RADAM) w -= k.c1 * s1 / (sqrtf(s2 * k.c2) + k.eps);       // c1 = lr r_t/(1-b1^t), c2 = 1/(1-b2^t)
    else w -= k.c1 * s1;                                                                   // RAdam before rectification: c1 = lr/(1-b1^t)
  }
}

// One workgroup's chunk of one tensor under an update rule: mt_walk's float4 path where the chunk is whole and every pointer
// 16-byte aligned, element by element on tails and unaligned tensors.  update(w, g', slot1, slot2), g' = fma(l2x2, w, g).
template <int RULE, class Update>
__device__ __forceinline__ void opt_walk(const OptTensor& t, long first, Update update) {
  constexpr bool S1 = RULE != EMBNET_OPT_SGD, S2 = RULE >= EMBNET_OPT_ADAM && RULE <= EMBNET_OPT_RADAM_WARM;
  const bool vec = (((uintptr_t)t.w | (uintptr_t)t.g | (uintptr_t)t.s1 | (uintptr_t)t.s2) & 15) == 0;
  mt_walk(first, t.n, vec,
          [&](long i) {
            float4 w = *reinterpret_cast<const float4*>(t.w + i);
            float4 g = *reinterpret_cast<const float4*>(t.g + i);
            g.x = fmaf(t.l2x2, w.x, g.x); g.y = fmaf(t.l2x2, w.y, g.y); g.z = fmaf(t.l2x2, w.z, g.z); g.w = fmaf(t.l2x2, w.w, g.w);
            float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
            if (S1) a = *reinterpret_cast<const float4*>(t.s1 + i);
            if (S2) b = *reinterpret_cast<const float4*>(t.s2 + i);
            update(w.x, g.x, a.x, b.x); update(w.y, g.y, a.y, b.y);
            update(w.z, g.z, a.z, b.z); update(w.w, g.w, a.w, b.w);
            *reinterpret_cast<float4*>(t.w + i) = w;
            if (S1) *reinterpret_cast<float4*>(t.s1 + i) = a;
            if (S2) *reinterpret_cast<float4*>(t.s2 + i) = b;
          },
          [&](long i) {
            float w = t.w[i], a = S1 ? t.s1[i] : 0.f, b = S2 ? t.s2[i] : 0.f;
            update(w, fmaf(t.l2x2, w, t.g[i]), a, b);
            t.w[i] = w;
            if (S1) t.s1[i] = a;
            if (S2) t.s2[i] = b;
          });
}

template <int RULE>
__global__ __launch_bounds__(256) void opt_step_kernel(const OptTensor* __restrict__ table, const int* __restrict__ chunks,
                                                       OptCoef k, const float* __restrict__ coef_dev) {
  if (coef_dev) {                                          // step-dependent scalars from device memory: a captured graph replays
    k.lr = coef_dev[0]; k.b1 = coef_dev[1]; k.b2 = coef_dev[2]; k.eps = coef_dev[3]; k.c1 = coef_dev[4]; k.c2 = coef_dev[5];
  }
  const MtChunk c = mt_chunk(chunks, blockIdx.x);
  const OptTensor t = table[c.tensor];
  if (!t.g) return;                                        // no gradient this step: Keras skips the variable
  opt_walk<RULE>(t, c.first, [&](float& w, float g, float& s1, float& s2) { opt_update<RULE>(w, g, s1, s2, k); });
}

// ---- parameter groups, decoupled decay, clipping, momentum (embnet_optimizer_step_groups) ---------------------------------------
// The same walk; what differs is workgroup-uniform: the tensor's group picks lr / c1 / decay, and two steps in front of the rule clip
// the gradient and decay the weight.
// opt_update leaves its multiply-adds to the compiler, and as built opt_step_kernel fuses the slot updates of RMSprop / Adam / RAdam
// one way on some lanes of its float4 path, another way on others, and not at all on its element-wise path.  No second statement of
// the rules can promise those bits, so a tensor that no option touches (no clip, d_g = 0, one of the five old rules) takes the very
// same walk over the very same opt_update here: with one group and no option the result is opt_step_kernel's, bit for bit, and a
// group's rate is all that tells two groups without options apart.  Where an option acts, every rounding is written out (contraction
// off, explicit fmaf), the same on both paths: there a tail or an unaligned tensor gets the bits of a whole aligned chunk.

constexpr int OPT_MOMENTUM_NESTEROV = EMBNET_OPT_MOMENTUM + 1;        // kernel-side rule code: the ABI passes `nesterov` beside the rule

struct OptGroups { float v[EMBNET_OPT_MAX_GROUPS][4]; };              // lr, c1, decay = (float)(lr * wd), unused
struct OptShared { float b1, b2, eps, c2, momentum, clipvalue; int n_groups; };

template <int RULE>
__device__ __forceinline__ void opt_update_options(float& w, float g, float& s1, float& s2, const OptCoef& k, float clipvalue,
                                                   bool scaled, float scale, float decay) {
#pragma clang fp contract(off)
  if (clipvalue > 0.f) g = fminf(fmaxf(g, -clipvalue), clipvalue);
  if (scaled) g = g * scale;
  if (decay != 0.f) w = fmaf(-decay, w, w);
  if (RULE == EMBNET_OPT_SGD) {
    w = fmaf(-k.lr, g, w);
  } else if (RULE == EMBNET_OPT_MOMENTUM || RULE == OPT_MOMENTUM_NESTEROV) {      // k.b1 = momentum; slot1 = the velocity
    const float step = -(k.lr * g);
    s1 = fmaf(k.b1, s1, step);
    w = w + (RULE == OPT_MOMENTUM_NESTEROV ? fmaf(k.b1, s1, step) : s1);
  } else if (RULE == EMBNET_OPT_RMSPROP) {
    s1 = fmaf(k.b1, s1, ((1.f - k.b1) * g) * g);
    w = w - (k.lr * g) / (sqrtf(s1) + k.eps);
  } else {
    s1 = fmaf(1.f - k.b1, g, k.b1 * s1);
    s2 = fmaf((1.f - k.b2) * g, g, k.b2 * s2);
    if (RULE == EMBNET_OPT_ADAM) w = w - (k.c1 * s1) / (sqrtf(s2) + k.eps);
    else if (RULE == EMBNET_OPT_RADAM) w = w - (k.c1 * s1) / (sqrtf(s2 * k.c2) + k.eps);
    else w = fmaf(-k.c1, s1, w);
  }
}

template <int RULE>
__global__ __launch_bounds__(256) void opt_step_groups_kernel(const OptTensor* __restrict__ table, const int* __restrict__ chunks,
                                                              OptGroups G, OptShared h, const float* __restrict__ coef_dev,
                                                              const float* __restrict__ group_dev,
                                                              const float* __restrict__ clip_scale_dev) {
  const MtChunk c = mt_chunk(chunks, blockIdx.x);
  const OptTensor t = table[c.tensor];
  if (!t.g) return;                                        // no gradient this step: no decay either, slots untouched
  const int gi = min(max(t.group, 0), h.n_groups - 1);     // whatever the word holds, the row is inside the arrays
  OptCoef k{0.f, h.b1, h.b2, h.eps, 0.f, h.c2};
  if (coef_dev) { k.b1 = coef_dev[1]; k.b2 = coef_dev[2]; k.eps = coef_dev[3]; k.c2 = coef_dev[5]; }
  float decay;
  if (group_dev) { k.lr = group_dev[4 * gi]; k.c1 = group_dev[4 * gi + 1]; decay = group_dev[4 * gi + 2]; }
  else { k.lr = G.v[gi][0]; k.c1 = G.v[gi][1]; decay = G.v[gi][2]; }
  constexpr bool OLD_RULE = RULE <= EMBNET_OPT_RADAM_WARM;
  if (!OLD_RULE) k.b1 = h.momentum;
  const float cv = h.clipvalue;
  const bool scaled = clip_scale_dev != nullptr;
  if (OLD_RULE && !(cv > 0.f) && !scaled && decay == 0.f) {  // no option touches this tensor: opt_step_kernel's walk (see above)
    opt_walk<OLD_RULE ? RULE : 0>(t, c.first, [&](float& w, float g, float& s1, float& s2) { opt_update<OLD_RULE ? RULE : 0>(w, g, s1, s2, k); });
    return;
  }
  const float cs = scaled ? *clip_scale_dev : 1.f;
  opt_walk<RULE>(t, c.first, [&](float& w, float g, float& s1, float& s2) { opt_update_options<RULE>(w, g, s1, s2, k, cv, scaled, cs, decay); });
}

// ---- the global gradient norm (embnet_optimizer_grad_norm) -------------------------------------------------------------------------
// A workgroup takes chunks c = blockIdx, blockIdx + grid, ...: the f64 sum of g'^2 over chunk c -> part[c]; the last workgroup to
// arrive adds the partials in a fixed order.  At most OPT_NORM_GRID workgroups: every arrival is an atomic on the one ticket word, and
// same-address atomics serialise at the memory side (one workgroup per chunk, 2 854 of them for ResNet18, spent 57 of its 61 us there).
constexpr int OPT_NORM_GRID = 512;
struct OptNormWorkspace { int ticket; int pad[3]; };                    // the partials (double [n_chunks]) follow
static_assert(sizeof(OptNormWorkspace) == 16, "embnet_optimizer_grad_norm_workspace_bytes");

__global__ __launch_bounds__(256) void opt_grad_norm_kernel(const OptTensor* __restrict__ table, const int* __restrict__ chunks,
                                                            int n_chunks, float clipnorm, int* ticket, double* part,
                                                            double* norm_out, float* scale_out) {
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const MtChunk ch = mt_chunk(chunks, c);
    const long first = ch.first;
    const OptTensor t = table[ch.tensor];
    double acc = 0.0;
    if (t.g) {                                             // workgroup-uniform; a tensor without a gradient is not in the norm
      const long end = min(first + MT_CHUNK, t.n);
      const bool l2 = t.l2x2 != 0.f;                       // the weight is only read where it joins the gradient
      const bool vec = (((uintptr_t)t.w | (uintptr_t)t.g) & 15) == 0;
      if (vec && end - first == MT_CHUNK) {
#pragma unroll
        for (int it = 0; it < MT_CHUNK / 1024; ++it) {
          const long i = first + it * 1024 + threadIdx.x * 4;
          float4 g = *reinterpret_cast<const float4*>(t.g + i);
          if (l2) {
            const float4 w = *reinterpret_cast<const float4*>(t.w + i);
            g.x = fmaf(t.l2x2, w.x, g.x); g.y = fmaf(t.l2x2, w.y, g.y); g.z = fmaf(t.l2x2, w.z, g.z); g.w = fmaf(t.l2x2, w.w, g.w);
          }
          acc += (double)g.x * (double)g.x; acc += (double)g.y * (double)g.y;
          acc += (double)g.z * (double)g.z; acc += (double)g.w * (double)g.w;
        }
      } else {                                             // the same elements per thread in the same order: the same bits
        for (int it = 0; it < MT_CHUNK / 1024; ++it) {
          for (int j = 0; j < 4; ++j) {
            const long i = first + it * 1024 + threadIdx.x * 4 + j;
            if (i >= end) break;
            float g = t.g[i];
            if (l2) g = fmaf(t.l2x2, t.w[i], g);
            acc += (double)g * (double)g;
          }
        }
      }
    }
    __syncthreads();                                       // block_sum256's array, between two chunks
    acc = block_sum256(acc);
    if (threadIdx.x == 0) part[c] = acc;
  }
  if (!last_workgroup_to_arrive(ticket)) return;           // (its barriers also separate the block_sum256 calls)
  double tot = 0.0;
  for (int i = threadIdx.x; i < n_chunks; i += 256) tot += __hip_atomic_load(&part[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  tot = block_sum256(tot);
  if (threadIdx.x == 0) {
    const double norm = sqrt(tot), c = (double)clipnorm;
    norm_out[0] = tot;
    norm_out[1] = norm;
    *scale_out = (float)(c / fmax(norm, c));
  }
}

}  // namespace embnet

using namespace embnet;

extern "C" int embnet_optimizer_chunk_elems(void) { return MT_CHUNK; }

extern "C" int embnet_optimizer_step(int rule, const void* table, int n_tensors, const int32_t* chunks, int n_chunks,
                                     float lr, float b1, float b2, float eps, float c1, float c2, const float* coef_dev,
                                     void* stream) {
  EMBNET_CHECK_ARG(table && chunks, "optimizer_step: null pointer");
  EMBNET_CHECK_ARG(n_tensors > 0 && n_chunks > 0, "optimizer_step: empty table");
  EMBNET_CHECK_ARG(rule >= EMBNET_OPT_SGD && rule <= EMBNET_OPT_RADAM_WARM, "optimizer_step: unknown rule %d", rule);
  const OptCoef k{lr, b1, b2, eps, c1, c2};
  const OptTensor* t = (const OptTensor*)table;
  hipStream_t s = (hipStream_t)stream;
  // algorithmic bytes: chunk count x chunk size x 4 B x (w read+write, g read, each slot read+write)
  EMBNET_TRACE("embnet::opt_step_kernel", TRACE_BYTES,
               4.0 * n_chunks * MT_CHUNK * (rule == EMBNET_OPT_SGD ? 3 : (rule == EMBNET_OPT_RMSPROP ? 5 : 7)), s);
  switch (rule) {
    case EMBNET_OPT_SGD: opt_step_kernel<EMBNET_OPT_SGD><<<n_chunks, 256, 0, s>>>(t, chunks, k, coef_dev); break;
    case EMBNET_OPT_RMSPROP: opt_step_kernel<EMBNET_OPT_RMSPROP><<<n_chunks, 256, 0, s>>>(t, chunks, k, coef_dev); break;
    case EMBNET_OPT_ADAM: opt_step_kernel<EMBNET_OPT_ADAM><<<n_chunks, 256, 0, s>>>(t, chunks, k, coef_dev); break;
    case EMBNET_OPT_RADAM: opt_step_kernel<EMBNET_OPT_RADAM><<<n_chunks, 256, 0, s>>>(t, chunks, k, coef_dev); break;
    default: opt_step_kernel<EMBNET_OPT_RADAM_WARM><<<n_chunks, 256, 0, s>>>(t, chunks, k, coef_dev); break;
  }
  return check_launch("optimizer_step");
}

extern "C" int embnet_optimizer_step_groups(int rule, const void* table, int n_tensors, const int32_t* chunks, int n_chunks,
                                            const float* group_coef, int n_groups, float b1, float b2, float eps, float c2,
                                            float momentum, int nesterov, float clipvalue, const float* clip_scale_dev,
                                            const float* coef_dev, const float* group_coef_dev, void* stream) {
  EMBNET_CHECK_ARG(table && chunks && group_coef, "optimizer_step_groups: null pointer");
  EMBNET_CHECK_ARG(n_tensors > 0 && n_chunks > 0, "optimizer_step_groups: empty table");
  EMBNET_CHECK_ARG(n_groups >= 1 && n_groups <= EMBNET_OPT_MAX_GROUPS, "optimizer_step_groups: %d groups (1..%d)", n_groups,
                   EMBNET_OPT_MAX_GROUPS);
  EMBNET_CHECK_ARG(rule >= EMBNET_OPT_SGD && rule <= EMBNET_OPT_MOMENTUM, "optimizer_step_groups: unknown rule %d", rule);
  EMBNET_CHECK_ARG(clipvalue >= 0.f, "optimizer_step_groups: negative clipvalue");          // (a NaN fails too)
  EMBNET_CHECK_ARG(!(clipvalue > 0.f && clip_scale_dev), "optimizer_step_groups: clipvalue and global_clipnorm are exclusive");
  EMBNET_CHECK_ARG(rule != EMBNET_OPT_MOMENTUM || momentum >= 0.f, "optimizer_step_groups: negative momentum");
  EMBNET_CHECK_ARG(rule == EMBNET_OPT_MOMENTUM || (momentum == 0.f && !nesterov),
                   "optimizer_step_groups: momentum belongs to EMBNET_OPT_MOMENTUM");
  OptGroups G = {};
  for (int i = 0; i < n_groups; ++i)
    for (int j = 0; j < 3; ++j) G.v[i][j] = group_coef[4 * i + j];
  const OptShared h{b1, b2, eps, c2, momentum, clipvalue, n_groups};
  const OptTensor* t = (const OptTensor*)table;
  hipStream_t s = (hipStream_t)stream;
  const int slots = rule == EMBNET_OPT_SGD ? 0 : (rule == EMBNET_OPT_RMSPROP || rule == EMBNET_OPT_MOMENTUM ? 1 : 2);
  EMBNET_TRACE("embnet::opt_step_groups_kernel", TRACE_BYTES, 4.0 * n_chunks * MT_CHUNK * (3 + 2 * slots), s);
#define EMBNET_OPT_GROUPS_LAUNCH(R) \
  opt_step_groups_kernel<R><<<n_chunks, 256, 0, s>>>(t, chunks, G, h, coef_dev, group_coef_dev, clip_scale_dev)
  switch (rule) {
    case EMBNET_OPT_SGD: EMBNET_OPT_GROUPS_LAUNCH(EMBNET_OPT_SGD); break;
    case EMBNET_OPT_RMSPROP: EMBNET_OPT_GROUPS_LAUNCH(EMBNET_OPT_RMSPROP); break;
    case EMBNET_OPT_ADAM: EMBNET_OPT_GROUPS_LAUNCH(EMBNET_OPT_ADAM); break;
    case EMBNET_OPT_RADAM: EMBNET_OPT_GROUPS_LAUNCH(EMBNET_OPT_RADAM); break;
    case EMBNET_OPT_RADAM_WARM: EMBNET_OPT_GROUPS_LAUNCH(EMBNET_OPT_RADAM_WARM); break;
    default:
      if (nesterov) EMBNET_OPT_GROUPS_LAUNCH(OPT_MOMENTUM_NESTEROV);
      else EMBNET_OPT_GROUPS_LAUNCH(EMBNET_OPT_MOMENTUM);
      break;
  }
#undef EMBNET_OPT_GROUPS_LAUNCH
  return check_launch("optimizer_step_groups");
}

extern "C" size_t embnet_optimizer_grad_norm_workspace_bytes(int n_chunks) {
  return n_chunks > 0 ? sizeof(OptNormWorkspace) + sizeof(double) * (size_t)n_chunks : 0;
}

extern "C" int embnet_optimizer_grad_norm(const void* table, int n_tensors, const int32_t* chunks, int n_chunks, float clipnorm,
                                          void* workspace, size_t workspace_bytes, double* norm_out, float* scale_out,
                                          void* stream) {
  EMBNET_CHECK_ARG(table && chunks && workspace && norm_out && scale_out, "optimizer_grad_norm: null pointer");
  EMBNET_CHECK_ARG(n_tensors > 0 && n_chunks > 0, "optimizer_grad_norm: empty table");
  EMBNET_CHECK_ARG(clipnorm > 0.f, "optimizer_grad_norm: clipnorm must be positive");       // (a NaN fails too)
  if (int rc = check_workspace("optimizer_grad_norm", workspace, workspace_bytes, embnet_optimizer_grad_norm_workspace_bytes(n_chunks)))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  OptNormWorkspace* ws = (OptNormWorkspace*)workspace;
  // algorithmic bytes: one read of g (w besides where a tensor has l2: not counted, the table is on the device)
  EMBNET_TRACE("embnet::opt_grad_norm_kernel", TRACE_BYTES, 4.0 * n_chunks * MT_CHUNK, s);
  opt_grad_norm_kernel<<<n_chunks < OPT_NORM_GRID ? n_chunks : OPT_NORM_GRID, 256, 0, s>>>(
      (const OptTensor*)table, chunks, n_chunks, clipnorm, &ws->ticket, (double*)(ws + 1), norm_out, scale_out);
  return check_launch("optimizer_grad_norm");
}
