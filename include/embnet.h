/* libembnet_hip.so — C ABI of the MI355X (gfx950) metric-learning hot path.
 *
 * The reference (RocketFlash/EmbeddingNet) is pure Python on Keras: it has no FFI
 * or operator-plugin interface.  Its boundary for this path is the Python call
 * surface that tools/train.py uses; embeddingnet_amd/ mirrors that
 * surface and lowers it onto the entry points below.  Each entry point names the
 * reference code it stands in for (paths relative to the reference root).
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer (HBM) unless marked "host";
 *     tensors are dense fp32, images/feature maps NHWC, conv kernels [R,S,Cin,Cout]
 *     (Keras HWIO), dense kernels [in,out];
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *     nothing synchronises, nothing allocates: the caller owns outputs and workspaces
 *     (sizes from the matching *_workspace_bytes call);
 *   - return 0 on success; <0 on error (EMBNET_E*), message via embnet_last_error()
 *     (thread-local).  Invalid arguments are rejected before anything is launched;
 *   - safe to call from several host threads on distinct streams/workspaces.
 */
#ifndef EMBNET_H
#define EMBNET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EMBNET_ABI_VERSION 22

enum {
  EMBNET_MINE_SEMIHARD = 0,    /* datagenerators.py:196-199 */
  EMBNET_MINE_HARDEST = 1,     /* datagenerators.py:188-190 */
  EMBNET_MINE_RANDOM_HARD = 2, /* datagenerators.py:192-194 */
  EMBNET_MINE_BATCH_HARD = 3   /* Hermans et al. (README.md:112 cites it; not in the reference's code): fused entry point only */
};

int embnet_abi_version(void);
const char* embnet_last_error(void);

/* Optional per-kernel timing (bench.py's roofline leg; build-defined, nothing in the reference to stand in for).
 * While enabled, every kernel launch of the entry points below is bracketed by two HIP events on the launch stream
 * and logged with the kernel's name and its ALGORITHMIC work: unit 0 = FLOP (MFMA-bound kernels: 2*M*N*K of the
 * GEMM the kernel computes), unit 1 = bytes (HBM-bound kernels: the bytes the operation must read and write once,
 * DESIGN.md §3.2); `bytes` is that byte count for every kernel (for a conv: input + kernel + output, once each).
 * embnet_trace_get waits for record i's end event and returns its duration; name/ms/work/unit/bytes are HOST
 * pointers.  Disabled (the default) a launch pays one flag test. */
int embnet_trace_enable(int on);          /* returns the previous state; the log is kept until embnet_trace_reset */
int embnet_trace_reset(void);
int embnet_trace_count(void);
int embnet_trace_get(int i, char* name, int name_cap, float* ms, double* work, int* unit, double* bytes);

/* ------------------------------------------------------------------ loss path */

/* datagenerators.py:219 `pairwise_distances(all_embeddings)` (scikit-learn euclidean):
 * dist[n,n] = sqrt(max(|x_i|^2 + |x_j|^2 - 2 x_i.x_j, 0)), diagonal 0; squared!=0 skips the sqrt.
 * x[n,e].  workspace >= embnet_pairwise_workspace_bytes(n, e) (row norms + the partial Gram slabs of a K-split launch: a
 * batch of n < 512 rows at a long e, e.g. the reference's default encodings_len = 4096, is too few tiles to fill the chip
 * otherwise; a workspace of only n floats is accepted and runs unsplit). */
size_t embnet_pairwise_workspace_bytes(int n, int e);
int embnet_pairwise_dist_f32(const float* x, int n, int e, float* dist, int squared,
                             void* workspace, size_t workspace_bytes, void* stream);

/* datagenerators.py:225-250 (+ selection rules :188-199): mine (anchor,positive,negative) row
 * indices from dist[n,n], n = p*k, class c = rows [c*k,(c+1)*k).  Pairs are visited in the
 * reference's order; triplets[T,3] is written in that order, T -> *count (>=1: the reference's
 * fallback triplet (n-2,n-1,0) when nothing qualifies).  triplets must hold
 * embnet_mine_max_triplets(p,k) rows; selected[pairs] receives the chosen negative row or -1;
 * cand_mask (optional, [pairs][ceil((n-k)/32)] words) receives the candidate set of each pair as
 * a bitmask over the ascending out-of-class columns.  seed drives the two random rules.
 * Non-finite distances (a NaN or inf embedding row): the loss value (dist[i,j] - dist[i,neg]) + margin is compared as it
 * comes out, so a NaN distance (either operand) is never a candidate and never the arg-max of `hardest`, and a +inf
 * distance to a negative (value -inf) disqualifies that negative; a pair left without a candidate selects -1.  Every
 * index written lies in [0, n). */
int embnet_mine_max_triplets(int p, int k);
int embnet_mine_triplets(const float* dist, int p, int k, float margin, int mode, uint64_t seed,
                         int32_t* triplets, int32_t* count, int32_t* selected, uint32_t* cand_mask,
                         void* stream);

/* Hermans batch-hard selection (README.md:112 cites it; no reference code): per anchor the
 * farthest same-class and the closest other-class row, the first index on ties.  triplets[n,3]; *count = n (optional).
 * Non-finite distances: a NaN never compares and +inf never wins among the negatives; when no column of a set compares
 * (the anchor's row is NaN), the set's first column is taken: the first same-class row other than the anchor, the first
 * other-class row (NumPy's arg-max / arg-min on an all-NaN set).  Both indices lie in [0, n) whatever dist holds; the same
 * rule holds for EMBNET_MINE_BATCH_HARD in embnet_fused_triplet_loss_fwd. */
int embnet_batch_hard(const float* dist, int p, int k, int32_t* triplets, int32_t* count, void* stream);

/* losses_and_accuracies.py:26-42 loss_function(y_true, y_pred): y_pred[t,3e] = concat(a,p,n);
 * loss[t] = max(|a-p|^2 - |a-n|^2 + margin, 0).  bwd: dy[t,3e] from dloss[t]. */
int embnet_triplet_hinge_fwd(const float* y_pred, int t, int e, float margin, float* loss, void* stream);
int embnet_triplet_hinge_bwd(const float* y_pred, const float* dloss, int t, int e, float margin,
                             float* dy, void* stream);

/* Same hinge on rows gathered from emb[n,e] by triplets[.,3] (fused train step; replaces the
 * three-branch concat of models.py:181-185 + the loss).  *count triplets are live (device
 * scalar, no host sync); loss[max_t], active[max_t] (1 where the hinge passes gradient);
 * *mean_loss = mean over the live triplets (Keras' reduction).  bwd: demb[n,e] =
 * (*upstream / count) * d(sum loss)/d emb, upstream NULL = 1. */
int embnet_triplet_gather_fwd(const float* emb, int n, int e, const int32_t* triplets,
                              const int32_t* count, int max_t, float margin, float* loss,
                              float* active, float* mean_loss, void* stream);
int embnet_triplet_gather_bwd(const float* emb, int n, int e, const int32_t* triplets,
                              const int32_t* count, int max_t, const float* active,
                              const float* upstream, float* demb, void* stream);

/* losses_and_accuracies.py:4-11 contrastive_loss (margin 1, y=1 same class): *loss = mean(...).
 * bwd: ddist[b] = *upstream * d loss / d dist. */
int embnet_contrastive_fwd(const float* y_true, const float* dist, int b, float* loss, void* stream);
int embnet_contrastive_bwd(const float* y_true, const float* dist, int b, const float* upstream,
                           float* ddist, void* stream);

/* losses_and_accuracies.py:47-50 accuracy: *acc = mean((dist < 0.5) == y_true). */
int embnet_accuracy(const float* y_true, const float* dist, int b, float* acc, void* stream);

/* backbones.py:38/:77/:118 K.l2_normalize(x, axis=1): y = x * rsqrt(max(sum x^2, 1e-12)).
 * rnorm[n] is saved for backward. */
int embnet_l2norm_fwd(const float* x, int n, int e, float* y, float* rnorm, void* stream);
int embnet_l2norm_bwd(const float* y, const float* rnorm, const float* dy, int n, int e, float* dx,
                      void* stream);

/* models.py:225 siamese 'l2' head: dist[b] = sqrt(max(sum (e1-e2)^2, 1e-7)). */
int embnet_pair_distance_fwd(const float* e1, const float* e2, int b, int e, float* dist, void* stream);
int embnet_pair_distance_bwd(const float* e1, const float* e2, const float* dist, const float* ddist,
                             int b, int e, float* de1, float* de2, void* stream);

/* Softmax pre-training head (backbones.py:128-204: Dense(n_classes, softmax), loss 'categorical_crossentropy',
 * metric 'accuracy'): logits/targets[b,c] (targets one-hot or soft); prob[b,c] kept for backward;
 * *mean_loss = mean_b(-sum_c t log softmax), *accuracy = mean(argmax z == argmax t). */
int embnet_softmax_xent_fwd(const float* logits, const float* targets, int b, int c, float* prob, float* row_loss,
                            float* row_correct, float* mean_loss, float* accuracy, void* stream);
int embnet_softmax_xent_bwd(const float* prob, const float* targets, int b, int c, const float* upstream,
                            float* dlogits, void* stream);

/* ---- evaluation right after training (models.py:128-161 predict_knn / calculate_prediction_accuracy, which
 * go through sklearn KNeighborsClassifier, brute-force Euclidean) ---- */
/* dist[nq,n] = Euclidean distance of every query row q[nq,e] to every gallery row x[n,e] (sklearn
 * euclidean_distances(Q, X) semantics; squared!=0 skips the sqrt). */
size_t embnet_cross_dist_workspace_bytes(int nq, int n);
int embnet_cross_dist_f32(const float* q, int nq, const float* x, int n, int e, float* dist, int squared,
                          void* workspace, size_t workspace_bytes, void* stream);
/* idx/val[rows,k] = the k smallest entries of each row of dist[rows,n], ascending, ties to the smaller column. */
int embnet_topk_smallest(const float* dist, int rows, int n, int k, int32_t* idx, float* val, void* stream);
/* pred[rows] = majority label among labels[idx[row,:]], ties to the smallest label (KNeighborsClassifier.predict). */
int embnet_knn_vote(const int32_t* idx, const int32_t* labels, int rows, int k, int32_t* pred, void* stream);

/* ---- retrieval evaluation (Recall@K, MRR): rank of each query's nearest same-class gallery item, computed without the
 * [nq,n] distance matrix (csrc/retrieval.hip).  Additions only: the ABI version stays 22.
 *   Inputs: queries q[nq,e] with labels q_labels[nq], gallery x[n,e] with labels x_labels[n] (int32, any order, no layout
 *     assumed).  self_exclude != 0: leave-one-out — nq == n is required, row i of q is row i of x, and column i is skipped
 *     for query i (neither a positive nor counted).
 *   Distance: the fp32 squared distance of embnet_cross_dist_f32, d2 = max(|q|^2 + |x|^2 - 2 q.x, 0), no square root (the
 *     order is the same); a NaN d2 counts as +inf, as in embnet_topk_smallest.
 *   Order: lexicographic on (d2, gallery index) — ties go to the smaller index (embnet_topk_smallest's rule).
 *   Positive of query r: a non-excluded column c with x_labels[c] == q_labels[r]; the first positive is the smallest one
 *     in the order.  Outputs per query:
 *       rank[r]      = 1 + the number of non-excluded NEGATIVE columns that precede the first positive; 0 without a positive
 *       pos_index[r] = gallery index of the first positive, or -1
 *       pos_d2[r]    = its d2, or +inf
 *   A minimum and an integer count: bitwise reproducible.  Two passes of the distance GEMM: one counts (2*nq*n*e FLOP), the
 *   other finds the first positives and visits only the tile pairs whose label sets can meet (a per-tile label filter: a few
 *   per cent of the tiles when labels come grouped by class, all of them when they come in random order).  O(nq + n) bytes
 *   of workspace (>= embnet_retrieval_workspace_bytes(nq, n), 16-byte aligned, no initialisation needed; a short one is
 *   refused with -3), no [nq,n] buffer, each embedding block below 2 GiB.  No allocation and no synchronisation inside.
 * embnet_retrieval_reduce: over the queries with rank > 0, hits[j] = #{rank <= ks[j]} (ks[nk] device int32, every ks[j] >= 1,
 *   no upper limit), *n_valid = #{rank > 0}, *sum_inv_rank = sum 1 / rank (f64, fixed order).  recall@K = hits / n_valid and
 *   mrr = sum_inv_rank / n_valid are the caller's divisions. */
size_t embnet_retrieval_workspace_bytes(int nq, int n);
int embnet_retrieval_first_positive(const float* q, const int32_t* q_labels, int nq,
                                    const float* x, const int32_t* x_labels, int n, int e, int self_exclude,
                                    int32_t* rank, int32_t* pos_index, float* pos_d2,
                                    void* workspace, size_t workspace_bytes, void* stream);
int embnet_retrieval_reduce(const int32_t* rank, int nq, const int32_t* ks, int nk,
                            int32_t* hits, int32_t* n_valid, double* sum_inv_rank, void* stream);

/* ---- retrieval evaluation (MAP@R, R-precision): the position of EVERY same-class gallery item of a query (csrc/retrieval.hip).
 * Additions only: the ABI version stays 22.
 *   Distance, order, exclusion, positives: exactly those of embnet_retrieval_first_positive above — d2 = rn + cn - 2 acc from the
 *     same fp32 chain, NaN -> +inf, max(., 0); lexicographic order on (d2, gallery index); self_exclude skips the query's own
 *     column; a positive is a non-excluded column with the query's label.
 *   For query r let R be the number of its positives and p_1 .. p_R the positives in that order.  pos(p_j) = the 1-based position
 *     of p_j among ALL non-excluded gallery items = j + the number of negatives in front of p_j.  Then
 *       r_precision[r] = #{j : pos(p_j) <= R} / R
 *       ap_at_r[r]     = (1 / R) * sum over {j : pos(p_j) <= R} of j / pos(p_j)
 *       ap[r]          = (1 / R) * sum over all j of j / pos(p_j)
 *     A query with R = 0 is invalid: its three values are NaN and it is left out of the sums.  map@r, r_precision and map are the
 *     sums over the valid queries divided by n_valid (the caller's divisions).  pos(p_1) is embnet_retrieval_first_positive's rank.
 * embnet_retrieval_positive_ranks.  Labels are DENSE ids in [0, num_classes).  Outputs (CSR):
 *       offset[nq + 1] int64   offset[r + 1] - offset[r] = R of query r, offset[0] = 0
 *       pos_index[capacity]    pos_index[offset[r] + j - 1] = gallery index of p_j
 *       pos_rank[capacity]     pos_rank[offset[r] + j - 1]  = pos(p_j), strictly increasing within a query
 *       status[1]              0 = ok; 1 = the sum of R exceeds `capacity`; 2 = some R exceeds EMBNET_RETRIEVAL_R_MAX; 3 = a label
 *                              outside [0, num_classes) (the largest that applies).  Everything that depends on label CONTENTS is
 *                              found on the device and reported here, not through the return value.  On a non-zero status offset is
 *                              still written in full, pos_index / pos_rank are not written at all, and embnet_retrieval_map_reduce
 *                              must not be called on them; every address derived from offset is guarded in the kernels (slot < R,
 *                              offset + R <= capacity) whatever the status.
 *   EMBNET_RETRIEVAL_R_MAX = 4096 positives per query: a segment of 4096 eight-byte keys is 32 KB, which a workgroup sorts in LDS
 *     without the large-LDS opt-in.  Larger classes are refused (status 2).
 *   Properties.  No [nq, n] buffer is formed: two walks of the distance GEMM consume d2 in registers.  The workspace is
 *     O(nq + n + num_classes + capacity) bytes (>= embnet_retrieval_positive_ranks_workspace_bytes, 16-byte aligned, short -> -3).
 *     Every result is an exact integer (stores of unique keys, a sort, integer counts).  The outputs are bitwise reproducible
 *     across runs, streams and graph replay, although the slot a gallery item takes inside its class is not: the sort removes it.
 *     The workspace needs no initialisation: counters, histogram and status are zeroed by the call's own kernels.  Both tile
 *     geometries (64x64, 128x128, chosen as for embnet_retrieval_first_positive) and both loaders (16-byte; scalar for unaligned
 *     pointers or e % 4 != 0) compute the same arithmetic.  No allocation and no synchronisation inside.
 * embnet_retrieval_map_reduce: per query ap_at_r / r_precision / ap (f64[nq] each, NaN for R = 0) from offset and pos_rank;
 *   sums[3] = their sums over the queries with R > 0 and *n_valid the number of those, folded in a fixed order (no float atomics). */
#define EMBNET_RETRIEVAL_R_MAX 4096
size_t embnet_retrieval_positive_ranks_workspace_bytes(int nq, int n, int num_classes, long capacity);
int embnet_retrieval_positive_ranks(const float* q, const int32_t* q_labels, int nq,
                                    const float* x, const int32_t* x_labels, int n, int e, int self_exclude,
                                    int num_classes, long capacity, long long* offset, int32_t* pos_index, int32_t* pos_rank,
                                    int32_t* status, void* workspace, size_t workspace_bytes, void* stream);
int embnet_retrieval_map_reduce(const long long* offset, const int32_t* pos_rank, int nq,
                                double* ap_at_r, double* r_precision, double* ap, double* sums, int32_t* n_valid, void* stream);

/* ---- k-means on encodings (the clustering behind the NMI evaluation; scikit-learn KMeans(algorithm='lloyd') is what it stands in
 * for, the reference has none): csrc/kmeans.hip.  Additions only: the ABI version stays 22.
 *   Shapes: points x[n,e], centres[k,e], 1 <= k <= n, each block below 2 GiB.  One workspace serves all of a fit's calls:
 *     >= embnet_kmeans_workspace_bytes(n, k, e) bytes (0 for a refused shape), 16-byte aligned, no initialisation needed, short -> -3.
 *     It grows as O(n + (n / 512 + k) * e) bytes.  Nothing allocates or synchronises.
 * embnet_kmeans_assign: labels[i] = the centre nearest to point i.  Distance, NaN rule and order are those of
 *     embnet_retrieval_first_positive (the same walk of the fp32 distance GEMM with the points as queries and the centres as
 *     gallery): d2 = max(|x|^2 + |c|^2 - 2 x.c, 0), NaN -> +inf, order (d2, centre index) — ties go to the smaller index, exactly.
 *     A point without a finite distance takes label 0 and d2 = +inf.  No [n,k] matrix is formed.
 *       labels[n] int32, d2[n] float (to the chosen centre)
 *       *changed int32 = #{i : labels[i] != labels_prev[i]} (labels_prev NULL: n); labels_prev must not be `labels`
 *       *inertia f64 = sum of d2 in a fixed order (8-byte aligned)
 *     reuse_point_norms != 0: the point norms an earlier call on the SAME x left in this workspace are used again (a fit computes
 *     them once); the centre norms are computed by every call.  A minimum, an integer count and fixed-order sums: two calls
 *     return the same bits.
 * embnet_kmeans_update: centres_out[j] = the mean of the points with labels[i] == j (centres_out may be `centres`).
 *       count[k] int32, exact.  A label outside [0,k) belongs to no cluster.
 *       Each element is summed in f64 in an order that depends on (n, e, k, labels) alone — a cluster's points ascending by index
 *       in chunks of 512, four interleaved row chains per chunk, the chunks in order — divided in f64 and rounded to f32 once.
 *       A cluster without points keeps its centre bit for bit; *n_empty int32 counts them.
 *       *shift f64 = sum over the non-empty clusters of |new - old|^2, fixed order (8-byte aligned).
 * embnet_kmeans_pp_update / embnet_kmeans_pp_pick: k-means++ seeding by plain D^2 sampling, one draw per centre (not
 *     scikit-learn's greedy variant).  pp_update: mind2[i] = min(mind2[i], |x_i - x_c|^2) for the row c = *index (device), by the
 *     lane-strided fp32 chain on the difference; first != 0 stores instead of taking the minimum.  pp_pick, draw 0:
 *     *index = rng(seed, 0, 0) mod n and *u = 0 (mind2 may be NULL).  Draw j >= 1: *u = (53 bits of rng(seed, j, 0) : rng(seed, j, 1))
 *     * 2^-53 (f64, 8-byte aligned); *index = the first row of positive weight whose inclusive f64 prefix sum of mind2 (fixed
 *     two-level order) exceeds *u * total, so a row of weight 0 is never drawn while total > 0; total == 0: floor(*u * n).
 *     A non-finite or negative mind2 weighs 0.  rng is the library's counter-based generator (csrc/common.h rng_u32). */
size_t embnet_kmeans_workspace_bytes(int n, int k, int e);
int embnet_kmeans_assign(const float* x, int n, const float* centres, int k, int e, int reuse_point_norms,
                         const int32_t* labels_prev, int32_t* labels, float* d2, int32_t* changed, double* inertia,
                         void* workspace, size_t workspace_bytes, void* stream);
int embnet_kmeans_update(const float* x, const int32_t* labels, int n, const float* centres, int k, int e,
                         float* centres_out, int32_t* count, double* shift, int32_t* n_empty,
                         void* workspace, size_t workspace_bytes, void* stream);
int embnet_kmeans_pp_update(const float* x, int n, int e, const int32_t* index, int first, float* mind2, void* stream);
int embnet_kmeans_pp_pick(const float* mind2, int n, uint64_t seed, int draw, int32_t* index, double* u, void* stream);

/* ---- verification (ROC AUC, EER, TAR@FAR): every pair of encodings counted into a same-class and an other-class histogram of its
 * distance, without the [nq,n] matrix and without a sort (csrc/verification.hip).  Additions only: the ABI version stays 22.
 *   Bin contract.  A histogram has `bins` bins over [lo, lo + bins * w): bins a power of two in [2, EMBNET_VERIFICATION_MAX_BINS],
 *     w a positive power of two (a normal float), lo finite (0 for distances).
 *       bin(v) = clamp((int)floorf((v - lo) * (1 / w)), 0, bins - 1),   bin(NaN) = bins - 1   (as the walk's "NaN counts as +inf")
 *     1 / w is a power of two, so the product is exact: the bin is an EXACT function of the fp32 value v (of v - lo, which is v
 *     for distances), not a second rounding, and a host restatement in float32 gives the same integer.  Thresholds are the edges
 *     t_j = lo + j * w, j = 0 .. bins; a pair is accepted as "same" at threshold t_j iff its bin is below j, that is iff v < t_j
 *     (for j < bins; everything from the last edge on, +inf and NaN included, sits in the last bin).
 *   Outputs: hist_same[bins], hist_other[bins], uint64, 8-byte aligned.  The call zeroes them with a kernel of its own (not a
 *     memset node), then adds exact integers with integer atomics: the result does not depend on scheduling and is bitwise
 *     reproducible across runs, streams and graph replay.
 * embnet_verification_all_pairs: one walk of the fp32 distance GEMM of embnet_retrieval_first_positive — the same d2 =
 *     max(|q|^2 + |x|^2 - 2 q.x, 0), NaN -> +inf, the same tile and split plan (both geometries) and loaders (16-byte; scalar for
 *     unaligned pointers or e % 4 != 0) — whose epilogue counts bin(d2) of every pair (query r, gallery column c) into hist_same
 *     when the labels agree and into hist_other otherwise; lo = 0, w = d2_max / bins, d2_max a positive power of two.
 *     x == NULL (then x_labels must be NULL and n == nq): leave-one-out, the gallery IS the query block and pair (i, i) is
 *     skipped; every unordered pair is then counted TWICE (as (i, j) and as (j, i)), and halving is the caller's.
 *     A gallery that IS the query block (x == q, or q a part of x) is an ordinary gallery: all nq * n pairs count, the
 *     d2 = 0 self pairs among the same-class ones.
 *     A workgroup counts into a private LDS histogram with 32-bit counters and adds its non-zero bins to the outputs every
 *     `flush_tiles` gallery tiles and at the end of its walk.  flush_tiles = 0: the largest interval that cannot overflow a
 *     counter, (2^32 - 1) / (BM * BN) for the plan's BM x BN tile; a positive value above that is refused, any other is honoured
 *     (the result is the same for every value).  Workspace: >= embnet_verification_all_pairs_workspace_bytes(nq, n) bytes
 *     (0 for nq <= 0 or n <= 0), 16-byte aligned, no initialisation needed, short -> -3.  Refused with -1: a null pointer, bins or
 *     d2_max outside the contract, sizes the walk refuses (a block of 2 GiB or more, nq, n, e <= 0), too large a flush_tiles.
 *     2*nq*n*e FLOP, O(nq + n) bytes of workspace.  No allocation and no synchronisation inside.
 * embnet_verification_values: the same bin function and LDS histogram over a vector: values[m] f32, same[m] int32 (non-zero:
 *     a same-class pair).  m = 0 is accepted and yields zeros.  It serves explicit pair lists (the distances of
 *     embnet_pair_distance_fwd) and similarity scores.  Refused with -1: a null pointer, m < 0, bins, w or lo outside the contract. */
#define EMBNET_VERIFICATION_MAX_BINS 4096
size_t embnet_verification_all_pairs_workspace_bytes(int nq, int n);
int embnet_verification_all_pairs(const float* q, const int32_t* q_labels, int nq,
                                  const float* x, const int32_t* x_labels, int n, int e, int bins, float d2_max, int flush_tiles,
                                  uint64_t* hist_same, uint64_t* hist_other,
                                  void* workspace, size_t workspace_bytes, void* stream);
int embnet_verification_values(const float* values, const int32_t* same, int m, float lo, float w, int bins,
                               uint64_t* hist_same, uint64_t* hist_other, void* stream);

/* ---- k-nearest-neighbour search: the k nearest gallery items of every query, computed without the [nq,n] distance matrix
 * (csrc/knn_search.hip).  Additions only: the ABI version stays 22.
 *   Distance, order, exclusion: exactly those of embnet_retrieval_first_positive above — d2 = max(rn + cn - 2 acc, 0) from the
 *     same fp32 chain, NaN -> +inf; lexicographic order on (d2, gallery index), ties to the smaller index (embnet_topk_smallest's
 *     rule); self_exclude != 0 needs nq == n (row i of q is row i of x) and skips column i for query i.
 *   Eligible columns of query r, by `select`: 0 every non-excluded column; 1 only those with x_labels[c] == q_labels[r] (nearest
 *     positives); 2 only those with another label (hard negatives).  select == 0: the label arrays may be NULL (they are not
 *     read); select != 0: both are required.
 *   Outputs, 1 <= k <= EMBNET_KNN_K_MAX:
 *       found[nq] int32   found[r] = min(k, number of eligible columns of r)
 *       idx[nq,k] int32   the first found[r] entries: the eligible columns with the smallest (d2, index), ascending in that order
 *       d2[nq,k] float    their squared distances
 *     Entries from found[r] on are idx = -1, d2 = +inf.  A NaN distance is a real entry: d2 = +inf with its index >= 0, behind
 *     every finite one.  k may exceed n (the rows are padded).
 *   Properties.  One walk of the distance GEMM (2*nq*n*e FLOP) whose epilogue keeps the candidates of a tile's rows in LDS and
 *     writes each row's k best per gallery split; a second kernel merges the splits.  Keys are unique, so the k smallest do not
 *     depend on the order in which they are met: the outputs are bitwise reproducible across runs, streams and graph replay.
 *     Workspace: >= embnet_knn_search_workspace_bytes(nq, n, k) bytes (0 for a refused shape), 16-byte aligned, no initialisation
 *     needed, short -> -3; O(n + nq + splits * nq * k) bytes with splits * ceil(nq / 64) <= 512 + ceil(nq / 64) — never O(nq * n).
 *     Both loaders (16-byte; scalar for unaligned pointers or e % 4 != 0) compute the same arithmetic; the walk runs on 64x64
 *     tiles.  Refused with -1: a null pointer, nq, n, e <= 0, a block of 2 GiB or more, k outside [1, EMBNET_KNN_K_MAX], select
 *     outside {0, 1, 2}, select != 0 without both label arrays, self_exclude with nq != n, an unaligned workspace.
 *     No allocation and no synchronisation inside. */
#define EMBNET_KNN_K_MAX 128
size_t embnet_knn_search_workspace_bytes(int nq, int n, int k);
int embnet_knn_search(const float* q, const int32_t* q_labels, int nq,
                      const float* x, const int32_t* x_labels, int n, int e,
                      int self_exclude, int select, int k,
                      int32_t* idx, float* d2, int32_t* found,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ backbone layers
 * Stand-ins for the Keras layers that backbones.py:19-121 instantiates (TensorFlow kernels in the
 * reference).  All NHWC fp32. */

/* Conv2D (backbones.py:21-31, :44-68, zoo ResNet/EfficientNet convs): implicit GEMM.  fp32 in, fp32 out, fp32
 * accumulation; each fp32 product is formed on the bf16 matrix instruction from an EXACT three-way split of both
 * operands by truncation (x = x1 + x2 + x3, 8 significant bits each) as six of the nine cross terms.
 * ERROR BOUND.  The three dropped terms x2*y3 + x3*y2 + x3*y3 are <= 2^-20 |x||y| in the worst case (the low 16 mantissa
 * bits of both operands all ones; typically 2^-22) and have the product's sign, so on top of fp32 accumulation a result is
 * LOW by at most 2^-20 * sum|x||y| — a bias, not zero-mean noise.  Measured on that adversarial input with all-positive
 * operands (tests/test_round3_gpu.py::test_conv_split_worst_case, profiles/r03_split_worst_case_*.json), relative to
 * sum|x||y|:  K = 576: 1.5e-6 max / -4.4e-7 mean (a float32 CPU convolution on the same input: 2.1e-6 / -9.4e-7);
 * K = 4608 forward: 3.3e-5 / -2.2e-5 (float32 CPU: 1.9e-5 / -1.4e-5: fp32 accumulation dominates there), data gradient
 * 2.3e-6 (6.7e-6), weight gradient 5.8e-7 (1.1e-7).  On operands with random mantissas the error is that of the fp32
 * MFMA's k-ordered fma chain (test_conv2d_products_are_fp32_accurate); on integer-valued operands results are exact.
 * The three bf16 pieces of THIS (six-term) form keep fp32's exponent range (no overflow / underflow beyond fp32's own); the
 * two-piece fp16 form of the *_ex entry points and of the planes kernels does not — its bound is stated under PRECISION below.  INFINITY: an infinite operand yields
 * NaN where an fp32 product would yield inf (inf - inf inside the split) — training has diverged by then either way.
 * embnet_conv_mfma_terms() = bf16 MFMA terms per product in this build (6), or 1 for a build on v_mfma_f32_32x32x2_f32.
 * x[n,h,w,c], w[r,s,c,k], y[n,oh,ow,k]; taps outside the image read 0 (pad_t/pad_l = top/left
 * padding; bottom/right follow from oh/ow, which the caller computes: Keras 'valid', 'same' incl. its
 * bottom/right asymmetry, or an explicit ZeroPadding2D).  bias may be NULL; relu!=0 fuses the activation;
 * residual (NULL or [n,oh,ow,k]) is added last — the Add layer that closes a residual unit.
 * in_scale/in_shift [c] (NULL or both) + in_act (0 none, 1 relu, 2 swish): the conv reads
 * act(x*in_scale + in_shift) instead of x — the BatchNormalization(+activation) in front of it, applied in
 * registers between the gather and LDS so the normalised tensor is never written; padding stays 0.
 * Needs c % 4 == 0 and k % 4 == 0.  conv2d_wgrad takes the same triple (it re-derives the conv input).
 * stats (NULL or [2][k][P], P = embnet_conv2d_fwd_stats_rows): per-channel sum and sum of squares of y, by row
 * band, written by the epilogue while the tile is in registers — the statistics pass of the BatchNormalization
 * that follows (hand them to embnet_bn_train_fwd as partial_in).
 * workspace (optional, may be NULL/0): >= embnet_conv2d_fwd_workspace_bytes lets the launcher cut the
 * `tiles mod 256` left-over output tiles along K so the last round of workgroups fills every CU
 * (partial tiles + fixed-order fix-up; results differ from the unsplit launch only in fp32 summation order). */
int embnet_conv_mfma_terms(void);
/* ... per fp32 product in the kernels that read pre-split planes (embnet_conv2d_patch_f32, embnet_conv2d_wgrad_planes_f32):
 * 3 in the default planes format (two fp16 pieces + a power-of-two scale per tensor), 6 with EMBNET_PLANES_F16=0 (three bf16 pieces). */
int embnet_conv_planes_mfma_terms(void);
size_t embnet_conv2d_fwd_workspace_bytes(int n, int c, int r, int s, int k, int oh, int ow);
int embnet_conv2d_fwd_stats_rows(int n, int c, int r, int s, int k, int oh, int ow);
int embnet_conv2d_fwd_f32(const float* x, const float* w, const float* bias, float* y, int n, int h, int wd, int c,
                          int r, int s, int k, int stride, int pad_t, int pad_l, int oh, int ow, int relu,
                          const float* residual, const float* in_scale, const float* in_shift, int in_act,
                          float* stats, void* workspace, size_t workspace_bytes, void* stream);
/* dx[n,h,w,c] from dy[n,oh,ow,k] (gradient w.r.t. the conv input).  workspace as for fwd (stride 1 only).
 * accumulate != 0: dx += instead of dx = (the input feeds two convs, e.g. a residual unit's 3x3 and its 1x1
 * projection shortcut: the second dgrad adds in its epilogue and skips pixels no tap reaches).
 * dx_add (NULL or [n,h,w,c]): dx = result + dx_add — the gradient reaching x through a skip connection. */
size_t embnet_conv2d_dgrad_workspace_bytes(int n, int h, int wd, int c, int r, int s, int k, int stride);
int embnet_conv2d_dgrad_f32(const float* dy, const float* w, float* dx, int n, int h, int wd, int c, int r, int s,
                            int k, int stride, int pad_t, int pad_l, int oh, int ow, int accumulate, const float* dx_add,
                            void* workspace, size_t workspace_bytes, void* stream);
/* Data gradient that also emits the BatchNorm-backward sums of the layer that produced this conv's input: the conv read
 * a = act(bn_x*bn_scale + bn_shift) (a BatchNormalization with a fused activation, /root/reference/embedding_net/backbones.py:99-104:
 * the zoo ResNets' pre-activation units), so  dz = dx * act'(..)  is that layer's output gradient; bn_partial [2][c][bn_rows]
 * (bn_rows = embnet_conv2d_dgrad_bnsums_rows(...), 0 = geometry not supported: stride 1, c % 4 == 0, k % 4 == 0) receives the
 * per-row-band sums of dz and dz * (bn_x - bn_mean) * bn_rstd — what embnet_bn_bwd's reduction pass would compute from two
 * tensors — for embnet_bn_bwd_partials.  Everything else as embnet_conv2d_dgrad_f32 without accumulate / dx_add. */
int embnet_conv2d_dgrad_bnsums_rows(int n, int h, int wd, int c, int r, int s, int k, int stride);
int embnet_conv2d_dgrad_bnsums_f32(const float* dy, const float* w, float* dx, int n, int h, int wd, int c, int r, int s,
                                   int k, int stride, int pad_t, int pad_l, int oh, int ow, const float* bn_x,
                                   const float* bn_scale, const float* bn_shift, const float* bn_mean, const float* bn_rstd,
                                   int bn_act, float* bn_partial, int bn_rows, void* workspace, size_t workspace_bytes,
                                   void* stream);
/* dw[r,s,c,k]; split-K slabs live in `workspace` (>= embnet_conv2d_wgrad_workspace_bytes). */
size_t embnet_conv2d_wgrad_workspace_bytes(int n, int c, int r, int s, int k, int oh, int ow);
int embnet_conv2d_wgrad_f32(const float* x, const float* dy, float* dw, void* workspace, size_t workspace_bytes,
                            int n, int h, int wd, int c, int r, int s, int k, int stride, int pad_t, int pad_l,
                            int oh, int ow, const float* in_scale, const float* in_shift, int in_act, void* stream);

/* conv2d_wgrad in two calls (split-K MFMA kernel into the slabs; then the fixed-order slab sum), same
 * arguments: lets a caller time the MFMA kernel alone.  conv2d_wgrad_f32 == slabs + reduce. */
int embnet_conv2d_wgrad_slabs_f32(const float* x, const float* dy, float* dw, void* workspace, size_t workspace_bytes,
                                  int n, int h, int wd, int c, int r, int s, int k, int stride, int pad_t, int pad_l,
                                  int oh, int ow, const float* in_scale, const float* in_shift, int in_act,
                                  void* stream);
int embnet_conv2d_wgrad_reduce_f32(const float* x, const float* dy, float* dw, void* workspace, size_t workspace_bytes,
                                   int n, int h, int wd, int c, int r, int s, int k, int stride, int pad_t, int pad_l,
                                   int oh, int ow, const float* in_scale, const float* in_shift, int in_act,
                                   void* stream);
/* Split count of conv2d_wgrad's plan for a geometry (1 = the kernel writes dw itself, no slabs). */
int embnet_conv2d_wgrad_splits(int n, int c, int r, int s, int k, int oh, int ow);
/* The slab sums of MANY weight gradients in one launch (a step's backward runs embnet_conv2d_wgrad_slabs_f32 into
 * per-layer slab buffers and adds them up once, before the optimizer / a bucket's all-reduce).
 * host_table: HOST array of n_tensors descriptors { const float* slabs; float* out; int64 n; int32 splits; int32 reserved }
 * (32 bytes; device pointers inside): out[i] = sum_s slabs[s*n + i], in embnet_conv2d_wgrad_reduce_f32's order
 * (bit-identical).  The descriptors travel as kernel arguments (112 per launch), so nothing has to stay alive for a
 * captured graph.  slabs and out 16-byte aligned when n % 4 == 0. */
int embnet_slab_reduce_multi(const void* host_table, int n_tensors, void* stream);

/* ---- three products per fp32 product for the implicit-GEMM ("gather") convolutions above (ABI 21 / 22; csrc/conv.hip "Ranges") -------
 * The layers of backbones.py:99-104 the patch kernels do not take — the 7x7 stem, the stride-2 3x3 convs, every 1x1 conv — split
 * their fp32 operands inside the kernel.  Given the RANGE of BOTH operands they use the planes kernels' arithmetic (below: two fp16
 * pieces of x s, three products, the sums x 1 / s x 1 / s') instead of three bf16 pieces and six products: half the matrix
 * instructions.  Without either range a call computes the six-term products: there is NO default scale (ABI 20 ran activations at
 * s = 1, which loses precision for tensors of amplitude << 2^-3 and clamps above 65504; see PRECISION under the planes format).
 * A RANGE SLOT is one uint32 in device memory holding the bit pattern of a float B >= max |element| of a tensor (0: an all-zero
 * tensor).  Who writes it:
 *   kernels      embnet_range_multi: the exact maxima of many tensors (a model's kernels, once per optimizer step) in two launches;
 *                device table of 24-byte rows { const float* x; int64 n; uint32* slot; }, chunk list int32 [n_chunks][2] = (row,
 *                chunk of embnet_range_chunk_elems() elements);
 *   gradients    `dx_range` of embnet_bn_bwd_ex / embnet_bn_bwd_partials_ex / embnet_bn_act_maxpool_bwd_ex: the exact max |dx| of the
 *                fp32 dx the call writes.  The slot has embnet_range_slot_words() words: the workgroups of the apply pass join their
 *                maxima into the words behind the first (zeroed by the finalize kernel; an order-independent unsigned maximum, spread
 *                over many words because same-address atomics serialise) and a one-workgroup launch folds them into word 0.  The
 *                call fails if it cannot emit (planes-only dx, c % 4 != 0, no saved statistics);
 *   activations  `y_range` of embnet_bn_train_fwd_ex / embnet_affine_act_planes_ex: an UPPER BOUND of max |act(BN(x))|, known before
 *                the apply pass runs — per channel |scale_c| sqrt(q_c) + |shift_c| with q_c the largest per-band sum of squares
 *                among the statistics partials (>= max x^2), folded over the channels; above the true maximum by at most
 *                sqrt(rows per band) (3.3 binades for a conv epilogue's bands), never below it.
 *   without a BatchNormalization (ABI 22; the `simple` / `simple2` backbones, reference backbones.py:19-81): the exact maximum of what
 *                the pass writes, a slot of embnet_range_slot_words() words as for gradients — `y_range` of embnet_pad_channels_ex
 *                (the image batch) and embnet_maxpool_fwd_ex (pooled activations), `dz_range` of embnet_maxpool_relu_bwd_colsum_ex,
 *                embnet_relu_bwd_colsum_ex and embnet_bn_bwd_inrelu[_dropout]_ex (the gradient behind a fused ReLU's mask).  These
 *                passes zero the slot with a KERNEL: a hipMemsetAsync node did not zero it when a captured HIP graph was replayed.
 * Who reads it: the last two pointer arguments (in front of `stream`) of embnet_conv2d_{fwd, dgrad, dgrad_bnsums, wgrad,
 * wgrad_slabs}_f32_ex — the ranges of the call's first and second tensor argument (x, w | dy, w | x, dy); NULL = unknown.  The
 * scale of a tensor puts B into [2^14, 2^15).  The scalar-load kernels (c or k % 4 != 0), a fused input transform and the thin
 * 1x1 streams compute as if no range had been given.  Results differ from the six-term kernels' in the last bits
 * (tests/test_conv_ranges_gpu.py: both against float64, activation amplitudes 1e-4 ... 1e5).
 * DEPRECATED, kept for one round: embnet_range_emit(slot) and embnet_conv2d_ranges(a, b) arm the same slots for the NEXT non-_ex
 * call of the calling thread (ABI 20) — hidden per-thread state: a binding in another language, a second stream on one thread or
 * an exception between the two calls gets the wrong arithmetic silently.  Every conv / bn_bwd entry point clears the request. */
/* out = the range slot of a tensor y with |y| <= factor * max_c bound[c] (+ the range in add_range, or NULL): for the outputs of
 * the fused BatchNorm passes that are not plain applies (act(BN(x)) * gate; skip + drop_factor * BN(x)); bound from embnet_bn_train_fwd_ex. */
int embnet_range_from_bound(const float* bound, int c, float factor, const uint32_t* add_range, uint32_t* out, void* stream);
int embnet_range_slot_words(void);
int embnet_range_emit(uint32_t* slot);
int embnet_range_chunk_elems(void);
int embnet_range_multi(const void* table, int n_tensors, const int32_t* chunks, int n_chunks, void* stream);
int embnet_conv2d_ranges(const uint32_t* a, const uint32_t* b);
int embnet_conv2d_fwd_f32_ex(const float* x, const float* w, const float* bias, float* y, int n, int h, int wd, int c,
                             int r, int s, int k, int stride, int pad_t, int pad_l, int oh, int ow, int relu,
                             const float* residual, const float* in_scale, const float* in_shift, int in_act,
                             float* stats, void* workspace, size_t workspace_bytes, const uint32_t* x_range,
                             const uint32_t* w_range, void* stream);
int embnet_conv2d_dgrad_f32_ex(const float* dy, const float* w, float* dx, int n, int h, int wd, int c, int r, int s,
                               int k, int stride, int pad_t, int pad_l, int oh, int ow, int accumulate, const float* dx_add,
                               void* workspace, size_t workspace_bytes, const uint32_t* dy_range, const uint32_t* w_range,
                               void* stream);
/* (the _ex form of dgrad_bnsums writes bn_partial as [3][c][bn_rows]: the two sums and max |dz| per row band) */
int embnet_conv2d_dgrad_bnsums_f32_ex(const float* dy, const float* w, float* dx, int n, int h, int wd, int c, int r, int s,
                                      int k, int stride, int pad_t, int pad_l, int oh, int ow, const float* bn_x,
                                      const float* bn_scale, const float* bn_shift, const float* bn_mean, const float* bn_rstd,
                                      int bn_act, float* bn_partial, int bn_rows, void* workspace, size_t workspace_bytes,
                                      const uint32_t* dy_range, const uint32_t* w_range, void* stream);
int embnet_conv2d_wgrad_f32_ex(const float* x, const float* dy, float* dw, void* workspace, size_t workspace_bytes,
                               int n, int h, int wd, int c, int r, int s, int k, int stride, int pad_t, int pad_l,
                               int oh, int ow, const float* in_scale, const float* in_shift, int in_act,
                               const uint32_t* x_range, const uint32_t* dy_range, void* stream);
int embnet_conv2d_wgrad_slabs_f32_ex(const float* x, const float* dy, float* dw, void* workspace, size_t workspace_bytes,
                                     int n, int h, int wd, int c, int r, int s, int k, int stride, int pad_t, int pad_l,
                                     int oh, int ow, const float* in_scale, const float* in_shift, int in_act,
                                     const uint32_t* x_range, const uint32_t* dy_range, void* stream);

/* Which kernel symbol (as rocprofv3 names it) the conv entry points launch for a geometry:
 * kind 0 = fwd, 1 = dgrad, 2 = wgrad.  Host-only helper for attributing timings. */
const char* embnet_conv2d_kernel_name(int kind, int n, int h, int wd, int c, int r, int s, int k, int oh, int ow);

/* 1x1 convolutions with a thin reduction (csrc/conv_thin.hip): embnet_conv2d_fwd_f32 with r = s = 1, pad 0, c <= 40 (EfficientNet's
 * expand convs) and embnet_conv2d_dgrad_f32 with r = s = 1, stride 1, k <= 40 (its project convs' data gradient) run as an HBM
 * stream — exact fp32 FMA chains over the reduction, the dense output written as one contiguous stream, statistics rows as
 * embnet_conv2d_fwd_stats_rows reports — instead of an implicit GEMM with a one-tile K loop; embnet_conv2d_wgrad_f32 with
 * r = s = 1, pad 0 and min(c, k) in {4, 8, ..., 20, 24, 32, 40} likewise (one slab per workgroup; embnet_conv2d_wgrad_splits /
 * _workspace_bytes report this path's counts).  1 when (reduction, output columns) takes the forward / data-gradient path
 * (EMBNET_CONV_THIN=0 turns all of it off, EMBNET_CONV_THIN_WGRAD=0 the weight gradient). */
int embnet_conv1x1_thin_supported(int red, int ncols);

/* ---- stride-1 3x3 convolution on pre-split operands ("patch" kernel, csrc/conv_patch.hip) --------------------------------
 * The zoo ResNets' 3x3 stride-1 layers (backbones.py:99-104), forward and data gradient, 1.1-1.25x faster than the kernels
 * above: every fp32 operand value is split into its three bf16 pieces ONCE, by the kernel that produces the tensor, and the
 * convolution keeps a patch of the padded input in LDS so that each input value is fetched once per output tile instead of
 * once per tap.  Summation order (chunk, r, s, channel).
 * FORMAT OF THE PLANES (one per process, csrc/common.h planes_f16()).  Default (ABI 19, end of round 5): TWO fp16 pieces of x s,
 * s a power of two per tensor — x = (h1 + h2) / s, h1 = fp16(x s) rounded to nearest, h2 = fp16(x s - h1): 22 mantissa bits —
 * and THREE products per fp32 product (h1 h1' + h1 h2' + h2 h1', v_mfma_f32_32x32x16_f16), the result x 1 / (s s') (exact).
 * Error on top of fp32 accumulation <= 2^-21 sum|x||y| (each operand kept to 2^-23 of itself, the dropped product <= 2^-22);
 * measured on the adversarial input above 4.1e-7 / 3.0e-7 / 1.7e-7 (forward / data gradient / weight gradient, K = 4608;
 * tests/test_round3_gpu.py::test_planes_split_worst_case, profiles/r05_split_worst_case_planes_*.json).
 * PRECISION.  s puts a bound B >= max |x| of the tensor into [2^14, 2^15).  Elements with |x s| >= 2^-3 (within 2^17 of B) are
 * kept to 2^-22 of themselves; below, h2 is an fp16 subnormal and the element carries an ABSOLUTE error <= 2^-25 / s <= 2^-39 B
 * — not a relative one: a tensor is only as precise as its largest element allows.  |x s| > 65504 cannot happen with a sound B and is
 * not clamped: it overflows to inf / NaN, loudly.  Where B comes from: the tensor's own largest element for kernels
 * (embnet_conv_weight_planes: a max pass) and gradients (embnet_bn_bwd's dx_planes: a dry run of the pass; embnet_planes_from_f32:
 * an abs-max pass); for activations the BatchNormalization's output bound (embnet_affine_act_planes_ex `y_bound`: RANGE SLOT above)
 * or, without one, a dry run of the pass.  (ABI 20 and earlier fixed s = 1 for activations: tensors of amplitude << 2^-3 sat on
 * the subnormal floor — 1.8e-4 relative error at amplitude 1e-4)
 * What this costs ONE ELEMENT of a result, by how far its operands lie below their tensor's bound, is measured in DESIGN.md 3.14 (9)
 * (the envelope table of tests/test_split_ref_cpu.py, and how deep the shipped ResNets' channels lie): fp32-class down to 2^16 below
 * the bound, 2^(d - 39) of sum |a||b| at depth d beyond that; tests/test_three_product_elementwise_gpu.py holds every kernel to
 * exactly this arithmetic, element by element.
 * The buffers keep the three-plane size below: planes 0 and 1 hold the pieces, the first two floats of the third plane's space
 * hold (s, 1 / s) (and a scratch word).  EMBNET_PLANES_F16=0: three bf16 pieces (exact split by truncation) and the six-term products documented above.
 *   planes of an activation / gradient x[pixels, c] (c % 16 == 0):  16-bit [3][c/16][pixels][16]  (piece, 16-channel chunk,
 *     pixel, channel in chunk) — written by embnet_affine_act_planes, by embnet_bn_bwd(dx_planes), or from an fp32 tensor by
 *     embnet_planes_from_f32;
 *   planes of a kernel w[r,s,c,k]:  16-bit [3][r][red/16][s][rows][16] — flip 0 (forward: rows = k, reduction channels = c) or
 *     flip 1 (stride-1 data gradient: rows = c, reduction = k, taps flipped) — written for any number of kernels by ONE launch
 *     of embnet_conv_weight_planes over a device table of 40-byte descriptors
 *       { const float* w; void* out; int32 r, s, c, k, flip, pad; }   and a chunk list int32 [n_chunks][2] =
 *     (tensor index, chunk of embnet_conv_weight_planes_chunk_elems() elements), typically once per optimizer step.
 * embnet_conv2d_patch_f32: y[n,oh,ow,k] = conv(x planes, w planes) with the epilogue options of embnet_conv2d_fwd_f32 (bias,
 * relu, residual, stats with P = embnet_conv2d_patch_stats_rows) — and, with dy planes, flip-1 kernel planes, c and k
 * swapped and pad = kernel - 1 - pad, the data gradient (residual = the gradient of the tensor's other consumer).
 * embnet_conv2d_patch_supported: 1 for 3x3, stride 1, c % 16 == 0, k % 4 == 0 and a patch that fits LDS. */
int embnet_conv2d_patch_supported(int n, int c, int r, int s, int k, int stride, int oh, int ow);
size_t embnet_conv2d_patch_workspace_bytes(int n, int c, int r, int s, int k, int oh, int ow);
int embnet_conv2d_patch_stats_rows(int n, int oh, int ow);
int embnet_conv2d_patch_f32(const void* x_planes, const void* w_planes, const float* bias, float* y, int n, int h, int wd, int c,
                            int r, int s, int k, int pad_t, int pad_l, int oh, int ow, int relu, const float* residual,
                            float* stats, void* workspace, size_t workspace_bytes, void* stream);
/* ABI 22 — the zoo ResNets' stem (7x7, stride 2, 4 -> 64 channels; reference backbones.py:99-104 via image-classifiers) forward as a
 * kernel of its own (csrc/conv_stem.hip): x fp32 [n,h,wd,4] (the image widened to four channels), w fp32 [7,7,4,64], y [n,oh,ow,64];
 * taps outside the image read zeros (pad_t / pad_l: where output (0, 0)'s window starts above / left of the image).  Every input
 * pixel reaches LDS once per 16 x 16 output tile (LDS-DMA), the kernel is split into its fp16 pieces by each workgroup, the products
 * are the three-term form: BOTH range slots are required.  stats (NULL or [2][64][embnet_conv2d_stem_stats_rows(n, oh, ow)]): the
 * BatchNorm statistics partials of the layer behind, as embnet_conv2d_fwd_f32's.  The gather kernel's result to fp32 rounding. */
int embnet_conv2d_stem_supported(int n, int h, int wd, int c, int r, int s, int k, int stride, int pad_t, int pad_l, int oh, int ow);
int embnet_conv2d_stem_stats_rows(int n, int oh, int ow);
int embnet_conv2d_stem_f32(const float* x, const float* w, float* y, int n, int h, int wd, int pad_t, int pad_l, int oh, int ow,
                           float* stats, const uint32_t* x_range, const uint32_t* w_range, void* stream);
/* 1x1 convolutions on the planes (ABI 21; csrc/conv_patch.hip conv1x1_planes_kernel): the bottleneck units' conv1 / conv3 and the
 * projection shortcuts (backbones.py:99-104) as a GEMM whose operands arrive by LDS-DMA from the planes — x planes of [n,h,wd,c],
 * kernel planes of a [1,1,c,k] kernel (embnet_conv_weight_planes; flip 1 and dy planes give the stride-1 data gradient) —
 * y[n,oh,ow,k] = sum_c x[n, oh*stride, ow*stride, c] w[c,k], epilogue options and workspace as embnet_conv2d_patch_f32
 * (embnet_conv2d_patch_supported / _workspace_bytes / _stats_rows with r = s = 1: c % 32 == 0, k % 4 == 0, stride 1 or 2, the
 * two-piece planes format). */
int embnet_conv2d_planes1x1_f32(const void* x_planes, const void* w_planes, const float* bias, float* y, int n, int h, int wd, int c,
                                int k, int stride, int oh, int ow, int relu, const float* residual, float* stats,
                                void* workspace, size_t workspace_bytes, void* stream);
/* ABI 22 — the same 1x1 product with the ACTIVATION operand read as fp32 (csrc/conv_patch.hip conv1x1_a32_kernel): no planes of x
 * have to exist.  x fp32 [n,h,wd,c] reaches LDS by DMA (16-byte pieces, one 128-byte line per pixel and 32-channel step, three stages
 * in flight) and is split into its two fp16 pieces by the matrix waves; x_range: x's RANGE SLOT (required — its scale); wp: the kernel
 * planes of embnet_conv_weight_planes (r = s = 1; flip 0).  With dy, dy's range slot, the flip-1 planes and c, k swapped (stride 1) the
 * call is the DATA GRADIENT (residual = a gradient to add).  c % 32 == 0, k % 4 == 0, stride 1 or 2, the tensor below 4 GiB:
 * embnet_conv2d_dma1x1_supported.  Workspace: embnet_conv2d_patch_workspace_bytes(n, c, 1, 1, k, oh, ow).  The Python layers leave it
 * off by default (layers.CONV1X1_DMA; DESIGN 3.14: 1.1 - 1.3 x the gather kernel back to back, no gain inside the HBM-bound C3 step). */
int embnet_conv2d_dma1x1_supported(int n, int h, int wd, int c, int k, int stride, int oh, int ow);
int embnet_conv2d_dma1x1_f32(const float* x, const void* wp, const float* bias, float* y, int n, int h, int wd, int c, int k,
                             int stride, int oh, int ow, int relu, const float* residual, float* stats, const uint32_t* x_range,
                             void* workspace, size_t workspace_bytes, void* stream);
/* The patch kernel as a stride-1 data gradient (dy planes, flip-1 kernel planes, c and k swapped as above) whose epilogue ALSO
 * emits the BatchNorm-backward sums of the BatchNormalization in front of the conv — the conv's input was
 * act(bn_scale * bn_x + bn_shift): embnet_conv2d_dgrad_bnsums_f32's contract on this kernel, bn_partial [2][k][bn_rows] with
 * bn_rows = embnet_conv2d_patch_stats_rows(n, oh, ow); embnet_bn_bwd_partials consumes it (ABI 19). */
int embnet_conv2d_patch_bnsums_f32(const void* x_planes, const void* w_planes, float* y, int n, int h, int wd, int c, int r, int s,
                                   int k, int pad_t, int pad_l, int oh, int ow, const float* bn_x, const float* bn_scale,
                                   const float* bn_shift, const float* bn_mean, const float* bn_rstd, int bn_act,
                                   float* bn_partial, int bn_rows, void* workspace, size_t workspace_bytes, void* stream);
/* The squeeze-and-excite gate of an MBConv block, gate = sigmoid(swish(pooled w1 + b1) w2 + b2) (pooled [n,c], w1 [c,s], w2 [s,c]),
 * as one forward launch (z1 [n,s]: the first layer's pre-activation, kept for backward) and two backward launches (dz1 [n,s]:
 * scratch; writes dpooled [n,c], dw1 [c,s], db1 [s], dw2 [s,c], db2 [c]; sums over the samples in sample order) instead of
 * twelve dense / activation / column-sum launches.  embnet_se_mlp_supported: 1 where they apply (s <= 160, LDS). */
int embnet_se_mlp_supported(int n, int c, int s);
int embnet_se_mlp_fwd(const float* pooled, const float* w1, const float* b1, const float* w2, const float* b2, int n, int c, int s,
                      float* z1, float* gate, void* stream);
int embnet_se_mlp_bwd(const float* dgate, const float* gate, const float* z1, const float* pooled, const float* w1, const float* w2,
                      int n, int c, int s, float* dz1, float* dpooled, float* dw1, float* db1, float* dw2, float* db2, void* stream);
int embnet_planes_from_f32(const float* x, long pixels, int c, void* planes, void* stream);
int embnet_conv_weight_planes_chunk_elems(void);
int embnet_conv_weight_planes(const void* table, int n_tensors, const int32_t* chunks, int n_chunks, void* stream);
/* y (NULL or [m,c]) = act(x*scale + shift) as embnet_affine_act, AND the same values as planes: the BatchNormalization in
 * front of a patch convolution writes the convolution's operand in its final form.
 * _ex: y_bound (NULL or [c]: the per-channel bounds embnet_bn_train_fwd_ex left) gives the planes' scale without another look at
 * the data; NULL (and the non-_ex form): a dry run of the pass finds the exact maximum first (+ 4 B per element read).
 * y_range (NULL or a range slot, needs y): the bound (or the exact maximum) as the range slot of the fp32 y. */
int embnet_affine_act_planes(const float* x, long m, int c, const float* scale, const float* shift, int act, float* y,
                             void* planes, void* stream);
int embnet_affine_act_planes_ex(const float* x, long m, int c, const float* scale, const float* shift, int act, float* y,
                                void* planes, const float* y_bound, uint32_t* y_range, void* stream);
/* Weight gradient of a 3x3, stride-1, pad-1 ('same') convolution FROM THE PLANES (csrc/conv_wgrad_planes.hip):
 * dw[3,3,c,k] = sum over pixels of x[n,h,wd,c] (shifted by the tap) * dy[n,h,wd,k], both operands as planes (layout above).
 * Every operand byte is fetched once per (64 channels x 64 filters) tile and all nine taps are accumulated from one window
 * of positions in LDS; split over pixel ranges into fp32 slabs [splits][9*c*k] in `workspace` and summed in fixed order
 * (bitwise reproducible).  reduce = 0 leaves the slabs for embnet_slab_reduce_multi (descriptor: workspace, dw, 9*c*k,
 * embnet_conv2d_wgrad_planes_splits).  Products in the planes' format (above); against embnet_conv2d_wgrad_f32 the order of the
 * pixel sum differs too, so results agree within fp32 rounding, not bitwise.  supported: 1 for r = s = 3, stride 1, pad 1, oh = h,
 * ow = wd <= 62, c % 64 == 0, k % 64 == 0. */
int embnet_conv2d_wgrad_planes_supported(int n, int h, int wd, int c, int r, int s, int k, int stride, int pad_t, int pad_l,
                                         int oh, int ow);
int embnet_conv2d_wgrad_planes_splits(int n, int h, int wd, int c, int k);
size_t embnet_conv2d_wgrad_planes_workspace_bytes(int n, int h, int wd, int c, int k);
int embnet_conv2d_wgrad_planes_f32(const void* x_planes, const void* dy_planes, float* dw, void* workspace,
                                   size_t workspace_bytes, int n, int h, int wd, int c, int k, int reduce, void* stream);

/* Input pipeline, last step (datagenerators.py:145-156: cv2 decode -> resize -> `/ 255.` on the host, per batch): uint8
 * images [n_src, pixels, c_in] (BGR as decoded) -> float32 batch dst[n, pixels, c_out]:
 *   dst[i][p][j] = j < c_in ? src[index ? index[i] : i][p][j] / denom : 0      (float32 division: the reference's values bit for bit)
 * index (NULL = the first n images in order) gathers a batch out of a dataset that is resident in HBM as uint8; c_out > c_in
 * pads channels with zeros (the 4-channel image the stem convolution gathers 16 bytes at a time).  n <= 65535. */
int embnet_u8_to_f32(const void* src, const int32_t* index, int n, long pixels, int c_in, int c_out, float denom, float* dst,
                     void* stream);

/* Device augmentation (csrc/augment.hip): the augmenting form of embnet_u8_to_f32, seeded and reproducible.  Stands in for the
 * albumentations pipelines of the reference (embedding_net/augmentations.py), which its configs never build.  Additions only:
 * the ABI version stays 22.
 * OPS: a host array of n_ops <= 8 records of 8 floats { opcode, p, a0, a1, a2, a3, 0, 0 }; an op fires with probability p:
 *   1 random_resized_crop  a0, a1 = scale (lo, hi), a2, a3 = ratio (lo, hi): torchvision's rule, 10 attempts, centre fallback
 *   2 center_crop          a0 = frac of the current box, resized back to h x w
 *   3 horizontal_flip      4 vertical_flip      5 random_rotate90 (k uniform in 0..3; square images only)
 *   6 brightness_contrast  a0 = brightness limit, a1 = contrast limit:  v * (1 + U(+-a1)) + U(+-a0) * 255
 *   7 gamma                a0, a1 = gamma_limit (lo, hi):  255 (v / 255)^(U(lo, hi) / 100)
 *   8 hue_saturation_value a0, a1, a2 = hue, sat, val shift limits: OpenCV 8-bit float HSV of the BGR pixel (H wraps at 180)
 *   9 blur                 a0 = blur_limit (1..7): k x k box, odd k uniform in [3, max(3, limit)], reflect-101 borders
 *  10 gauss_noise          a0, a1 = var_limit (lo, hi): sigma = sqrt(U(lo, hi)), one normal draw per element
 *  (11 clahe is not an op record: embnet_augment_params_clahe below takes it apart from the list)
 * Only 6-8 may repeat.  Application order is fixed: geometry (every crop in list order, each inside the previous box, then
 * rot90, hflip, vflip composed into one output -> source map, bilinear with half-pixel centres and clamped borders; a map
 * without a crop is integer and reads one texel), the pixel ops 6-8 in list order, blur, noise, then v / 255.f.  Float32 on
 * the 0..255 scale, clipped to [0, 255] after every op.  Rejected before a launch: n_ops > 8, an unknown opcode, p outside
 * [0, 1], a repeated non-pixel op, rot90 with h != w, blur_limit > 7, limits out of order, null pointers.
 * RNG: u(op i, draw j) = top 24 bits of rng_u32(seed, batch_no * 65536 + row, 32 i + j) / 2^24 (csrc/common.h); draw 0
 *   decides firing (u < p); noise element e = (y w + x) c_in + ch uses b = 2^32 + 2 (e / 2) and + 1 for a Box-Muller pair
 *   (cos for even e, sin for odd).  A row's values depend on (seed, batch_no, row) only.
 * TABLE: float32 [n][embnet_augment_param_floats() = 48], 16-byte aligned:
 *   0-3 crop box x0, y0, w, h in source pixels ((0, 0, w, h) = no crop); 4 hflip; 5 vflip; 6 rot90 k; 7 blur k (0 = off);
 *   8 noise sigma; 9 noise fired; 10 number of ops fired; 11-14 CLAHE's (below; zero unless it fired); 15 zero;
 *   16 + 4 i .. 19 + 4 i, op i: { opcode if it fired else 0, s0, s1, s2 }: rrc (w, h, attempt 1-10 or 0 = fallback),
 *   center_crop (w, h), rot90 (k), brightness_contrast (alpha, beta), gamma (gamma), hsv (dh, ds, dv), blur (k),
 *   gauss_noise (sigma, variance); zeros for ops not fired or beyond n_ops.
 * APPLY: src uint8 [*, h, w, c_in] (1 <= c_in <= 4), index as embnet_u8_to_f32, dst float32 [n, h, w, c_out] (c_out <= 16,
 *   zero padding), table from embnet_augment_params for the same (n, h, w).  seed and batch_no key the noise.  An image with
 *   no op fired is bit for bit what embnet_u8_to_f32(denom = 255) writes.  n <= 65535, 4 <= h, w <= 16384.
 *   embnet_augment_apply ignores table fields 11-14: given a table with CLAHE it writes the output without CLAHE. */
size_t embnet_augment_param_floats(void);
int embnet_augment_params(const float* ops, int n_ops, uint64_t seed, uint64_t batch_no, int n, int h, int w, float* table,
                          void* stream);
int embnet_augment_apply(const void* src, const int32_t* index, int n, int h, int w, int c_in, int c_out, const float* table,
                         uint64_t seed, uint64_t batch_no, float* dst, void* stream);
/* CLAHE (opcode 11): OpenCV's 8-bit CLAHE (cv::createCLAHE(clip, grid).apply, what albumentations' A.CLAHE calls), kept out of
 * the 8 op slots so that no other op's record, draw or table field moves.
 * RECORD: { 11, p, clip_lo, clip_hi, gx, gy, 0, 0 } (tile_grid_size = (gx columns, gy rows), cv::Size order) plus pos = the
 *   number of other ops listed before it.  Rejected before a launch: p outside [0, 1], not 0 < clip_lo <= clip_hi, gx or gy not
 *   an integer in 1..16, 2 gx > w or 2 gy > h (the pad stays below the image size), pos outside [0, n_ops], c_in not 1 or 3.
 * DRAWS: RNG op index 8 (no slot uses it, so every other op draws what it draws without CLAHE): fires if u(8, 0) < p (b = 256);
 *   clip = clip_lo + (clip_hi - clip_lo) u(8, 1) in float32 (b = 257).  Only when it fires: field 10 counts it, 11 = clip,
 *   12 = pos, 13 = gx, 14 = gy; a row where it did not fire is bit for bit the row of the list without it.
 * ORDER: geometry -> pixel ops in slots < pos -> CLAHE -> pixel ops in slots >= pos -> blur -> noise -> / 255.
 * VALUE equalised: 1 channel: v itself.  3 channels: L* of the pixel read as BGR (as the HSV op reads it; albumentations calls
 *   COLOR_RGB2LAB on cv2's BGR arrays, so the two differ as for HSV), scaled by 255/100.  OpenCV's float Lab: c = v / 255,
 *   linear = c <= 0.04045 ? c / 12.92 : ((c + 0.055) / 1.055)^2.4, OpenCV's D65 sRGB->XYZ matrix, X /= 0.950456, Z /= 1.088754,
 *   f(t) = t > 0.008856 ? cbrt(t) : 7.787 t + 16/116, L = Y > 0.008856 ? 116 cbrt(Y) - 16 : 903.3 Y, a = 500 (f(X) - f(Y)),
 *   b = 200 (f(Y) - f(Z)).  bin = rint(clamp(L8, 0, 255)).
 * TILES: if w % gx or h % gy is non-zero, BOTH axes are padded at the bottom / right with reflect-101 by g - size % g (an axis
 *   that divides gains a full g: OpenCV's copyMakeBorder quirk); tw = padded_w / gx, th = padded_h / gy; padded pixels count.
 * LUT per tile: clip = max(1, (int)((double)clip * tw th / 256)); each bin is clipped at clip and the excess summed; excess / 256
 *   is added to every bin, then 1 to bins 0, step, 2 step, ... until excess % 256 is used up (step = max(256 / remainder, 1));
 *   LUT[i] = saturate(rint((float)cumsum_i * (255.f / (tw th)))), round half even, bytes.
 * MAPPING of output pixel (y, x): txf = x (1.f / tw) - 0.5f, tx1 = floor(txf), xa = txf - tx1, tx2 = min(tx1 + 1, gx - 1),
 *   tx1 = max(tx1, 0), the same for y; res = (L11 (1 - xa) + L12 xa)(1 - ya) + (L21 (1 - xa) + L22 xa) ya, each L that tile's
 *   LUT at the pixel's bin, float32, not rounded.  1 channel: v = res.  3 channels: L* = res 100/255 with the pixel's own a*, b*
 *   back through OpenCV's float Lab -> XYZ -> BGR (linear values clipped to [0, 1], then the inverse companding), * 255, clipped.
 *   Halo pixels of a blur get CLAHE at their own (reflected) coordinates.
 * ENTRY POINTS: embnet_augment_params_clahe = embnet_augment_params plus the CLAHE draws (clahe_rec NULL: exactly
 *   embnet_augment_params).  embnet_augment_clahe_luts writes uint8 luts[n][gy][gx][256] (embnet_augment_clahe_lut_bytes,
 *   4-byte aligned) for the rows where CLAHE fired and leaves the other rows untouched; gx, gy are the record's.
 *   embnet_augment_apply_clahe = embnet_augment_apply with the CLAHE stage, reading those LUTs; c_in 1 or 3. */
int embnet_augment_params_clahe(const float* ops, int n_ops, const float* clahe_rec, int clahe_pos, uint64_t seed,
                                uint64_t batch_no, int n, int h, int w, float* table, void* stream);
size_t embnet_augment_clahe_lut_bytes(int n, int gx, int gy);
int embnet_augment_clahe_luts(const void* src, const int32_t* index, int n, int h, int w, int c_in, int gx, int gy,
                              const float* table, void* luts, void* stream);
int embnet_augment_apply_clahe(const void* src, const int32_t* index, int n, int h, int w, int c_in, int c_out, const float* table,
                               const void* luts, int gx, int gy, uint64_t seed, uint64_t batch_no, float* dst, void* stream);

/* Dense (backbones.py:35,72,75,114,116; models.py:44): x[m,in], w[in,out], y[m,out].
 * workspace (optional, may be NULL/0): >= embnet_dense_fwd_workspace_bytes lets a forward with few output tiles and a long
 * reduction (simple2's Flatten -> Dense(512): 12 800 x 512 at batch 32) cut K over workgroups (partial slabs + fixed-order
 * sum with bias / ReLU); 0 bytes = this shape runs unsplit. */
size_t embnet_dense_fwd_workspace_bytes(int m, int in, int out);
int embnet_dense_fwd_f32(const float* x, const float* w, const float* bias, float* y, int m, int in, int out,
                         int relu, void* workspace, size_t workspace_bytes, void* stream);
int embnet_dense_dgrad_f32(const float* dy, const float* w, float* dx, int m, int in, int out, void* stream);
int embnet_dense_wgrad_f32(const float* x, const float* dy, float* dw, int m, int in, int out, void* stream);

/* BatchNormalization over the last axis of x[m,c] (backbones.py:46-69; zoo ResNet BN with eps 2e-5).
 * train: biased batch variance; moving <- momentum*moving + (1-momentum)*batch (updated in place, may
 * be NULL); gamma NULL = scale=False; relu = fused activation after the affine: 0 none, 1 ReLU, 2 swish
 * (backward recomputes it from x, nothing extra is stored).  save_mean/save_rstd/scale/shift
 * ([c] each) are kept by the caller for backward.  y may be NULL (statistics and scale/shift only, for a
 * fused consumer).  partial_in (NULL, or [2][c][partial_rows] sums / sums of squares of x over disjoint row
 * sets, e.g. from conv2d_fwd's epilogue) replaces the kernel's own read of x for the statistics. */
size_t embnet_bn_workspace_bytes(long m, int c);
int embnet_bn_train_fwd(const float* x, long m, int c, const float* gamma, const float* beta, float eps,
                        float momentum, int relu, float* y, float* save_mean, float* save_rstd, float* scale,
                        float* shift, float* moving_mean, float* moving_var, const float* partial_in,
                        int partial_rows, void* workspace, size_t workspace_bytes, void* stream);
/* _ex: y_bound (NULL or [c]) receives, per channel, an upper bound of |act(scale_c x + shift_c)| over the batch (RANGE SLOT above);
 * y_range (NULL or a range slot; needs y_bound and y): their maximum, as the range slot of y;  xhat_bound (NULL or [c]): an upper
 * bound of |x - mean_c| rstd_c — what embnet_bn_bwd_ex needs to bound its dx without a dry run. */
int embnet_bn_train_fwd_ex(const float* x, long m, int c, const float* gamma, const float* beta, float eps,
                           float momentum, int relu, float* y, float* save_mean, float* save_rstd, float* scale,
                           float* shift, float* moving_mean, float* moving_var, const float* partial_in,
                           int partial_rows, void* workspace, size_t workspace_bytes, float* y_bound, uint32_t* y_range,
                           float* xhat_bound, void* stream);
/* BatchNormalization (training) of x[m,c] with c % 4 != 0 whose output y[m,cp] has cp = 4 * ceil(c / 4) channels (the image batch
 * in front of the zoo ResNet stem, 3 -> 4): two passes over x — statistics, then act(scale x + shift) written widened — with the
 * results of embnet_pad_channels followed by embnet_bn_train_fwd_ex on the widened copy, bit for bit, without that copy.
 * gamma / beta / the moving statistics / every output row have cp entries (the pad channels' statistics are those of zeros);
 * workspace >= embnet_bn_workspace_bytes(m, cp); y is required. */
int embnet_bn_train_fwd_pad_ex(const float* x, long m, int c, int cp, const float* gamma, const float* beta, float eps,
                               float momentum, int act, float* y, float* save_mean, float* save_rstd, float* scale,
                               float* shift, float* moving_mean, float* moving_var, void* workspace, size_t workspace_bytes,
                               float* y_bound, uint32_t* y_range, float* xhat_bound, void* stream);
int embnet_bn_infer_fwd(const float* x, long m, int c, const float* gamma, const float* beta,
                        const float* moving_mean, const float* moving_var, float eps, int relu, float* y,
                        float* scale, float* shift, void* stream);
/* dx_add (NULL or [m,c]) is added to dx: the gradient that reaches x through its other consumer (the identity
 * shortcut of a residual unit), so autograd needs no separate accumulation pass. */
int embnet_bn_bwd(const float* dy, const float* x, long m, int c, const float* save_mean, const float* save_rstd,
                  const float* scale, const float* shift, int relu, int training, const float* dx_add, float* dx,
                  float* dgamma, float* dbeta, void* dx_planes, void* workspace, size_t workspace_bytes, void* stream);
/* _ex: dx_range (NULL or a range slot of embnet_range_slot_words() words) receives max |dx| of the fp32 dx (RANGE SLOT) — exact, or,
 * where dx is also written as planes from a bound, that bound.
 * xhat_bound ([c] from embnet_bn_train_fwd_ex, or NULL), dx_add_range (the range slot of dx_add, or NULL): with dx_planes in the
 * two-piece format the planes' scale then comes from an upper bound of |dx| —
 *   |scale_c| (max |dz| + |dbeta_c| / m + xhat_bound_c |dgamma_c| / m)  [+ the range of dx_add],
 * max |dz| per channel being a third output of the reduction pass — instead of from a DRY RUN of the apply pass (8 B per element
 * read once more: round 5's form, still taken when either pointer is missing). */
int embnet_bn_bwd_ex(const float* dy, const float* x, long m, int c, const float* save_mean, const float* save_rstd,
                     const float* scale, const float* shift, int relu, int training, const float* dx_add, float* dx,
                     float* dgamma, float* dbeta, void* dx_planes, void* workspace, size_t workspace_bytes, uint32_t* dx_range,
                     const float* xhat_bound, const uint32_t* dx_add_range, void* stream);
/* BatchNorm backward of a layer whose output is also globally average-pooled (the squeeze-and-excite block of the EfficientNet
 * MBConv, reference backbones.py:84-98): the output gradient is dy[n,p,c] + dpool[n,c] / hw; both passes form it on the fly with
 * embnet_gap_bwd's arithmetic (the result of embnet_gap_bwd(dx_add = dy) followed by embnet_bn_bwd to the last bits), so the
 * summed tensor is never written.  gate (NULL or [n,c]): dy is the gradient of the GATED tensor y * gate (embnet_channel_scale_fwd)
 * and the scaling's backward multiply is applied here too — its caller then only needs embnet_channel_scale_dgate.
 * Training statistics, c % 4 == 0; workspace as embnet_bn_bwd. */
int embnet_bn_bwd_gap(const float* dy, const float* dpool, const float* gate, int n, int hw, const float* x, int c, const float* save_mean,
                      const float* save_rstd, const float* scale, const float* shift, int relu, float* dx, float* dgamma,
                      float* dbeta, void* workspace, size_t workspace_bytes, void* stream);
/* Squeeze-and-excite backward without a BatchNorm reduction pass.  embnet_se_bn_sums: ONE pass over dg = d(gated tensor) and the
 * BatchNormalization's input x gives sums[n][5][c]: row 0 = the gate's gradient sum_p dg * act(BN(x)) (what
 * embnet_channel_scale_dgate computes from the stored activation), rows 1..4 = sum_p of a' dg, a', a' dg xhat, a' xhat
 * (a' = act'(BN(x))).  embnet_bn_bwd_gap_sums: dbeta / dgamma from those rows, the gate and the pooled gradient (the layer's
 * output gradient is a' (dg gate + dpool / hw), linear in the two per-(n,c) factors), then embnet_bn_bwd_gap's apply pass. */
int embnet_se_bn_sums(const float* dg, const float* x, int n, int hw, int c, const float* save_mean, const float* save_rstd,
                      const float* scale, const float* shift, int act, float* sums, void* stream);
int embnet_bn_bwd_gap_sums(const float* dy, const float* dpool, const float* gate, const float* sums, int n, int hw, const float* x,
                           int c, const float* save_mean, const float* save_rstd, const float* scale, const float* shift, int relu,
                           float* dx, float* dgamma, float* dbeta, void* stream);
/* BatchNorm backward whose column sums came from the data gradient of the conv that consumed this layer's output
 * (embnet_conv2d_dgrad_bnsums_f32 below): partials [2][c][rows] -> dbeta / dgamma (added in double), then the apply pass of
 * embnet_bn_bwd.  Training statistics, c % 4 == 0. */
int embnet_bn_bwd_partials(const float* dy, const float* x, long m, int c, const float* save_mean, const float* save_rstd,
                           const float* scale, const float* shift, int relu, const float* partials, int rows,
                           const float* dx_add, float* dx, float* dgamma, float* dbeta, void* dx_planes, void* stream);
/* _ex: partial_kinds = 3: partials is [3][c][rows], the third plane holding max |dz| per row band (what
 * embnet_conv2d_dgrad_bnsums_f32_ex writes): with xhat_bound / dx_add_range as for embnet_bn_bwd_ex, no dry run. */
int embnet_bn_bwd_partials_ex(const float* dy, const float* x, long m, int c, const float* save_mean, const float* save_rstd,
                              const float* scale, const float* shift, int relu, const float* partials, int rows,
                              const float* dx_add, float* dx, float* dgamma, float* dbeta, void* dx_planes, uint32_t* dx_range,
                              int partial_kinds, const float* xhat_bound, const uint32_t* dx_add_range, void* stream);
/* BatchNorm backward for a BN whose input x is the output of a layer with a fused ReLU (conv -> ReLU -> BN, the small
 * backbones' block): dz = d(x) * [x > 0] (the gradient the producer's data / weight gradients consume, ReLU backward
 * included) and dbias[c] = column sums of dz (the producer's bias gradient), in the pass that computes d(x).  c % 4 == 0. */
int embnet_bn_bwd_inrelu(const float* dy, const float* x, long m, int c, const float* save_mean, const float* save_rstd,
                         const float* scale, const float* shift, int relu, int training, float* dz, float* dgamma,
                         float* dbeta, float* dbias, void* workspace, size_t workspace_bytes, void* stream);
/* ABI 22 — the same with `dz_range` (NULL or a RANGE SLOT): the exact max |dz| in its first word, for the producer's data and
 * weight gradient on three products */
int embnet_bn_bwd_inrelu_ex(const float* dy, const float* x, long m, int c, const float* save_mean, const float* save_rstd,
                            const float* scale, const float* shift, int relu, int training, float* dz, float* dgamma,
                            float* dbeta, float* dbias, void* workspace, size_t workspace_bytes, uint32_t* dz_range, void* stream);
/* dx_planes (NULL, or 3*m*c bf16, c % 16 == 0): dx ALSO as the pre-split planes embnet_conv2d_patch_f32 takes (below) —
 * the gradient of the convolution output in front of this BatchNormalization, i.e. that convolution's data-gradient operand.
 * With dx_planes given, dx may be NULL (embnet_bn_bwd, embnet_bn_bwd_partials; c % 4 == 0): the fp32 tensor is not written —
 * for a convolution that takes both its data gradient (embnet_conv2d_patch_f32) and its weight gradient
 * (embnet_conv2d_wgrad_planes_f32) from the planes. */

/* y = act(x*scale[c] + shift[c]) on x[m,c]: the apply half of BatchNormalization on its own (scale/shift from
 * bn_train_fwd / bn_infer_fwd with y = NULL), for a deferred BN output whose consumer cannot fuse it. */
int embnet_affine_act(const float* x, long m, int c, const float* scale, const float* shift, int act, float* y,
                      void* stream);

/* MaxPool2D (backbones.py:23,26,29: 2x2/2; zoo ResNet: ZeroPadding2D(1) + 3x3/2).  Taps outside the
 * image read 0 and take no gradient.  argmax[n,oh,ow,c] (uint8) is kept for backward. */
int embnet_maxpool_fwd(const float* x, int n, int h, int w, int c, int k, int stride, int pad, int oh, int ow,
                       float* y, uint8_t* argmax, void* stream);
/* ABI 22 — the same with `y_range` (NULL, or a RANGE SLOT of embnet_range_slot_words() words, c % 4 == 0): the exact max |y| of the
 * pooled tensor is left in its first word, for the three-product conv that reads y (the `simple` backbone's conv -> ReLU -> pool
 * blocks have no BatchNormalization whose statistics could bound the activation; reference backbones.py:21-31). */
int embnet_maxpool_fwd_ex(const float* x, int n, int h, int w, int c, int k, int stride, int pad, int oh, int ow,
                          float* y, uint8_t* argmax, uint32_t* y_range, void* stream);
int embnet_maxpool_bwd(const float* dy, const uint8_t* argmax, int n, int h, int w, int c, int k, int stride,
                       int pad, int oh, int ow, float* dx, void* stream);
/* embnet_maxpool_bwd followed by embnet_relu_bwd_colsum in one pass, for the conv -> ReLU -> MaxPool blocks of the
 * 'simple' backbone (reference backbones.py:21-31): y is the pool's input (the Conv2D's ReLU output); dz[n,h,w,c] is the
 * gradient w.r.t. the Conv2D's pre-activation, dbias[c] its column sums.  The scattered full-size gradient never exists
 * (8 + 5/stride^2 bytes per element of y instead of 16 + 5/stride^2).  dz equals the two-call result bit for bit; dbias is
 * the same sum in another fp32 order.  c % 4 == 0, n*h*w < 2^31; workspace >= embnet_bn_workspace_bytes(n*h*w, c). */
int embnet_maxpool_relu_bwd_colsum(const float* dy, const uint8_t* argmax, const float* y, int n, int h, int w, int c,
                                   int k, int stride, int pad, int oh, int ow, float* dz, float* dbias, void* workspace,
                                   size_t workspace_bytes, void* stream);
/* ABI 22 — the same with `dz_range` (NULL or a RANGE SLOT): the exact max |dz| in its first word, for the conv's data and
 * weight gradient on three products. */
int embnet_maxpool_relu_bwd_colsum_ex(const float* dy, const uint8_t* argmax, const float* y, int n, int h, int w, int c,
                                      int k, int stride, int pad, int oh, int ow, float* dz, float* dbias, void* workspace,
                                      size_t workspace_bytes, uint32_t* dz_range, void* stream);

/* BatchNorm-apply + activation + ZeroPadding2D(pad) + MaxPool(k,stride) in one pass (the zoo ResNet stem
 * bn0 -> relu -> pad -> pool, reference backbones.py:99-104 via image-classifiers).  scale/shift come from
 * embnet_bn_train_fwd / embnet_bn_infer_fwd called with y = NULL.  Backward takes the POOLED gradient and
 * returns dx (w.r.t. the BN input), dgamma, dbeta; the activation tensor and its gradient never exist.
 * c % 4 == 0.  Same results as bn -> maxpool (sums in a different fp32 order).
 * xwin (optional, [n,oh,ow,c]): forward also stores the BN input at each window's winning tap; handing it to backward
 * turns the dgamma/dbeta reduction's gather through the arg-max into a streaming read (188 -> ~60 us on the ResNet stem). */
int embnet_bn_act_maxpool_fwd(const float* x, int n, int h, int w, int c, const float* scale, const float* shift, int act,
                              int k, int stride, int pad, int oh, int ow, float* y, uint8_t* argmax, float* xwin,
                              void* stream);
size_t embnet_bn_act_maxpool_bwd_workspace_bytes(int n, int oh, int ow, int c);
int embnet_bn_act_maxpool_bwd(const float* dy, const uint8_t* argmax, const float* x, int n, int h, int w, int c, int k,
                              int stride, int pad, int oh, int ow, const float* save_mean, const float* save_rstd,
                              const float* scale, const float* shift, int act, int training, const float* xwin, float* dx,
                              float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream);
int embnet_bn_act_maxpool_bwd_ex(const float* dy, const uint8_t* argmax, const float* x, int n, int h, int w, int c, int k,
                                 int stride, int pad, int oh, int ow, const float* save_mean, const float* save_rstd,
                                 const float* scale, const float* shift, int act, int training, const float* xwin, float* dx,
                                 float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, uint32_t* dx_range,
                                 void* stream);
/* _band_ex: band_rows > 0 runs the dx pass on bands of that many consecutive input rows per workgroup (the pooled rows that
 * neighbouring input rows share stay in one CU's cache); 0 is _ex.  dx, dgamma, dbeta and dx_range do not depend on it. */
int embnet_bn_act_maxpool_bwd_band_ex(const float* dy, const uint8_t* argmax, const float* x, int n, int h, int w, int c, int k,
                                      int stride, int pad, int oh, int ow, const float* save_mean, const float* save_rstd,
                                      const float* scale, const float* shift, int act, int training, const float* xwin,
                                      float* dx, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                                      uint32_t* dx_range, int band_rows, void* stream);

/* GlobalAveragePooling2D (backbones.py:111): x[n,hw,c] -> y[n,c]. */
/* act(x*scale + shift) -> y AND its per-image channel means -> gap[n,c], one pass (the BatchNormalization + swish in front
 * of a squeeze-and-excite block, whose pooling reads what the BN writes); scale/shift from embnet_bn_train_fwd(y = NULL). */
/* y = drop_n(x*scale + shift) + skip: the BatchNormalization apply, the per-sample drop-connect (embnet_sample_dropout's mask) and the
 * residual Add of an MBConv block (reference backbones.py:84-98) in one pass; factor [n,c] receives 1/(1-rate) or 0 per sample —
 * the gate of embnet_bn_bwd_gap for the backward (dpool = zeros).  rate = 0: a plain BatchNorm apply + Add. */
int embnet_affine_drop_add(const float* x, int n, int hw, int c, const float* scale, const float* shift, float rate, uint64_t seed,
                           const uint64_t* seed_add_dev, const float* skip, float* y, float* factor, void* stream);
/* y = act(x*scale + shift) * gate[n,c] in one pass (the BatchNormalization apply and the squeeze-and-excite multiply; the pooled
 * means the gate was computed from come from embnet_affine_act_gap with y = NULL, so the activated tensor is never written). */
int embnet_affine_act_scale(const float* x, int n, int hw, int c, const float* scale, const float* shift, int act,
                            const float* gate, float* y, void* stream);
int embnet_affine_act_gap(const float* x, int n, int hw, int c, const float* scale, const float* shift, int act, float* y,
                          float* gap, void* stream);
int embnet_gap_fwd(const float* x, int n, int hw, int c, float* y, void* stream);
int embnet_gap_bwd(const float* dy, int n, int hw, int c, const float* dx_add, float* dx, void* stream);   /* dx_add (NULL or
    [n,hw,c], c % 4 == 0): gradient of x's other consumer, summed in the same pass */

/* Generalised-mean pooling (GeM, Radenovic et al., TPAMI 2019; no reference code: the reference pools with the mean only):
 * y[n,c] = (mean_hw max(x, eps)^p)^(1/p) on x[n,hw,c].  The exponent is read from DEVICE memory, p[0] when p_stride == 0 and
 * p[ch * p_stride] (p_stride == 1: one exponent per channel) otherwise; the host never reads it, so a captured launch replays
 * with whatever the exponent holds then.  p > 0 and eps > 0 (eps is checked, p cannot be: with p <= 0 or NaN the results are
 * undefined, though nothing is written out of bounds).
 * The arithmetic, per (sample, channel), all fp32 (library log2f / exp2f, IEEE division, no fast-math forms):
 *   z_i = fmaxf(x_i, eps);  M = max_i z_i;  r_i = z_i / M  in (0, 1];  l_i = log2f(r_i);  e_i = exp2f(p * l_i);
 *   s = (sum_i e_i) / hw;   y = M * exp2f(log2f(s) / p).
 * The sum is normalised by the maximum, so no power overflows or flushes at any amplitude with eps / M >= 2^-126: every e_i is
 * in (0, 1] and the largest is exactly 1.  With `dydp` ([n,c], NULL: not formed) the same pass gives
 *   t = (sum_i e_i * (l_i * ln2)) / hw;   dydp = y * (t / (p * s) - (log2f(s) * ln2) / (p * p)) = dy/dp   (M cancels).
 * Summation order over hw (fixed by the shape alone, never by the scheduling):  c % 4 == 0 (gem_fwd4_kernel: one workgroup per
 * sample and 64 channels, 16 channel quads x 16 pixel lanes): lane j adds its pixels j, j + 16, ... in ascending order from 0,
 * then the 16 lane sums are added in ascending lane order from lane 0's.  c % 4 != 0 (gem_fwd_kernel, one thread per (sample,
 * channel)): pixels in ascending order.  x is read from memory once while hw <= 144 (nine pixels per lane stay in registers);
 * beyond that the second sweep reads it again.
 * bwd:  dx_i = (dy / hw) * exp2f((p - 1) * log2f(z_i / y)) where x_i >= eps, exactly 0 where x_i < eps (torch.clamp's gradient);
 * z_i / y <= hw^(1/p), so nothing overflows.  x, dy, y and dx may not alias.  With `dp` (then dydp is required; NULL: no
 * reduction is launched) the exponent's gradient, summed in float64 in a fixed order and rounded once:
 *   p_stride == 0: dp[0] = sum_{n,c} dy * dydp;   p_stride == 1: dp[ch] = sum_n dy * dydp.
 * Order: per channel the samples j, j + 16, ... ascending in 16 lanes, the lanes ascending; p_stride == 0: then the 16 channels of
 * a workgroup ascending, the workgroups' partials in 256 strided chains and block_sum256's tree.  No floating-point atomics.
 * workspace >= embnet_gem_bwd_workspace_bytes(c) when dp is given (else it may be NULL), 16-byte aligned, its first 16 bytes
 * ZERO before the first launch (the arrival ticket, which re-arms itself); one workspace serves one stream at a time.
 * n <= 65535. */
int embnet_gem_fwd(const float* x, int n, int hw, int c, const float* p, int p_stride, float eps, float* y, float* dydp,
                   void* stream);
size_t embnet_gem_bwd_workspace_bytes(int c);
int embnet_gem_bwd(const float* dy, const float* x, const float* y, const float* p, int p_stride, float eps, int n, int hw, int c,
                   float* dx, const float* dydp, float* dp, void* workspace, size_t workspace_bytes, void* stream);

/* Elementwise helpers of the backward pass and the residual blocks. */
int embnet_relu_bwd(const float* dy, const float* y, long total, float* dz, void* stream);   /* dz = dy*[y>0] */
/* the same on dy/y[m,c] plus dbias[c] = column sums of dz, one pass (Conv2D / Dense with bias and a fused ReLU);
 * workspace >= embnet_colsum_workspace_bytes(m, c) */
int embnet_relu_bwd_colsum(const float* dy, const float* y, long m, int c, float* dz, float* dbias, void* workspace,
                           size_t workspace_bytes, void* stream);
/* ABI 22 — the same with `dz_range` (NULL or a RANGE SLOT): the exact max |dz| in its first word */
int embnet_relu_bwd_colsum_ex(const float* dy, const float* y, long m, int c, float* dz, float* dbias, void* workspace,
                              size_t workspace_bytes, uint32_t* dz_range, void* stream);
size_t embnet_colsum_workspace_bytes(long m, int c);
int embnet_colsum(const float* x, long m, int c, float* out, void* workspace, size_t workspace_bytes,
                  void* stream);                                                                /* bias grads */
int embnet_add(const float* a, const float* b, long total, float* y, void* stream);           /* Add() */
int embnet_scale(const float* x, long total, float alpha, const float* alpha_dev, float* y, void* stream);
/* out[c] = sum_{tap,k} w[tap,c,k] * tap_sums[tap,k]: gradient of a per-channel offset added to a conv
 * input (the zoo ResNet's bn_data beta) from per-tap sums of dy — avoids a full 3-channel dgrad. */
int embnet_tap_contract(const float* w, const float* tap_sums, int taps, int c, int k, float* out, void* stream);
/* tap_sums[r,s,k] for embnet_tap_contract when dy[n,oh,ow,k] sums to zero over the pixels of every channel (dy is the
 * data gradient of a training-mode BatchNormalization: the zoo ResNet's bn0 behind conv0): the sum over the pixels
 * whose tap (r,s) is inside the image = minus the sum over those whose tap falls into the padding — border strips
 * only (row sums + column sums - corners), 6 % of the tensor for the 7x7/2 stem.  The caller vouches for the zero-sum
 * property. */
size_t embnet_tap_border_sums_workspace_bytes(int n, int oh, int ow, int k, int r, int s, int stride, int pad_t, int pad_l,
                                              int h, int w);
int embnet_tap_border_sums(const float* dy, int n, int oh, int ow, int k, int r, int s, int stride, int pad_t, int pad_l,
                           int h, int w, float* tap_sums, void* workspace, size_t workspace_bytes, void* stream);
/* y[pixels,cout] = [x[pixels,cin] | 0]: widens 3-channel images to 4 channels for 16-byte stem gathers. */
int embnet_pad_channels(const float* x, long pixels, int cin, int cout, float* y, void* stream);
/* ABI 22 — the same with `y_range` (NULL or a RANGE SLOT): the exact max |x| of the image batch in its first word */
int embnet_pad_channels_ex(const float* x, long pixels, int cin, int cout, float* y, uint32_t* y_range, void* stream);
/* Dropout (backbones.py:53,64,73): inverted scaling, counter-based mask from (seed, index). */
int embnet_dropout(const float* x, long total, float rate, uint64_t seed, const uint64_t* seed_add_dev, float* y,
                   void* stream);   /* seed_add_dev (NULL or device uint64): added to seed — a replayed HIP graph draws a new mask per step */
/* A Dropout layer directly behind a BatchNormalization (simple2's bn3 -> drop1, bn6 -> drop2: backbones.py:52-55,63-66)
 * riding on the BatchNormalization's passes, with embnet_dropout's mask and arithmetic (bit-identical to the two
 * layers run separately):  forward  y = dropout(act(x*scale + shift));  backward  embnet_bn_bwd_inrelu with
 * dy := dropout_backward(dy) applied as dy is read. */
int embnet_affine_act_dropout(const float* x, long m, int c, const float* scale, const float* shift, int act, float rate,
                              uint64_t seed, const uint64_t* seed_add_dev, float* y, void* stream);
int embnet_bn_bwd_inrelu_dropout(const float* dy, const float* x, long m, int c, const float* save_mean,
                                 const float* save_rstd, const float* scale, const float* shift, int relu, int training,
                                 float rate, uint64_t seed, const uint64_t* seed_add_dev, float* dz, float* dgamma,
                                 float* dbeta, float* dbias, void* workspace, size_t workspace_bytes, void* stream);
int embnet_bn_bwd_inrelu_dropout_ex(const float* dy, const float* x, long m, int c, const float* save_mean,
                                    const float* save_rstd, const float* scale, const float* shift, int relu, int training,
                                    float rate, uint64_t seed, const uint64_t* seed_add_dev, float* dz, float* dgamma,
                                    float* dbeta, float* dbias, void* workspace, size_t workspace_bytes, uint32_t* dz_range,
                                    void* stream);                                         /* ABI 22: + dz_range, as above */
/* ---- EfficientNet MBConv pieces (backbones.py:84-98, `efficientnet` zoo package) and the siamese 'l1' head ---- */
/* DepthwiseConv2D: x[n,h,w,c], w[r,s,c] (Keras depthwise_kernel [r,s,c,1]), y[n,oh,ow,c]; padding as conv2d. */
int embnet_dwconv2d_fwd_f32(const float* x, const float* w, float* y, int n, int h, int wd, int c, int r, int s,
                            int stride, int pad_t, int pad_l, int oh, int ow, void* stream);
/* DepthwiseConv2D forward that also writes the statistics partials [2][c][P] (sum, sum of squares of y per channel, one row per
 * workgroup; P = embnet_dwconv2d_fwd_stats_rows(...), 0 = not available for the geometry) of the BatchNormalization that follows
 * (embnet_bn_train_fwd's `partials`): that layer then does not read y for its statistics.  Every (channel, row) is written
 * (since ABI 19; earlier, wide layers — c / 4 > 256 — wanted `stats` zeroed first, which remains harmless). */
int embnet_dwconv2d_fwd_stats_rows(int n, int c, int r, int s, int stride, int oh, int ow);
int embnet_dwconv2d_fwd_stats_f32(const float* x, const float* w, float* y, int n, int h, int wd, int c, int r, int s, int stride,
                                  int pad_t, int pad_l, int oh, int ow, float* stats, void* stream);
int embnet_dwconv2d_dgrad_f32(const float* dy, const float* w, float* dx, int n, int h, int wd, int c, int r, int s,
                              int stride, int pad_t, int pad_l, int oh, int ow, void* stream);
/* Depthwise data gradient (stride 1 or 2) that also emits the BatchNorm-backward sums of the layer in front of the depthwise conv (its
 * input was act(bn_x*bn_scale + bn_shift): an MBConv block's expand BatchNormalization), as embnet_conv2d_dgrad_bnsums_f32 does
 * for the gather convs: bn_partial [2][c][bn_rows], bn_rows = embnet_dwconv2d_dgrad_bnsums_rows(...) (0: not available);
 * every (channel, row) of bn_partial is written (ABI 19; zeroing it first, as wide layers once required, stays harmless).  For
 * embnet_bn_bwd_partials. */
int embnet_dwconv2d_dgrad_bnsums_rows(int n, int h, int wd, int c, int r, int s, int stride);
int embnet_dwconv2d_dgrad_bnsums_f32(const float* dy, const float* w, float* dx, int n, int h, int wd, int c, int r, int s,
                                     int stride, int pad_t, int pad_l, int oh, int ow, const float* bn_x, const float* bn_scale,
                                     const float* bn_shift, const float* bn_mean, const float* bn_rstd, int bn_act,
                                     float* bn_partial, int bn_rows, void* stream);
size_t embnet_dwconv2d_wgrad_workspace_bytes(int n, int c, int r, int s, int oh, int ow);
int embnet_dwconv2d_wgrad_f32(const float* x, const float* dy, float* dw, void* workspace, size_t workspace_bytes,
                              int n, int h, int wd, int c, int r, int s, int stride, int pad_t, int pad_l, int oh,
                              int ow, void* stream);
/* kind 0 = sigmoid, 1 = swish (x*sigmoid(x)); backward recomputes from x. */
int embnet_activation_fwd(const float* x, long total, int kind, float* y, void* stream);
int embnet_activation_bwd(const float* x, const float* dy, long total, int kind, float* dx, void* stream);
/* squeeze-excite multiply: y[n,p,c] = x[n,p,c]*s[n,c]; bwd gives dx and ds[n,c]. */
int embnet_channel_scale_fwd(const float* x, const float* s, int n, int hw, int c, float* y, void* stream);
/* ds[n,c] = sum_p dy * x only (embnet_channel_scale_bwd without dx: see embnet_bn_bwd_gap's gate).  c % 4 == 0. */
int embnet_channel_scale_dgate(const float* x, const float* dy, int n, int hw, int c, float* ds, void* stream);
int embnet_channel_scale_bwd(const float* x, const float* s, const float* dy, int n, int hw, int c, float* dx,
                             float* ds, void* stream);
/* drop-connect: Dropout with noise_shape (None,1,1,1): one keep/drop decision per sample, inverted scaling. */
int embnet_sample_dropout(const float* x, long total, long per_sample, float rate, uint64_t seed,
                          const uint64_t* seed_add_dev, float* y, void* stream);
/* models.py:218 L1 layer: y = |a - b|. */
int embnet_absdiff_fwd(const float* a, const float* b, long total, float* y, void* stream);
int embnet_absdiff_bwd(const float* a, const float* b, const float* dy, long total, float* da, float* db,
                       void* stream);

/* kernel_regularizer=l2(lambda) (backbones.py:22-36): *out = alpha * sum x^2. */
/* All regularisers of a model in one launch pair: *out = sum_t alpha_t * sum(x_t^2).
 *   table   device array of n_tensors descriptors, 24 bytes each: { const float* x; int64 n; float alpha; int32 pad; }
 *   chunks  device int32 [n_chunks][2] = (tensor index, chunk index), chunk = embnet_sumsq_chunk_elems() elements
 *   workspace >= n_chunks floats. */
int embnet_sumsq_chunk_elems(void);
int embnet_sumsq_multi(const void* table, int n_tensors, const int32_t* chunks, int n_chunks, float* out, void* workspace,
                       size_t workspace_bytes, void* stream);
size_t embnet_sumsq_workspace_bytes(void);
int embnet_sumsq(const float* x, long total, float alpha, float* out, void* workspace, size_t workspace_bytes,
                 void* stream);

/* The same loss path in ONE launch for small batches (the sizes the reference trains at): distances of each class's K
 * anchors to all N = p*k rows (sklearn arithmetic, kept in LDS), mine-and-select (mode as embnet_mine_triplets, or
 * EMBNET_MINE_BATCH_HARD), squared-L2 hinge of each selected triplet, and — by the last workgroup to finish — compaction
 * in pair order, the reference's fallback triplet and the mean.  Stands in for datagenerators.py:219,225-250 +
 * losses_and_accuracies.py:26-42 (+ Keras' mean), i.e. for embnet_pairwise_dist_f32 + embnet_mine_triplets +
 * embnet_triplet_gather_fwd, and writes the same outputs (triplets[T,3], count, selected[pairs], loss[max_t],
 * active[max_t], mean_loss), so embnet_triplet_gather_bwd is the backward of both.  batch-hard: T = N, one triplet per
 * anchor, `selected` unused; triplets/loss/active must hold N rows.
 * embnet_fused_loss_supported: 1 when N <= 512, k <= 16 and k*(e+N) floats fit 64 KiB of LDS.
 * workspace (embnet_fused_loss_workspace_bytes): zero-filled ONCE by the caller; every launch leaves its counter zeroed.
 * seed_dev (NULL or a device uint64): the seed of the random rules read from device memory instead of `seed`, so that
 * a captured HIP graph of the training step draws new negatives at every replay. */
int embnet_fused_loss_supported(int p, int k, int e);
size_t embnet_fused_loss_workspace_bytes(int p, int k);
int embnet_fused_triplet_loss_fwd(const float* emb, int p, int k, int e, float margin, int mode, uint64_t seed,
                                  const uint64_t* seed_dev, int32_t* triplets, int32_t* count, int32_t* selected,
                                  float* loss, float* active, float* mean_loss, void* workspace, size_t workspace_bytes,
                                  void* stream);

/* Batch-all triplet loss (Moindrot; Hermans et al. name it beside batch-hard; README.md cites both, the reference has no
 * code for it): build-defined, selected as TripletTrainer(negatives_selection_mode="batch_all").  Additions only: the ABI
 * version stays 22, since no existing entry point changed and older callers never see these symbols.
 *   emb[n,e], n = p*k class-contiguous; d(i,j) = sum_c (x_ic - x_jc)^2; valid triplets (a,p,n): p in a's class, p != a,
 *   n in another class, T = n (k-1) (n-k).  b = (d(a,p) - d(a,n)) + margin; ACTIVE iff b > 0 (strict; the `active` flags
 *   of the selection rules above use b >= 0).  A = #active:
 *     *n_active = A,  *frac_active = A / T,  *mean_loss = sum_active b / max(A, 1)   (0 when A = 0)
 *     pair_w[n][n]: W[a,p] = #{n : (a,p,n) active}, W[a,n] = -#{p : (a,p,n) active}, 0 elsewhere (integers, exact)
 *   bwd, A held constant: demb_i = (2 g / max(A,1)) * sum_j (W_ij + W_ji) (x_i - x_j), g = *upstream (NULL = 1); A is read
 *   from n_active in device memory.
 * Range: p >= 2, k >= 2, n <= 4096, 1 <= e <= 4096 and T <= 2^31 - 1 (n_active is int32; at n = 4096 that is k <= 128);
 * anything else is rejected before a launch.  path: 0 = auto (embnet_batch_all_path), EMBNET_BATCH_ALL_PER_CLASS = one launch,
 * a workgroup per class with the distances in LDS in the difference form (n <= 512, k <= 16, k*(e+n) floats in 64 KiB),
 * EMBNET_BATCH_ALL_DISTANCE_MATRIX = embnet_pairwise_dist_f32(squared) into the workspace (Gram-form rounding) + a sweep
 * launch over the anchor rows.  The backward is one launch (f64 matrix instructions: every product of an integer weight and
 * an fp32 x is exact).  No floating-point atomics: bitwise reproducible; no host synchronisation or allocation.
 * workspace (embnet_batch_all_workspace_bytes, either path, 16-byte aligned): zero-filled ONCE by the caller; every launch
 * leaves its arrival counter zeroed. */
enum { EMBNET_BATCH_ALL_PER_CLASS = 1, EMBNET_BATCH_ALL_DISTANCE_MATRIX = 2 };
int embnet_batch_all_path(int p, int k, int e);          /* the path `auto` takes; 0 outside the range */
size_t embnet_batch_all_workspace_bytes(int p, int k, int e);
int embnet_batch_all_loss_fwd(const float* emb, int p, int k, int e, float margin, int path, float* pair_w,
                              int32_t* n_active, float* frac_active, float* mean_loss, void* workspace,
                              size_t workspace_bytes, void* stream);
int embnet_batch_all_loss_bwd(const float* emb, int n, int e, const float* pair_w, const int32_t* n_active,
                              const float* upstream, float* demb, void* stream);

/* Multi-similarity loss (Wang et al., CVPR 2019: the pair-based baseline of "A Metric Learning Reality Check", whose metrics
 * embnet_retrieval_* report; the reference has no pair-based loss): build-defined, selected as
 * TripletTrainer(negatives_selection_mode="multi_similarity").  Additions only: the ABI version stays 22.
 *   Inputs.  emb[n,e] fp32, n = p*k; rows c*k .. c*k+k-1 are class c.
 *   Similarity.  S_ij = sum_c x_ic x_jc: the cosine similarity of the L2-normalised rows the backbones produce; unit rows are
 *     not required.
 *   Parameters.  alpha > 0, beta > 0, base (the paper's lambda), epsilon >= 0; the Python layers default to 2, 50, 0.5, 0.1.
 *   Pair sets of anchor i.  Positives P_i: the other rows of its class.  Negatives N_i: the rows of other classes.
 *   Mining, one rounding form (the fp32 add of epsilon to the negative's similarity):
 *     a negative n is kept iff fl(S_in + epsilon) > min_{p in P_i} S_ip;
 *     a positive p is kept iff fl(max_{n in N_i} S_in + epsilon) > S_ip.
 *     fl is monotone, so an anchor keeps both a positive and a negative (it is ACTIVE) or nothing.  The kept sets are constants
 *     for the backward.
 *   Per-anchor loss.  t+_p = -alpha (S_ip - base) over kept positives, t-_n = beta (S_in - base) over kept negatives,
 *     l_i = (1/alpha) log(1 + sum_p e^{t+_p}) + (1/beta) log(1 + sum_n e^{t-_n}),
 *     each logarithm in the stable form: with m = max(0, max t) the term is m + log(e^{-m} + sum e^{t-m}), so unnormalised
 *     embeddings cannot overflow.  *mean_loss = (1/n) sum_i l_i; inactive anchors contribute 0.
 *   Pair weights pair_g[n][n], the derivative of l_i by S_ij (without the 1/n); all n*n entries are written:
 *     G[i,p] = -e^{t+_p - m+} / (e^{-m+} + sum e^{t+ - m+}) for kept positives,
 *     G[i,n] = +e^{t-_n - m-} / (e^{-m-} + sum e^{t- - m-}) for kept negatives, 0 elsewhere, the diagonal included.  Every
 *     row's positive part and negative part each have an absolute sum below 1.
 *   Backward.  demb_i = (g / n) sum_j (G_ij + G_ji) x_j, g = *upstream (NULL = 1).
 *   Counters.  counts[4], int32, exact: {kept positives, kept negatives, active anchors, kept positives + kept negatives}.
 * Range: p >= 2, k >= 2, n <= 4096, 1 <= e <= 4096; alpha, beta finite and positive, base finite, epsilon finite and
 * non-negative; anything else is rejected before a launch.  path: 0 = auto (embnet_ms_loss_path), EMBNET_MS_PER_CLASS = one
 * launch, a workgroup per class with its similarity rows in LDS (per-lane fma chain over the columns + wave sum; n <= 512,
 * k <= 16, k*(e+n) floats in 64 KiB), EMBNET_MS_SIMILARITY_MATRIX = S = X X^T through embnet_dense_dgrad_f32 (a k-ordered fp32
 * chain per element) into the workspace + a sweep launch over the anchor rows.  The backward is one launch on the f64 matrix
 * instructions: one fp32 rounding of an f64 sum.  No floating-point atomics, every reduction in a fixed order: bitwise
 * reproducible; no host synchronisation or allocation.
 * workspace (embnet_ms_loss_workspace_bytes, either path, 16-byte aligned): zero-filled ONCE by the caller; every launch leaves
 * its arrival counter zeroed. */
enum { EMBNET_MS_PER_CLASS = 1, EMBNET_MS_SIMILARITY_MATRIX = 2 };
int embnet_ms_loss_path(int p, int k, int e);             /* the path `auto` takes; 0 outside the range */
size_t embnet_ms_loss_workspace_bytes(int p, int k, int e);   /* sized for either path; 0 outside the range */
int embnet_ms_loss_fwd(const float* emb, int p, int k, int e, float alpha, float beta, float base, float epsilon, int path,
                       float* pair_g, int32_t* counts, float* mean_loss, void* workspace, size_t workspace_bytes,
                       void* stream);
int embnet_ms_loss_bwd(const float* emb, int n, int e, const float* pair_g, const float* upstream, float* demb,
                       void* stream);

/* SupCon / NT-Xent (the softmax / InfoNCE family of the Reality Check's loss table; the reference has no such loss):
 * build-defined, selected as TripletTrainer(negatives_selection_mode="supcon").  Additions only: the ABI version stays 22.
 *   Inputs.  emb[n,e] fp32, n = p*k; rows c*k .. c*k+k-1 are class c.  S = X X^T; unit rows are not required.
 *   Pair sets of anchor i.  Positives P_i: the other rows of its class, |P_i| = k-1.  Negatives N_i: the rows of other classes.
 *   Parameters.  temperature tau, positive and finite, with fl(1/tau) a normal fp32 number; denominator EMBNET_SUPCON_ALL or
 *     EMBNET_SUPCON_NEGATIVES.  The Python layers default to 0.1 and `all`.
 *   Logit.  t_ij = S_ij / tau, in ONE rounding form: t_ij = fl(S_ij * r) with r = fl(1/tau), one correctly rounded division taken
 *     once per call.  r > 0 and fl is monotone: the order of the logits is the order of S.
 *   EMBNET_SUPCON_ALL (SupCon: Khosla et al., NeurIPS 2020, the L_out form).
 *     l_i = lse_{a != i} t_ia - (1/(k-1)) sum_{p in P_i} t_ip,
 *     G_ij = dl_i/dS_ij = (1/tau) (softmax_{a != i}(t_i.)_j - [j in P_i] / (k-1)),  G_ii = 0.
 *   EMBNET_SUPCON_NEGATIVES (NT-Xent as "A Metric Learning Reality Check" and pytorch-metric-learning define it: the denominator
 *     holds the pair itself and the anchor's negatives only).  d_ip = e^{t_ip} + sum_{n in N_i} e^{t_in},
 *     l_ip = log d_ip - t_ip,  l_i = (1/(k-1)) sum_p l_ip,
 *     G_ip = (1/tau) (1/(k-1)) (e^{t_ip} / d_ip - 1),  G_in = (1/tau) (1/(k-1)) e^{t_in} sum_p 1 / d_ip,  G_ii = 0.
 *   Stable forms (part of the contract: every logarithm takes an argument >= 1, so no input of finite S overflows or takes
 *     log 0).  `all`: with M = max_{a != i} t_ia,  l_i = log(sum_{a != i} e^{t_ia - M}) + (1/(k-1)) sum_p (M - t_ip).
 *     `negatives`: the maximum is PER PAIR, m_ip = max(t_ip, max_n t_in):
 *     l_ip = (m_ip - t_ip) + log(e^{t_ip - m_ip} + e^{max_n t_in - m_ip} sum_n e^{t_in - max_n t_in}).
 *   Common.  *mean_loss = (1/n) sum_i l_i.  pair_g[n][n] = G (without the 1/n); all n*n entries are written; every row of G sums
 *     to zero in exact arithmetic.  Backward: demb_i = (g / n) sum_j (G_ij + G_ji) x_j, g = *upstream (NULL = 1) — this is
 *     embnet_ms_loss_bwd's contract, and embnet_ms_loss_bwd(emb, n, e, pair_g, upstream, demb, stream) is the backward.
 *   Counters.  counts[2], int32, exact: counts[0] = positive pairs n (k-1); counts[1] = violating anchors, the anchors with
 *     max_{n in N_i} S_in >= min_{p in P_i} S_ip on the device's fp32 S (it goes to zero as the classes separate).
 * Range: p >= 2, k >= 2, n <= 4096, 1 <= e <= 4096; anything else is rejected before a launch.  path: 0 = auto
 * (embnet_supcon_loss_path), EMBNET_SUPCON_PER_CLASS, EMBNET_SUPCON_SIMILARITY_MATRIX: the two forward paths, the fit rule and the
 * workspace of embnet_ms_loss_fwd (the kernels share one skeleton, csrc/pair_loss.h).  No floating-point atomics, every
 * reduction in a fixed order: bitwise reproducible; no host synchronisation or allocation.
 * workspace (embnet_supcon_loss_workspace_bytes, either path, 16-byte aligned): zero-filled ONCE by the caller; every launch
 * leaves its arrival counter zeroed. */
enum { EMBNET_SUPCON_ALL = 1, EMBNET_SUPCON_NEGATIVES = 2 };
enum { EMBNET_SUPCON_PER_CLASS = 1, EMBNET_SUPCON_SIMILARITY_MATRIX = 2 };
int embnet_supcon_loss_path(int p, int k, int e);         /* the path `auto` takes; 0 outside the range */
size_t embnet_supcon_loss_workspace_bytes(int p, int k, int e);   /* sized for either path; 0 outside the range */
int embnet_supcon_loss_fwd(const float* emb, int p, int k, int e, float temperature, int denominator, int path, float* pair_g,
                           int32_t* counts, float* mean_loss, void* workspace, size_t workspace_bytes, void* stream);

/* FastAP and Smooth-AP (the ranking family of the Reality Check's loss table: smooth surrogates of the average precision of each
 * anchor's ranked list, the quantity embnet_retrieval_* reports as MAP@R; the reference has no such loss): build-defined,
 * selected as TripletTrainer(negatives_selection_mode="fast_ap" | "smooth_ap").  Additions only: the ABI version stays 22.
 *   Inputs.  emb[n,e] fp32, n = p*k; rows c*k .. c*k+k-1 are class c.  S = X X^T, computed as embnet_ms_loss_fwd computes it.
 *   Pair sets of anchor i.  Positives P_i: the other rows of its class, |P_i| = k-1.  Negatives N_i: the rows of other classes.
 *   FastAP (Cakir et al., CVPR 2019).  bins = L, a whole number in [2, 64]; the Python layers default to 10.  Rows are expected
 *     L2-normalised, so that d = 2 - 2 S lies in [0, 4]; nothing requires it.
 *     Position of a pair, ONE rounding form: inv = L / 4 (exact in fp32), d = fl(2 - 2 S_ij), u = fl(d inv), l0 = floor(u),
 *     f = u - l0 (exact).  The pair adds fl(1 - f) to bin l0 and f to bin l0 + 1 of the anchor's histogram h+ (j in P_i) or h-
 *     (j in N_i); the bins are 0 .. L and a bin index outside that range is dropped.  This is the triangular pulse
 *     max(0, 1 - |d - l Delta| / Delta), Delta = 4 / L, used as it is for a d outside [0, 4]; a d exactly on a centre belongs to
 *     the interval on its right.
 *     Hp_l, Hn_l: the running sums of h+, h- from bin 0 up; H_l = Hp_l + Hn_l.
 *     F_i = sum_{l : H_l > 0} h+_l Hp_l / H_l,   l_i = 1 - F_i / (k-1).
 *     b_l = h+_l Hp_l / H_l^2,  c_l = h+_l Hn_l / H_l^2 (this is h+_l / H_l - b_l, formed without the subtraction); both are 0
 *     where H_l = 0, which is every bin below the anchor's smallest distance.
 *     A-_m = -sum_{l >= m} b_l,   A+_m = Hp_m / H_m + sum_{l >= m} c_l (the quotient 0 where H_m = 0);  A outside 0 .. L is 0.
 *     G_ij = dl_i/dS_ij = (2 inv / (k-1)) (A^c_{l0+1} - A^c_{l0}),  c = + for j in P_i, - for j in N_i;  G_ii = 0.
 *     A pair whose u is within the rounding of S of a whole number may take either neighbouring interval: the histogram is
 *     continuous across a centre, the pair's own G_ij is not.  The rows of G do not sum to zero.
 *   Smooth-AP (Brown et al., ECCV 2020).  temperature tau, positive and finite, with fl(1/tau) a normal fp32 number; the Python
 *     layers default to 0.01.  k <= 65 (k-1 <= 64 positives; anything above is rejected).
 *     r = fl(1/tau), one correctly rounded division taken once per call.  For a positive p and a column j not in {i, p}:
 *     z_pj = fl(fl(S_ij - S_ip) r),  t = e^{-|z|},  s_pj = sigma(z) = 1 / (1 + t) for z >= 0 and t / (1 + t) otherwise,
 *     s'_pj = r t / (1 + t)^2.  The subtraction 1 - s is never used.
 *     R_p = 1 + sum_{q in P_i, q != p} s_pq,  Nn_p = sum_{n in N_i} s_pn,  Q_p = R_p + Nn_p  (the ranks of p among the positives and
 *     among all),  U_p = sum_{q in P_i, q != p} s'_pq,  Tn_p = sum_{n in N_i} s'_pn,  T_p = U_p + Tn_p.
 *     l_i = 1 - (1/(k-1)) sum_p R_p / Q_p.
 *     G_ij = (1/(k-1)) [ sum_{p in P_i, p != j} s'_pj (R_p / Q_p^2 - [j in P_i] / Q_p) + [j in P_i] (U_j / Q_j - R_j T_j / Q_j^2) ],
 *     G_ii = 0, evaluated as R_p / Q_p^2 - 1 / Q_p = -Nn_p / Q_p^2 and U_j / Q_j - R_j T_j / Q_j^2 = (U_j Nn_j - R_j Tn_j) / Q_j^2.
 *     Every row of G sums to zero in exact arithmetic.
 *   Common.  *mean_loss = (1/n) sum_i l_i.  pair_g[n][n] = G (without the 1/n); all n*n entries are written.  Backward:
 *     demb_i = (g / n) sum_j (G_ij + G_ji) x_j, g = *upstream (NULL = 1) — this is embnet_ms_loss_bwd's contract, and
 *     embnet_ms_loss_bwd(emb, n, e, pair_g, upstream, demb, stream) is the backward.
 *   Counters.  counts[2], int32, exact: counts[0] = positive pairs n (k-1); counts[1] = violating anchors, the anchors with
 *     max_{n in N_i} S_in >= min_{p in P_i} S_ip on the device's fp32 S (embnet_supcon_loss_fwd's counter).
 * Range: p >= 2, k >= 2, n <= 4096, 1 <= e <= 4096, and the parameter ranges above; anything else is rejected before a launch.
 * path: 0 = auto (embnet_*_ap_loss_path), EMBNET_AP_PER_CLASS, EMBNET_AP_SIMILARITY_MATRIX: the two forward paths, the fit rule and
 * the workspace of embnet_ms_loss_fwd (the kernels share one skeleton, csrc/pair_loss.h).  No floating-point atomics, every sum
 * in a fixed order: bitwise reproducible; no host synchronisation or allocation.
 * workspace (embnet_*_ap_loss_workspace_bytes, either path, 16-byte aligned): zero-filled ONCE by the caller; every launch leaves
 * its arrival counter zeroed. */
enum { EMBNET_AP_PER_CLASS = 1, EMBNET_AP_SIMILARITY_MATRIX = 2 };
int embnet_fast_ap_loss_path(int p, int k, int e);        /* the path `auto` takes; 0 outside the range */
size_t embnet_fast_ap_loss_workspace_bytes(int p, int k, int e);   /* sized for either path; 0 outside the range */
int embnet_fast_ap_loss_fwd(const float* emb, int p, int k, int e, int bins, int path, float* pair_g, int32_t* counts,
                            float* mean_loss, void* workspace, size_t workspace_bytes, void* stream);
int embnet_smooth_ap_loss_path(int p, int k, int e);      /* the path `auto` takes; 0 outside the range */
size_t embnet_smooth_ap_loss_workspace_bytes(int p, int k, int e);   /* sized for either path; 0 outside the range */
int embnet_smooth_ap_loss_fwd(const float* emb, int p, int k, int e, float temperature, int path, float* pair_g, int32_t* counts,
                              float* mean_loss, void* workspace, size_t workspace_bytes, void* stream);

/* Proxy-Anchor (Kim et al., CVPR 2020) and CosFace / NormSoftmax (Wang et al., CVPR 2018; Zhai & Wu, BMVC 2019): the proxy /
 * classification family of the Reality Check's loss table, a batch scored against one learnable vector per class (the reference
 * has no such loss): build-defined, selected as ProxyTrainer(loss="proxy_anchor" | "proxy_softmax").  Additions only: the ABI
 * version stays 22.
 *   Inputs.  emb[n,e] fp32, proxies[c,e] fp32, labels[n] int32: general labels, the batch need not be class-contiguous.  A label
 *     outside [0, c) marks an UNLABELLED sample: it belongs to no set, its column (Proxy-Anchor) or row (CosFace) of G is zero
 *     and it receives no gradient.  A label value is compared, and used as an index only after the check 0 <= y < c has
 *     passed (the guard in the kernels is what keeps every label value from reading or writing out of bounds: it stays); there
 *     is no host check of the labels.
 *   Similarity, ONE rounding form.  ss_c = sum_k w_ck^2 in f64, in k order;  q_c = (float)(1.0 / sqrt(ss_c)), q_c = 0 when
 *     ss_c = 0 (a zero proxy has S = 0 and gets no gradient);  D_ic = the fp32 dot product of x_i and w_c;  S_ic = fl(D_ic q_c).
 *     Embedding rows are used as they are (unit rows are not required); proxies are normalised by q only.  q[c] is an output of
 *     the forward and an input of the backward.
 *   EMBNET_PROXY_ANCHOR (a = alpha > 0, b = delta; the Python layers default to 32 and 0.1; G stored [c][n]).
 *     P_c = {i : y_i = c},  N_c = the labelled samples with y_i != c,  C+ = {c : P_c not empty}.
 *     t+_ci = -alpha (S_ci - delta) = fl(-alpha fl(S_ci - delta)),  t-_ci = alpha (S_ci + delta) = fl(alpha fl(S_ci + delta)),
 *     loss = (1/|C+|) sum_{c in C+} log(1 + sum_{P_c} e^{t+}) + (1/c) sum_c log(1 + sum_{N_c} e^{t-});
 *     an empty sum gives log 1 = 0, the first term is 0 when C+ is empty.  Stable form (multi-similarity's): every logarithm is
 *     m + log(e^{-m} + sum e^{t - m}) with m = max(0, max t), its argument >= 1: unnormalised embeddings cannot overflow.
 *     G_ci = -(alpha/|C+|) e^{t+ - m+} / (e^{-m+} + sum) on P_c,  +(alpha/c) e^{t- - m-} / (e^{-m-} + sum) on N_c,  0 elsewhere.
 *   EMBNET_PROXY_SOFTMAX (a = scale sigma > 0, b = margin mu; the Python layers default to 64 and 0.35; mu = 0 is NormSoftmax;
 *     G stored [n][c]).  For a labelled sample i of class y:  t_ic = sigma (S_ic - mu [c = y]) = fl(sigma fl(S_iy - mu)) for c = y
 *     and fl(sigma S_ic) otherwise;  l_i = lse_c t_ic - t_iy in the stable form log(sum_c e^{t_ic - M}) + (M - t_iy), M = max_c t_ic
 *     (the logarithm's argument is >= 1);  loss = (1/n_l) sum l_i over the n_l labelled samples, 0 when n_l = 0.
 *     G_ic = (sigma/n_l)(e^{t_ic - M} / sum - [c = y]);  an unlabelled row is zero.
 *   Common.  *mean_loss = loss.  pair_g = dloss/dS, normalisers included, every entry written.  Backward, g = *upstream (NULL = 1),
 *     Q_ci = q_c G_ci:  demb = g Q^T W (Proxy-Anchor) or g Q W (CosFace);  Y_c = sum_i G_ci x_i,
 *     dproxies_c = g q_c (Y_c - q_c^2 (Y_c . w_c) w_c).  The sums run on the f64 matrix instructions; every output element is one
 *     fp32 rounding of an f64 expression.
 *   Counters.  counts[3], int32, exact on the device's fp32 S:  counts[0] = anchors that carry a positive term (|C+| for
 *     Proxy-Anchor, n_l for CosFace);  counts[1] = labelled samples;  counts[2] = violating anchors, which go to zero as the classes
 *     separate: the c in C+ with N_c not empty and max_{N_c} S >= min_{P_c} S (Proxy-Anchor), the labelled i with
 *     max_{c != y} S_ic >= S_iy (CosFace).
 * Range: 2 <= n <= 4096, 2 <= c <= 16384, 1 <= e <= 4096; a and b finite, a > 0; kind one of the two; anything else is rejected
 * before a launch.  path: 0 = auto (embnet_proxy_loss_path), EMBNET_PROXY_SMALL = a prep launch (q, class sizes) and one launch
 * in which a workgroup holds four anchors and their rows of D in LDS (per-lane fma chain over the columns + wave sum; it needs
 * e + max(n, c) <= 4096 and n c e <= 2^25), EMBNET_PROXY_MATRIX = prep, D through embnet_dense_dgrad_f32 (a k-ordered fp32
 * chain per element) into the workspace and a sweep launch in which one wave walks one anchor's row of D.  The backward is three
 * launches, four where few samples meet many classes (demb's class sum is then split into slices added in slice order).  No floating-point atomics, every reduction in a fixed order: bitwise reproducible; no host synchronisation or
 * allocation.
 * workspace (embnet_proxy_loss_workspace_bytes, either path and the backward, 16-byte aligned; 4 c n + 8 c e bytes and a few per
 * anchor): zero-filled ONCE by the caller; every launch leaves its arrival counter zeroed.  The backward uses it as scratch
 * only: it need not be the forward's. */
enum { EMBNET_PROXY_ANCHOR = 1, EMBNET_PROXY_SOFTMAX = 2 };
enum { EMBNET_PROXY_SMALL = 1, EMBNET_PROXY_MATRIX = 2 };
int embnet_proxy_loss_path(int n, int c, int e);          /* the path `auto` takes; 0 outside the range */
size_t embnet_proxy_loss_workspace_bytes(int n, int c, int e);    /* sized for either path and the backward; 0 outside the range */
int embnet_proxy_loss_fwd(const float* emb, const float* proxies, const int32_t* labels, int n, int c, int e, int kind, float a,
                          float b, int path, float* pair_g, float* q, int32_t* counts, float* mean_loss, void* workspace,
                          size_t workspace_bytes, void* stream);
int embnet_proxy_loss_bwd(const float* emb, const float* proxies, int n, int c, int e, int kind, const float* pair_g,
                          const float* q, const float* upstream, float* demb, float* dproxies, void* workspace,
                          size_t workspace_bytes, void* stream);

/* SoftTriple (Qian et al., ICCV 2019) and sub-centre ArcFace (Deng et al., CVPR 2019; ECCV 2020): the losses of the Reality Check's
 * table that score a batch against SEVERAL learnable centres per class (the reference has no such loss): build-defined, selected as
 * ProxyTrainer(loss="soft_triple" | "arcface") on a ProxyHead(centers_per_class=kc).  A sample's kc similarities to one class's
 * centres are pooled into one class similarity (ArcFace: their maximum; SoftTriple: their softmax-weighted mean), then a margin
 * softmax runs over the c classes.  Additions only: the ABI version stays 22.
 *   Inputs.  emb[n,e] fp32;  centres[c kc, e] fp32, class-major: row c' kc + j is centre j of class c';  labels[n] int32 with the
 *     proxy losses' rules: a label outside [0, c) marks an UNLABELLED sample, its row of G is zero and it gets no loss and no
 *     gradient; a label is used as an index only behind the range check (the guard in the kernels stays); no host check of labels.
 *   Similarity, the proxy losses' form over the nb = c kc rows.  ss_r = sum_k w_rk^2 in f64, in k order;  q_r = (float)(1.0 /
 *     sqrt(ss_r)), 0 when ss_r = 0;  D_ir = the fp32 dot product of x_i and w_r;  S_ir = fl(D_ir q_r).  Embedding rows are used as
 *     they are.  q[c kc] is an output of the forward and an input of the backward.
 *   Pooling, per sample i and class c' over j < kc (S_j = S_i,c'kc+j).  kc = 1: S' = S exactly, for both kinds.
 *     EMBNET_MPROXY_ARCFACE:  S' = max_j S_j;  p_j = [j = the first j that attains the maximum] (ties go to the smaller j).
 *     EMBNET_MPROXY_SOFT_TRIPLE:  z_j = fl(S_j / gamma),  zm = max_j z_j,  x_j = expf(fl(z_j - zm)),  den = the x_j added in j order
 *       (fp32, >= 1: rows of norm 30 with gamma 0.1 cannot overflow),  num = the chain fma(x_j, S_j, num) in j order,
 *       S' = fl(num / den);  p_j = fl(x_j / den);  dS'/dS_j = fl(p_j fl(1 + fl(fl(S_j - S') / gamma))).
 *   Logits, for a labelled sample of class y.
 *     SOFT_TRIPLE (a = lambda > 0, b = delta; the Python layers default to 20 and 0.01, gamma 0.1, tau 0.2):
 *       t_ic' = fl(lambda fl(S'_iy - delta)) for c' = y and fl(lambda S'_ic') otherwise: with kc = 1 CosFace's rounding form.
 *     ARCFACE (a = scale s > 0, b = margin m, 0 <= m < pi/2; the Python layers default to 64 and 0.5; gamma and tau are ignored):
 *       t_ic' = fl(s S'_ic') off the own class and fl(s phi(S'_iy)) on it.  cm = cos m, sm = sin m, th = cos(pi - m),
 *       mm = sin(pi - m) m are computed ONCE on the host in f64 from (double)m (pi = M_PI) and rounded to fp32.
 *       S' > th:  r = sqrt(max(0, fl(1 - fl(S'^2)))) (a correctly rounded fp32 root),  phi = fl(fl(S' cm) - fl(r sm)); for S' >= 1 this
 *         is S' cm: continuous, no clamp.  Otherwise (the usual non-easy-margin guard):  phi = fl(S' - mm).
 *       phi' = fl(cm + fl(fl(S' sm) / max(r, 2^-10))) for S' > th and r > 0,  cm where r = 0,  1 for S' <= th: the floor on r is what
 *       keeps a sample next to its centre from producing an infinite gradient.  m = 0 is NormSoftmax.
 *   Loss.  l_i = log(sum_c' e^{t_ic' - M}) + (M - t_iy), M = max_c' t_ic' (CosFace's stable form, the logarithm's argument is >= 1);
 *     *mean_loss = (float)((1/n_l) sum l_i + (double)*reg), the sum and the division in f64; the first term is 0 when n_l = 0.
 *   G = pair_g, stored [n][c kc], every entry written:  with v = e^{t - M} / sum - [c' = y] in CosFace's form and k = fl(a / n_l),
 *     G_i,c'j = fl(fl(k v) psi) dS'/dS_j: psi = phi'(S'_iy) multiplies the own class of ArcFace only, dS'/dS_j multiplies where kc > 1
 *     (ArcFace: the whole weight on the argmax, exactly 0 on the others).
 *   SoftTriple's regulariser (the authors' released form; kc > 1 and tau > 0, otherwise *reg = 0 and no launch; always 0 for ArcFace).
 *     g_st = q_s q_t sum_k w_sk w_tk, the sum in f64 in k order;  coef = tau / (c kc (kc - 1));
 *     R = coef sum_c' sum_{s<t} sqrt(max(0, 2 + 1e-5 - 2 g_st)), the pairs of a class added in (s, t) order, the classes in a fixed
 *     order;  H_st = H_ts = -coef / sqrt(2 + 1e-5 - 2 g_st) (|g| <= (1 + 2^-24)^2: the argument stays positive), H_ss = 0.  Everything
 *     in f64;  *reg = (float)R and reg_h[c][kc][kc] = (float)H are fp32 roundings.  reg_h is an output of the forward and an input of
 *     the backward; it may be NULL where there is no regulariser.
 *   Backward, g = *upstream (NULL = 1), Q_ir = q_r G_ir:  demb = g Q W;  Y_r = sum_i G_ir x_i + sum_{t != r, same class} H_rt q_t w_t
 *     (reg_h NULL: no second term);  dcentres_r = g q_r (Y_r - q_r^2 (Y_r . w_r) w_r).  The sums run on the f64 matrix instructions
 *     (the proxy losses' kernels with c := c kc); every output element is one fp32 rounding of an f64 expression.
 *   Counters.  counts[3], int32, exact on the device's fp32 values:  counts[0] = labelled samples n_l;  counts[1] = violating
 *     samples, max_{c' != y} S'_ic' >= S'_iy;  counts[2] = own-class lower-branch samples, S'_iy <= th (0 for SoftTriple).
 * Range: 2 <= n <= 4096, 2 <= c, 1 <= kc <= 32, c kc <= 16384, 1 <= e <= 4096; a finite and > 0; SoftTriple: b finite, gamma finite
 * and > 0, tau finite and >= 0; ArcFace: 0 <= b < pi/2; anything else is rejected before a launch.  path: 0 = auto
 * (embnet_multi_proxy_loss_path), EMBNET_MPROXY_SMALL = a prep launch (q) and one launch in which a workgroup holds four samples and
 * their rows of D in LDS (it needs e + c kc <= 4096 and n c kc e <= 2^25), EMBNET_MPROXY_MATRIX = prep, D through
 * embnet_dense_dgrad_f32 into the workspace and a sweep launch in which one wave walks one sample's row of D; the regulariser is one
 * more launch in front of either.  auto takes the small path where it fits AND c kc < 100 (from 100 centres on the matrix path
 * measured faster at every shape tried).  No floating-point atomics, every reduction in a fixed order: bitwise reproducible; no host
 * synchronisation or allocation, no memset node.
 * workspace (embnet_multi_proxy_loss_workspace_bytes, either path and the backward, 16-byte aligned): zero-filled ONCE by the caller;
 * every launch leaves its arrival counter zeroed.  The backward uses it as scratch only: it need not be the forward's. */
enum { EMBNET_MPROXY_SOFT_TRIPLE = 1, EMBNET_MPROXY_ARCFACE = 2 };
enum { EMBNET_MPROXY_SMALL = 1, EMBNET_MPROXY_MATRIX = 2 };
int embnet_multi_proxy_loss_path(int n, int c, int kc, int e);            /* the path `auto` takes; 0 outside the range */
size_t embnet_multi_proxy_loss_workspace_bytes(int n, int c, int kc, int e);      /* either path and the backward; 0 outside the range */
int embnet_multi_proxy_loss_fwd(const float* emb, const float* centres, const int32_t* labels, int n, int c, int kc, int e, int kind,
                                float a, float b, float gamma, float tau, int path, float* pair_g, float* q, float* reg_h,
                                int32_t* counts, float* mean_loss, float* reg, void* workspace, size_t workspace_bytes, void* stream);
int embnet_multi_proxy_loss_bwd(const float* emb, const float* centres, int n, int c, int kc, int e, const float* pair_g,
                                const float* q, const float* reg_h, const float* upstream, float* demb, float* dcentres,
                                void* workspace, size_t workspace_bytes, void* stream);

/* Cross-Batch Memory (Wang et al., CVPR 2020, "XBM"): the detached embeddings of the last m samples kept in a ring on the device,
 * and the pair losses of a batch against that ring (the reference has no memory): build-defined, selected as
 * XbmTrainer(memory=..., xbm_loss="contrastive" | "multi_similarity").  Additions only: the ABI version stays 22.
 *   The ring.  mem[m,e] fp32 and mem_labels[m] int32 belong to the caller, who initialises them ONCE to 0 and -1 (a negative bank
 *     label marks an empty or unlabelled slot);  *cursor is a DEVICE int32, the next slot to write, initialised once to 0.
 *     embnet_xbm_enqueue: row i of emb[n,e] goes to slot (cursor + i) mod m with labels[i], slots[i] receives that slot, and
 *     afterwards *cursor = (cursor + n) mod m.  1 <= n <= m <= 65536, 1 <= e <= 4096.  The cursor is read from device memory by the
 *     kernel at run time, never passed by value: a captured graph replays on the ring's current state.  It is advanced by the last
 *     workgroup to arrive, after every workgroup has read it: no workgroup sees the advanced value.  One launch, no memset node,
 *     vector stores only.  A cursor word outside [0, m) is taken modulo m as an unsigned number: no value of it addresses memory
 *     outside the ring.  workspace: 16 bytes, 16-byte aligned (the arrival counter).
 *   The loss.  emb[n,e] fp32 batch with labels[n] int32, mem[m,e] / mem_labels[m] the bank (DETACHED: it carries no gradient),
 *     self_slots[n] int32 or NULL.
 *   Similarity.  S_ij = sum_k x_ik y_jk, an fp32 dot product through embnet_dense_dgrad_f32 (a k-ordered chain per element: a rounded
 *     product and a rounded addition per k).  Unit rows are not required.
 *   Pair sets.  Labels are compared by value and never used as an index.  A NEGATIVE label marks an unlabelled batch row or an empty
 *     or unlabelled bank slot: such a row or column belongs to no pair set, its entries of G are zero and it receives no gradient.
 *     Column self_slots[i] is excluded for anchor i (the sample's own copy, just enqueued); a slot outside [0, m), or self_slots
 *     NULL, excludes nothing.  For y_i >= 0:  P_i = {j : z_j = y_i, j != self_i},  N_i = {j : z_j >= 0, z_j != y_i}.
 *   EMBNET_XBM_CONTRASTIVE (the XBM paper's own criterion as its released code has it; a = margin, the Python layers default to 0.5;
 *     b, c, d are ignored).  A positive is kept iff fl(1 - S_ip) > 0 (one fp32 subtraction); its term is fl(1 - S_ip) and G_ip = -1.
 *     A negative is kept iff S_in > margin; its term is S_in and G_in = +1.  l_i = the sum of the kept terms: the fp32 terms join an
 *     f64 sum in a fixed order.  (The released code drops positives with S >= 1 - 1e-5 to get rid of the self pair; here the self
 *     pair is excluded exactly by its slot, and the threshold is 1.)
 *   EMBNET_XBM_MULTI_SIMILARITY (a, b, c, d = alpha > 0, beta > 0, base, epsilon >= 0; defaults 2, 50, 0.5, 0.1).  The mining rule
 *     with its one rounding form, t+ / t-, the stable logarithms, l_i and G are embnet_ms_loss_fwd's, word for word, over P_i and
 *     N_i as above (the kernels share the code: csrc/pair_loss.h).  An anchor with an empty P_i or an empty N_i keeps nothing.
 *   Common.  *mean_loss = (1/n) sum_i l_i, n counting EVERY batch row.  pair_g[n][m] = dl_i/dS_ij (without the 1/n); every entry is
 *     written.  Backward: demb_i = (g / n) sum_j G_ij y_j, g = *upstream (NULL = 1); there is no column role, the bank is a
 *     constant.  The sum runs on the f64 matrix instructions: every element is one fp32 rounding of an f64 sum.
 *   Counters.  counts[4], int32, exact on the device's fp32 S: {kept positives, kept negatives, active anchors (those that keep a
 *     pair), labelled bank slots (z_j >= 0)}.
 * Range: 2 <= n <= 4096, n <= m <= 65536, n m <= 2^26, 1 <= e <= 4096; kind one of the two; margin finite; alpha, beta finite and
 * positive, base finite, epsilon finite and non-negative; anything else is rejected before a launch.  ONE forward path,
 * EMBNET_XBM_SWEEP: S into the workspace, then a sweep launch in which one wave walks one anchor's row of S (a row of 65536 floats
 * does not fit LDS, and at these sizes the rectangle never fits a workgroup the way the proxies' small path does);
 * embnet_xbm_loss_path exists so that a second path can join.  The backward is one launch, two against a long bank: the slot sum
 * is then split into slices whose f64 sums are added in slice order (a workspace of the forward's size holds them where S was).
 * No floating-point atomics, every reduction in a fixed order: bitwise reproducible; no host synchronisation or allocation.
 * workspace (embnet_xbm_loss_workspace_bytes, 16-byte aligned; 4 n m bytes and a few per anchor): zero-filled ONCE by the caller;
 * every launch, the enqueue's included, leaves its arrival counter zeroed.  The backward uses it as scratch only, behind the
 * counter and the partials: it may be the forward's (S is no longer needed) or another. */
enum { EMBNET_XBM_CONTRASTIVE = 1, EMBNET_XBM_MULTI_SIMILARITY = 2 };
enum { EMBNET_XBM_SWEEP = 1 };
int embnet_xbm_enqueue(const float* emb, const int32_t* labels, int n, int e, float* mem, int32_t* mem_labels, int m,
                       int32_t* cursor, int32_t* slots, void* workspace, void* stream);
int embnet_xbm_loss_path(int n, int m, int e);            /* EMBNET_XBM_SWEEP; 0 outside the range */
size_t embnet_xbm_loss_workspace_bytes(int n, int m, int e);      /* 0 outside the range */
int embnet_xbm_loss_fwd(const float* emb, const int32_t* labels, const float* mem, const int32_t* mem_labels,
                        const int32_t* self_slots, int n, int m, int e, int kind, float a, float b, float c, float d,
                        float* pair_g, int32_t* counts, float* mean_loss, void* workspace, size_t workspace_bytes, void* stream);
int embnet_xbm_loss_bwd(const float* mem, int n, int m, int e, const float* pair_g, const float* upstream, float* demb,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Circle loss (Sun et al., CVPR 2020, "Circle Loss: A Unified Perspective of Pair Similarity Optimization"; the pair-wise form, as
 * pytorch-metric-learning's CircleLoss has it; the reference has no such loss): build-defined, in-batch selected as
 * TripletTrainer(negatives_selection_mode="circle") and against the cross-batch memory as XbmTrainer(xbm_loss="circle").
 * Additions only: the ABI version stays 22.
 *   Parameters.  The relaxation m, finite, 0 <= m <= 1; the scale gamma, finite and positive.  The Python layers default to 0.4 and
 *     80 (pytorch-metric-learning's; the paper's face setting is 0.25 / 256).  Derived ONCE per call on the host, one fp32 operation
 *     each:  O+ = fl(1 + m),  O- = -m,  D+ = fl(1 - m),  D- = m.
 *   Similarity.  In-batch: emb[n,e] fp32, n = p*k, rows c*k .. c*k+k-1 are class c; S = X X^T, computed as embnet_ms_loss_fwd
 *     computes it.  Ring: S = X Mem^T through embnet_dense_dgrad_f32, as embnet_xbm_loss_fwd computes it.  Unit rows are not required.
 *   Pair sets of anchor i.  In-batch: P_i the other rows of its class, N_i the rows of other classes.  Ring: by label value, with
 *     negative labels and self_slots, embnet_xbm_loss_fwd's P_i and N_i word for word.
 *   Logits, in ONE rounding form (every fl one fp32 operation):
 *     alpha+_p = max(fl(O+ - S_ip), 0),   a+_p = fl(-gamma fl(alpha+_p fl(S_ip - D+)));
 *     alpha-_n = max(fl(S_in - O-), 0),   a-_n = fl( gamma fl(alpha-_n fl(S_in - D-))).
 *     A pair with alpha = 0 stays in its sum with logit 0 (the paper and the published implementations).
 *   Per-anchor loss.  L+ = lse_p a+_p,  L- = lse_n a-_n, each as M + log sum e^{a - M} with M the side's largest logit, so the
 *     logarithm's argument is >= 1;  z = fl(L+ + L-);  l_i = softplus(z) = max(z, 0) + log(1 + t), t = e^{-|z|}.  An anchor with an
 *     empty P_i or an empty N_i (the ring only) has l_i = 0 and a zero row of G.  *mean_loss = (1/n) sum_i l_i, n counting EVERY
 *     batch row.  The results are finite whenever every logit is finite in fp32.
 *   Pair weights.  alpha is a CONSTANT of the backward (the authors' code and pytorch-metric-learning detach it; this gives the
 *     paper's gradient).  sigma = sigmoid(z) = 1 / (1 + t) for z >= 0, t / (1 + t) otherwise.  With w+ = fl(fl(sigma gamma) / sum+)
 *     and w- = fl(fl(sigma gamma) / sum-), sum the side's sum of e^{a - M}:
 *     G_ip = -fl(w+ fl(alpha+_p e^{a+_p - M+})),   G_in = +fl(w- fl(alpha-_n e^{a-_n - M-})),   0 elsewhere, the diagonal or the
 *     self slot included; every entry of pair_g ([n][n] resp. [n][m_slots], without the 1/n) is written.  G is therefore NOT the
 *     derivative of l_i with alpha free: it lacks the term through d alpha / dS.
 *   Backward.  No entry point of its own.  In-batch: demb_i = (g / n) sum_j (G_ij + G_ji) x_j, embnet_ms_loss_bwd's contract, and
 *     embnet_ms_loss_bwd(emb, n, e, pair_g, upstream, demb, stream) is the backward.  Ring: demb_i = (g / n) sum_j G_ij y_j,
 *     embnet_xbm_loss_bwd as it stands.
 *   Counters, int32, exact on the device's fp32 S.  In-batch counts[3]: {positive pairs n (k-1) <= 4096 * 2047; violating
 *     anchors, max_{n in N_i} S_in >= min_{p in P_i} S_ip (embnet_supcon_loss_fwd's counter) <= n; negatives with alpha- > 0, the
 *     ones that still carry gradient, <= n (n - k) < 2^24}.  Ring counts[4]: {positives with alpha+ > 0, negatives with
 *     alpha- > 0, both over the active anchors and <= n m_slots <= 2^26; active anchors (P_i and N_i both non-empty); labelled
 *     bank slots}.
 * Range.  In-batch: embnet_ms_loss_fwd's (p >= 2, k >= 2, n <= 4096, 1 <= e <= 4096), with its two forward paths
 * (EMBNET_CIRCLE_PER_CLASS, EMBNET_CIRCLE_SIMILARITY_MATRIX; path 0 = auto, embnet_circle_loss_path), its fit rule and its
 * workspace (embnet_circle_loss_workspace_bytes).  Ring: embnet_xbm_loss_fwd's (2 <= n <= 4096, n <= m_slots <= 65536,
 * n m_slots <= 2^26, 1 <= e <= 4096), its one path and its workspace (embnet_xbm_loss_workspace_bytes).  Anything else, a
 * non-finite or out-of-range m or gamma included, is rejected before a launch.  No floating-point atomics, every reduction in a
 * fixed order: bitwise reproducible; no host synchronisation or allocation; capturable in a graph.  Either workspace (16-byte
 * aligned): zero-filled ONCE by the caller; every launch leaves its arrival counter zeroed. */
enum { EMBNET_CIRCLE_PER_CLASS = 1, EMBNET_CIRCLE_SIMILARITY_MATRIX = 2 };
int embnet_circle_loss_path(int p, int k, int e);         /* the path `auto` takes; 0 outside the range */
size_t embnet_circle_loss_workspace_bytes(int p, int k, int e);   /* sized for either path; 0 outside the range */
int embnet_circle_loss_fwd(const float* emb, int p, int k, int e, float m, float gamma, int path, float* pair_g, int32_t* counts,
                           float* mean_loss, void* workspace, size_t workspace_bytes, void* stream);
int embnet_xbm_circle_loss_fwd(const float* emb, const int32_t* labels, const float* mem, const int32_t* mem_labels,
                               const int32_t* self_slots, int n, int m_slots, int e, float m, float gamma, float* pair_g,
                               int32_t* counts, float* mean_loss, void* workspace, size_t workspace_bytes, void* stream);

/* Distance-weighted sampling and the margin loss (Wu, Manmatha, Smola, Kraehenbuehl, ICCV 2017, "Sampling Matters in Deep
 * Embedding Learning"; pytorch-metric-learning's DistanceWeightedMiner and MarginLoss; the reference has no such loss):
 * build-defined, selected as TripletTrainer(negatives_selection_mode="distance_weighted").  Additions only: the ABI version stays 22.
 *   Inputs.  emb[n,e] fp32, n = p*k, rows c*k .. c*k+k-1 are class c; the method assumes unit rows (the weights are the inverse
 *     of the density of pairwise distances on the unit sphere S^(e-1)), the kernels do not require them.
 *   Distance.  d2(i,j) = sum_c (x_ic - x_jc)^2 exactly as embnet_batch_all_loss_fwd forms it on either path (difference form
 *     per class; embnet_pairwise_dist_f32(squared), Gram form, on the matrix path).  D = sqrtf(max(d2, 0)), one fp32 sqrtf; a NaN
 *     stays a NaN.  On the matrix path the Gram form's clamp would turn the NaN of a non-finite row into 0: there a pair with a row
 *     whose squared norm (embnet_pairwise_dist_f32's own) is NaN or infinite has D = NaN.
 *   Parameters.  beta finite; alpha >= 0 finite; cutoff = c_lo and nonzero_loss_cutoff = c_hi finite with 0 < c_lo < c_hi < 2, so
 *     the second logarithm's argument below is positive.  The Python layers default to 1.2, 0.2, 0.5, 1.4 (the paper's).
 *   Weights of anchor i (global row).  An other-class column n is ELIGIBLE iff D_in is not NaN and D_in < c_hi.  In ONE rounding
 *     form, every fl one fp32 operation, logf / expf the device's:
 *       D~ = max(D_in, c_lo),   t = fl(1 - fl(0.25 fl(D~ D~))),   lw_n = fl(fl(a1 logf(D~)) - fl(a2 logf(t))),
 *       a1 = 2 - e and a2 = (e - 3) / 2, both exact in fp32;   M = max lw over the eligible columns, taken exactly;
 *       w_n = expf(fl(lw_n - M)) on eligible columns, exactly 0 elsewhere (own class, the anchor, ineligible).
 *     The maximal column has w = 1 exactly, so total >= 1 whenever a column is eligible; other weights may underflow to 0.
 *   Draws.  The anchor's k-1 positives in ascending column order have ordinals j = 0 .. k-2; each gets one negative, drawn
 *     independently and with replacement:  u_ij = (((rng(seed, i, 2j) << 32) | rng(seed, i, 2j+1)) >> 11) 2^-53  (rng = the
 *     counter generator of the mining rules; the 53-bit form of embnet_kmeans_pp_pick).  Prefix sums in f64, in this order: the
 *     row in chunks of 64 columns ascending (columns >= n weigh 0); inside chunk c the inclusive scan s of the chunk's weights in
 *     column order by doubling steps 1, 2, 4, .. 32 (column l adds the value held l - step columns below it);
 *     P_col = fl(carry_c + s_col), carry_0 = 0, carry_(c+1) = fl(carry_c + s_(c,63)); total = the carry behind the last chunk.
 *     The pick is the first column, in ascending order, with w > 0 and P_col > fl(u total); if rounding leaves none, the last
 *     column with w > 0.  total = 0 (no eligible column): the pick is the floor(u (n-k))-th other-class column in ascending order
 *     (the authors' uniform fall-back).  A zero-weight column is never drawn while total > 0, and every index written lies in
 *     [0, n) whatever the row holds.  seed_dev (NULL or a device uint64) overrides `seed` exactly as in
 *     embnet_fused_triplet_loss_fwd, so a captured step draws new negatives at every replay.
 *   Loss.  l+_ip = max(fl(fl(D_ip - beta) + alpha), 0) for every positive; l-_ij = max(fl(fl(beta - D_in) + alpha), 0) for draw
 *     j's negative n (a NaN distance gives 0).  c+ = #{l+ > 0}, c- = #{l- > 0} over the batch, a draw counting each time it is
 *     drawn; A = c+ + c-.  *mean_loss = (sum l+ + sum l-) / max(A, 1), the sums in f64: per anchor, lane (j mod 64) adds l+ then
 *     l- of ordinal j in ascending j, the 64 lanes fold by the xor butterfly 32, 16, .. 1; then the skeleton's fixed order over
 *     anchors and classes.  counts[3] = {c+, c-, A}: each of c+, c- is at most n (k-1) <= 4096 * 2047 < 2^23, so every partial
 *     and A fit an int32.
 *   Pair weights, pair_w[n][n], every entry written:  W[i,p] = +[l+_ip > 0] fl(1 / D_ip);  W[i,n] = -fl(m / D_in), m = the number
 *     of draws of i that picked n, where l-(D_in) > 0 (the hinge depends on the column alone);  a pair with D = 0 or NaN carries
 *     weight 0 (coincident rows have no direction) and still counts in c+ / c- if its hinge is positive;  0 elsewhere.
 *   Other outputs.  triplets[n (k-1)][3] int32 = (i, p_j, n_ij) in (anchor, ordinal) order, always n (k-1) rows, fit for
 *     embnet_triplet_gather_fwd as they are.  sample_w[n][n] fp32 (NULL skips it): the weights w as the sampler used them; a row of
 *     zeros marks a fall-back anchor.
 *   bwd, A held constant: with dD_ij/dx_i = (x_i - x_j) / D_ij,  demb_i = (g / max(A,1)) sum_j (W_ij + W_ji) (x_i - x_j),
 *     g = *upstream (NULL = 1); A is read from counts[2] in device memory.  One launch on the f64 matrix instructions: every
 *     product of an fp32 weight and an fp32 x is exact in f64.
 * Range: embnet_ms_loss_fwd's (p >= 2, k >= 2, n <= 4096, 1 <= e <= 4096), embnet_batch_all_loss_fwd's two forward paths and fit
 * rule (EMBNET_MARGIN_PER_CLASS, EMBNET_MARGIN_DISTANCE_MATRIX; path 0 = auto, embnet_margin_loss_path).  Anything else, a
 * non-finite or out-of-range parameter included, is rejected before a launch.  No floating-point atomics, every reduction in a
 * fixed order: the same seed gives the same bits; no host synchronisation or allocation; capturable in a graph.
 * workspace (embnet_margin_loss_workspace_bytes, either path, 16-byte aligned): zero-filled ONCE by the caller; every launch
 * leaves its arrival counter zeroed. */
enum { EMBNET_MARGIN_PER_CLASS = 1, EMBNET_MARGIN_DISTANCE_MATRIX = 2 };
int embnet_margin_loss_path(int p, int k, int e);         /* the path `auto` takes; 0 outside the range */
size_t embnet_margin_loss_workspace_bytes(int p, int k, int e);   /* sized for either path; 0 outside the range */
int embnet_margin_loss_fwd(const float* emb, int p, int k, int e, float beta, float alpha, float cutoff, float nonzero_loss_cutoff,
                           uint64_t seed, const uint64_t* seed_dev, int path, float* pair_w, int32_t* counts, int32_t* triplets,
                           float* sample_w, float* mean_loss, void* workspace, size_t workspace_bytes, void* stream);
int embnet_margin_loss_bwd(const float* emb, int n, int e, const float* pair_w, const int32_t* counts, const float* upstream,
                           float* demb, void* stream);

/* ------------------------------------------------------------------ t-SNE of saved encodings
 * utils.py:36-91 plot_tsne / plot_tsne_interactive: `TSNE().fit_transform(encodings['encodings'])` (scikit-learn).  The
 * entries below are scikit-learn's EXACT method (TSNE(method='exact', n_components=2), sklearn/manifold/_t_sne.py and
 * _utils.pyx) restated for the device; embeddingnet_amd/tsne.py drives them with scikit-learn's schedule.  Additions only:
 * the ABI version stays 22.  fp32 storage, 2 <= n <= 32768, P dense [n,n].
 *   embnet_tsne_affinities: d2[n,n] squared distances (embnet_pairwise_dist_f32 with squared != 0) -> p[n,n], beta[n].
 *     Row i: bisection on beta so that the entropy of p_j|i ~ exp(-beta d2_ij), j != i, equals log(perplexity): beta = 1,
 *     at most 100 steps, stop at |H - log perplexity| <= 1e-5, beta doubles / halves while its bracket is open, a zero row
 *     sum becomes 1e-8 (_binary_search_perplexity; the row minimum of d2 is subtracted before exp, which cancels).
 *     sigma_i = sqrt(1 / (2 beta_i)).  Then p = (p_cond + p_cond^T) / S, S = sum of the numerator (computed, fixed order),
 *     max(p, 2.220446e-16) off the diagonal, diagonal 0; p_ij and p_ji are bitwise equal.  p may be the same buffer as d2.
 *     1 <= perplexity < n.
 *   embnet_tsne_iterate: n_iter gradient-descent iterations on y[n,2] with update[n,2] and gains[n,2] (the caller starts
 *     them at 0 and 1): w_ij = 1 / (1 + |y_i - y_j|^2), Z = sum_{i != j} w_ij,
 *       g_i = 4 sum_j (exaggeration p_ij - w_ij / Z) w_ij (y_i - y_j)
 *       inc = (update < 0 and g > 0) or (update > 0 and g < 0)       [the sign of update * g, immune to fp32 underflow]
 *       gains = max(inc ? gains + 0.2 : gains * 0.8, 0.01);  update = momentum update - lr gains g;  y += update
 *     (_gradient_descent).  Two launches per iteration: row sums over p (HBM-bound: 4 n^2 bytes), then the update, whose
 *     workgroups each add the n row sums of w in the same fixed order in f64.  n_iter >= 0.
 *   embnet_tsne_kl: at the current y, *kl = sum_{i != j} p_ij log(max(p_ij, eps) / max(w_ij / Z, eps)) (eps = 2.220446e-16),
 *     *grad_norm = the 2-norm of g (exaggeration 1) over all 2n components, and, when grad != NULL, grad[n,2] = g
 *     (_kl_divergence).  Z, the KL sum and |g|^2 are accumulated in f64.
 * No atomics, every reduction in a fixed order: bitwise reproducible.  workspace >= embnet_tsne_workspace_bytes(n) (0 outside
 * the range of n), 16-byte aligned, no initialisation needed; a short one is refused with -3. */
size_t embnet_tsne_workspace_bytes(int n);
int embnet_tsne_affinities(const float* d2, int n, float perplexity, float* p, float* beta, void* workspace,
                           size_t workspace_bytes, void* stream);
int embnet_tsne_iterate(const float* p, int n, float* y, float* update, float* gains, float exaggeration, float momentum,
                        float lr, int n_iter, void* workspace, size_t workspace_bytes, void* stream);
int embnet_tsne_kl(const float* p, int n, const float* y, float* kl, float* grad_norm, float* grad, void* workspace,
                   size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ optimizer update
 * utils.py:143-153 get_optimizer(name, lr): `Adam(lr)`, `RMSprop(lr)`, `keras_radam.RAdam(lr)`, else `SGD(lr)`
 * with the library defaults — applied by Keras after train.py:160-177's compile/fit.  One launch updates every
 * tensor (multi-tensor apply).
 *   table   device array of n_tensors descriptors, 48 bytes each:
 *             { float* w; const float* g; float* slot1; float* slot2; int64 n; float l2x2; int32 pad; }
 *           g == NULL: the variable got no gradient this step and is skipped (Keras' behaviour);
 *           l2x2 = 2*lambda of the variable's kernel_regularizer=l2(lambda) (backbones.py:22-36), 0 for none: the kernel
 *           uses g + l2x2*w as the gradient (what Keras gets from differentiating loss + regularisers);
 *           slot1/slot2: Adam/RAdam m and v, RMSprop rms (slot2 unused), SGD none — zero-initialised by the caller;
 *   chunks  device int32 [n_chunks][2] = (tensor index, chunk index within it), chunk = embnet_optimizer_chunk_elems()
 *           consecutive elements; every element of every tensor must be covered exactly once;
 *   rule and host-computed scalars (t = 1-based step count):
 *     EMBNET_OPT_SGD         w -= lr*g
 *     EMBNET_OPT_RMSPROP     rms = b1*rms + (1-b1)*g^2;  w -= lr*g/(sqrt(rms)+eps)                 (b1 = rho)
 *     EMBNET_OPT_ADAM        m = b1*m+(1-b1)*g; v = b2*v+(1-b2)*g^2;  w -= c1*m/(sqrt(v)+eps),      c1 = lr*sqrt(1-b2^t)/(1-b1^t)
 *     EMBNET_OPT_RADAM       m, v as Adam;  w -= c1*m/(sqrt(v*c2)+eps),    c1 = lr*r_t/(1-b1^t), c2 = 1/(1-b2^t)   (sma_t >= 5)
 *     EMBNET_OPT_RADAM_WARM  m, v as Adam;  w -= c1*m,                     c1 = lr/(1-b1^t)                          (sma_t < 5)
 *   coef_dev (NULL or device float[6] = lr, b1, b2, eps, c1, c2): the scalars read from device memory instead of the
 *           arguments — a captured HIP graph of the training step replays with the step count's current coefficients.
 * HBM-bound: 12 (SGD) .. 28 (Adam/RAdam) bytes per element. */
enum { EMBNET_OPT_SGD = 0, EMBNET_OPT_RMSPROP = 1, EMBNET_OPT_ADAM = 2, EMBNET_OPT_RADAM = 3, EMBNET_OPT_RADAM_WARM = 4 };
int embnet_optimizer_chunk_elems(void);
int embnet_optimizer_step(int rule, const void* table, int n_tensors, const int32_t* chunks, int n_chunks,
                          float lr, float b1, float b2, float eps, float c1, float c2, const float* coef_dev, void* stream);

/* ------------------------------------------------------------------ optimizer update with parameter groups
 * The same launch over the same table and chunk list, with a learning rate and a decoupled weight decay per parameter group,
 * gradient clipping, and Keras' SGD momentum — what the published recipes of the proxy losses need (Proxy-Anchor: AdamW, the
 * proxies at 100 x the backbone's rate, gradients clipped; SoftTriple: centres at 1e-2 against 1e-4; ArcFace / CosFace: SGD with
 * momentum 0.9 and weight decay 5e-4).  The descriptor keeps its 48 bytes; its trailing int32 is the tensor's group here:
 *             { float* w; const float* g; float* slot1; float* slot2; int64 n; float l2x2; int32 group; }
 * (embnet_optimizer_step goes on ignoring that word.)  A group index outside [0, n_groups) is read as the nearest valid one.
 *   group_coef      HOST float [n_groups][4] = { lr_g, c1_g, d_g, 0 }, 1 <= n_groups <= EMBNET_OPT_MAX_GROUPS, copied into the
 *                   launch arguments: the group's rate, its c1 (the c1 of the rule above at lr_g), and d_g = (float)(lr_g * wd_g);
 *   group_coef_dev  NULL, or the same rows in DEVICE memory, read instead (a captured step replays with current rates);
 *   coef_dev        NULL, or device float[6] as above: b1, b2, eps and c2 are read from it (its lr and c1 are not used);
 *   momentum, nesterov   only with rule EMBNET_OPT_MOMENTUM;
 *   clipvalue       0: off;  > 0: every gradient element is clamped to [-clipvalue, clipvalue];
 *   clip_scale_dev  NULL: off;  else a device float s that every gradient element is multiplied with — the `scale` that
 *                   embnet_optimizer_grad_norm left (global_clipnorm).  The two clips are exclusive.
 * Per element, in this order (fp32):
 *     g' = fma(l2x2, w, g)
 *     clipvalue c > 0:      g' = min(max(g', -c), c)
 *     clip_scale_dev:       g' = g' * s
 *     d_g != 0:             w  = fma(-d_g, w, w)             [Keras AdamW: variable -= variable * wd * lr, before the rule]
 *     the rule with lr_g / c1_g — the five rules above, arithmetic unchanged — or
 *     EMBNET_OPT_MOMENTUM   v = momentum*v - lr_g*g';  w += nesterov ? momentum*v - lr_g*g' : v        (slot1 = v; Keras' SGD)
 * A tensor with g == NULL is skipped entirely: no decay, slots untouched.  Aligned whole chunks go through float4, tails and
 * unaligned tensors element by element.  Bits: a tensor that no option touches (no clip, d_g = 0, one of the five old rules) goes
 * through embnet_optimizer_step's own per-element code at its group's rate, so with one group and no option the result is that
 * entry point's, bit for bit, and several groups without options are as many one-group steps.  Where an option acts (and for the
 * momentum rule) every rounding is pinned — slot updates as one fma each, rms = fma(b1, rms, ((1-b1) g') g'),
 * m = fma(1-b1, g', b1 m), v = fma((1-b2) g', g', b2 v), w = fma(-lr, g', w) for SGD, the velocity as written above with
 * fma(momentum, v, -(lr g')) — and is the same on both paths: a tail or an unaligned tensor gets the bits of a whole aligned chunk.
 * HBM-bound at the same 12 .. 28 bytes per element (the momentum rule: 20).
 *
 * embnet_optimizer_grad_norm: one launch in front of the update when global_clipnorm is set.  A workgroup adds (double)g'^2
 * (g' = fma(l2x2, w, g) in fp32, as the update forms it; w is only read where l2x2 != 0) over one chunk at a time and writes that
 * chunk's partial (0 for a tensor without a gradient); the last workgroup to arrive adds the partials — thread j the partials j, j + 256, ... in ascending
 * order, then the 256 sums in a fixed tree — and writes
 *     norm_out[0] = N2 = sum g'^2,   norm_out[1] = sqrt(N2),   *scale_out = (float)(clipnorm / max(sqrt(N2), clipnorm))
 * (TensorFlow's clip_by_global_norm).  No floating-point atomics, a fixed order: the same inputs give the same bits.  Non-finite
 * gradients follow IEEE arithmetic.  workspace: embnet_optimizer_grad_norm_workspace_bytes(n_chunks) bytes, 16-byte aligned, its
 * first 16 bytes ZERO before the first launch (the arrival ticket, which re-arms itself); the partials behind it are fully
 * overwritten by every launch.  clipnorm > 0.  Reads 4 B per element (8 where a tensor has l2). */
#define EMBNET_OPT_MAX_GROUPS 8
enum { EMBNET_OPT_MOMENTUM = 5 };
int embnet_optimizer_step_groups(int rule, const void* table, int n_tensors, const int32_t* chunks, int n_chunks,
                                 const float* group_coef, int n_groups, float b1, float b2, float eps, float c2,
                                 float momentum, int nesterov, float clipvalue, const float* clip_scale_dev,
                                 const float* coef_dev, const float* group_coef_dev, void* stream);
size_t embnet_optimizer_grad_norm_workspace_bytes(int n_chunks);
int embnet_optimizer_grad_norm(const void* table, int n_tensors, const int32_t* chunks, int n_chunks, float clipnorm,
                               void* workspace, size_t workspace_bytes, double* norm_out, float* scale_out, void* stream);

/* ------------------------------------------------------------------ layer-wise adaptive updates (LARS / LAMB)
 * LARS (You et al. 2017, in the form of SimCLR's LARSOptimizer) and LAMB (You et al. 2020): every tensor's step is scaled by a
 * trust ratio r = eta |w| / |u|, u the tensor's update direction, so that a large batch's large rate moves every layer by the
 * same fraction of its own norm.  Two launches over the optimizer's table and chunk list above — the 48-byte descriptors
 * { w, g, slot1, slot2, n, l2x2, group } and the (tensor, chunk) pairs — with ONE more precondition: the chunks of a tensor are
 * consecutive and ascending in the list (as embeddingnet_amd/multi_tensor.py's chunk_list builds them: tensor by tensor).
 * The rules have codes of their own (embnet_optimizer_step_groups goes on refusing everything past EMBNET_OPT_MOMENTUM).
 *   group_coef      HOST float [n_groups][4] = { lr_g, 0, wd_g, eta_g }, 1 <= n_groups <= EMBNET_OPT_MAX_GROUPS: the group's rate,
 *                   its weight decay ITSELF (not lr * wd: the decay joins the direction, below) and its trust coefficient;
 *                   eta_g == 0 exempts the group from adaptation (r = 1: BatchNorm parameters and biases in the papers);
 *   group_coef_dev  NULL, or the same rows in DEVICE memory, read instead (a captured step replays with current rates);
 *   coef_dev        NULL, or device float[6] = lr, b1, b2, eps, c1, c2: b1, b2, eps, c1 and c2 are read from it (its lr is not);
 *   c1, c2          LAMB's bias corrections 1/(1-b1^t) and 1/(1-b2^t), computed by the host in double, passed in fp32 — best
 *                   from b1 and b2 as fp32 holds them, so that m*c1 and v*c2 are weighted means (1 - 0.999f is 1.3e-5 off 1e-3);
 *   clipvalue, clip_scale_dev   as embnet_optimizer_step_groups: exclusive; the scale is what embnet_optimizer_grad_norm left.
 * Both entry points launch one kernel, allocate nothing and never wait for the device: a stream capture records them.
 * Per element, fp32, contraction off, every rounding as written (fma = one rounding):
 *     g' = fma(l2x2, w, g);   clipvalue c > 0: g' = min(max(g', -c), c);   clip_scale_dev: g' = g' * s
 *     LARS   u = fma(wd_g, w, g')
 *     LAMB   m = fma(1-b1, g', b1*m);  v = fma((1-b2)*g', g', b2*v);  u = fma(wd_g, w, (m*c1) / (sqrtf(v*c2) + eps))
 * per tensor, in f64:  W2 = sum (double)w^2,  U2 = sum (double)u^2
 *     r = (eta_g > 0 && W2 > 0 && U2 > 0) ? (float)(eta_g * sqrt(W2) / sqrt(U2)) : 1        (f64 until the one conversion)
 *     LARS   s = lr_g * r;  su = s * u;  v = fma(momentum, v, su);  w = w - (nesterov ? fma(momentum, v, su) : v)     (slot1 = v)
 *     LAMB   s = lr_g * r;  w = fma(-s, u, w)                                                         (slot1 = m, slot2 = v)
 * A tensor with g == NULL (or without a slot its rule keeps) is skipped entirely: weight and slots untouched.
 *
 * embnet_optimizer_layerwise_norms: at most 512 workgroups walk the chunks; each chunk's W2 and U2 partial is the sum over its
 * elements — thread j of 256 adds elements 1024 i + 4 j .. 4 j + 3 (i = 0..3) of the chunk in ascending order, the 64 lanes of a
 * wave meet in a butterfly (offsets 32 .. 1), the four waves are added left to right — on the float4 path and element by element
 * alike.  For LAMB this pass writes m and v back.  The last workgroup to arrive then adds each tensor's partials p_0 .. p_{k-1}
 * (chunk order): lane j of one wave adds p_j, p_{j+64}, ... in ascending order onto 0, and the 64 sums meet in the same
 * butterfly.  That order depends on nothing but the tensor's size: not on the grid, not on the order of arrival.  No
 * floating-point atomics; the same inputs give the same bits.  It writes, with vector stores,
 *     stats_out[tensor] = { double W2; double U2; float r; float pad (0); }        24 bytes per tensor, 8-byte aligned
 * and { 0, 0, 1 } for a tensor that was skipped.  A tensor without elements has no chunk and gets no row.
 * workspace: embnet_optimizer_layerwise_workspace_bytes(n_chunks) bytes, 16-byte aligned, its first 16 bytes ZERO before the
 * first launch (the arrival ticket, which re-arms itself: no memset per step); the partials behind it are overwritten by every
 * launch.  Moves 8 bytes per element for LARS, 24 for LAMB.
 * embnet_optimizer_layerwise_step: one workgroup per chunk; reads r from `stats`.  LAMB recomputes u from the stored m, v and the
 * weight by the expression above — the norm is of the vector that is applied — and does not read the gradient.  Aligned whole
 * chunks go through float4, tails and unaligned tensors element by element, to the same bits.  momentum, nesterov: LARS only.
 * Moves 20 bytes per element for LARS, 16 for LAMB. */
enum { EMBNET_LAYERWISE_LARS = 0, EMBNET_LAYERWISE_LAMB = 1 };
size_t embnet_optimizer_layerwise_workspace_bytes(int n_chunks);
int embnet_optimizer_layerwise_norms(int rule, const void* table, int n_tensors, const int32_t* chunks, int n_chunks,
                                     const float* group_coef, int n_groups, float b1, float b2, float eps, float c1, float c2,
                                     float clipvalue, const float* clip_scale_dev, const float* coef_dev,
                                     const float* group_coef_dev, void* workspace, size_t workspace_bytes, void* stats_out,
                                     void* stream);
int embnet_optimizer_layerwise_step(int rule, const void* table, int n_tensors, const int32_t* chunks, int n_chunks,
                                    const float* group_coef, int n_groups, float b1, float b2, float eps, float c1, float c2,
                                    float momentum, int nesterov, float clipvalue, const float* clip_scale_dev,
                                    const float* coef_dev, const float* group_coef_dev, const void* stats, void* stream);

/* ------------------------------------------------------------------ averaged weights (EMA / SWA)
 * An averaged copy of every tensor of a model, kept by one launch per step beside the one-launch optimizer update, and a second
 * kernel that exchanges the model's tensors with their averages so that the averaged model is evaluated in place
 * (embeddingnet_amd/weight_average.py).  The exponential moving average and the stochastic weight average (the equal mean of
 * snapshots; Izmailov et al.) are the same per-element step with a host-computed coefficient c: EMA c = 1 - decay, SWA
 * c = 1 / (snapshots so far + 1).
 *   table   device array of n_tensors descriptors, 32 bytes each: { float* w; float* avg; int64 n; int64 reserved; } (reserved 0)
 *   chunks  device int32 [n_chunks][2] = (tensor index, chunk index within it), chunk = embnet_optimizer_chunk_elems()
 *           consecutive elements — the optimizer's list format; every element of every tensor covered exactly once.  A workgroup
 *           whose pair points outside the table or past the tensor's end does nothing.
 * embnet_weight_average_update: c is the argument, or *c_dev when c_dev is not NULL (device float: a captured HIP graph of the
 * training step replays with the step's current coefficient).  Per element, in fp32:
 *     !(c > 0)   nothing is read or written — the whole launch exits at once; a NaN read from c_dev counts as this case
 *     c >= 1     avg = w, a copy of the bits (a + 1 (w - a) is not w in fp32)
 *     otherwise  d = w - avg;  p = c * d;  avg = avg + p         — three roundings, never an fma
 * Aligned whole chunks go through float4, tails and tensors that are not 16-byte aligned element by element; both paths give the
 * same bits.  Moves 12 bytes per element.  With c_dev == NULL, c must lie in [0, 1].
 * embnet_weight_average_swap: w[i] <-> avg[i] as 32-bit words (NaN payloads survive), the same two paths, 16 bytes per element.
 * Two swaps are the identity.  Neither kernel uses atomics or a workspace. */
int embnet_weight_average_update(const void* table, int n_tensors, const int32_t* chunks, int n_chunks, float c,
                                 const float* c_dev, void* stream);
int embnet_weight_average_swap(const void* table, int n_tensors, const int32_t* chunks, int n_chunks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EMBNET_H */
