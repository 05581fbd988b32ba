/*
 * mcq.h -- C ABI of libmcq_hip.so: the MI355X (gfx950) index search and decode
 * of the multi-codebook quantizer.
 *
 * The reference (danpovey/quantization) has no FFI for this path: it is a Python
 * class whose private methods call torch ops.  Each entry point below replaces
 * the named reference method; the host-side mirror (quantization_amd/quantizer.py)
 * binds them with ctypes -- INTEGRATION.md shows the binding a maintainer of the
 * reference would add.
 *
 * Conventions
 *  - every pointer except `prepared`/`workspace` sizes is a BORROWED DEVICE pointer
 *    (torch `tensor.data_ptr()`), contiguous, alive until the stream has drained;
 *  - every function only enqueues work on `stream` (a hipStream_t passed as void*;
 *    NULL = the default stream) and returns immediately: no allocation, no
 *    synchronisation, re-entrant per (device, stream).  Process-wide state is limited to
 *    read-only tuning hooks (environment variables latched on first use; DESIGN.md lists
 *    them; none changes a result), a thread-local launch counter
 *    (mcq_last_encode_launches) and, per device, one side stream with two events: an encode of a
 *    large batch may run its chunks on two LANES, the caller's stream and that side stream.  It forks
 *    behind everything `stream` holds at the call and joins before it returns, so `stream` alone
 *    orders inputs, workspace and results as if every launch were on it; concurrent callers on one
 *    device are serialised over that section.  A capturing stream, or a device where the side stream
 *    cannot be made, gets the one-stream sequence (include/mcq_lanes.h);
 *  - return value: 0 = ok; MCQ_E* < 0 = rejected argument; > 0 = hipError_t of a
 *    failed launch.  Nothing is thrown across the boundary.
 *  - supported domain: codebook_size K a power of two in [16, 1024], num_codebooks N
 *    a power of two, N <= 64, N*K <= 16384 (the reference's trainer produces at most 64 x 16 and 32 x 256:
 *    bytes_per_frame <= 32, quantization/quantization.py:614; `prepared` holds the N*K x N*K Gram matrix).
 *    K = 512 / 1024 (Quantizer(codebook_size=...) with as_bytes=False, :35): the index search, mcq_refine_indexes,
 *    mcq_logits and mcq_decode (int64 codes); every uint8 output must be NULL there (MCQ_EINVAL otherwise), and the
 *    trainer's entry points (mcq_logits_argmax, mcq_logits_refine, mcq_logits_refine_codes, mcq_loss_*, mcq_recon_fwd,
 *    mcq_decode_backward_u8(_ex), ...) answer MCQ_EUNSUPPORTED.  Any
 *    dim 1 <= D <= 16384 (rows are zero-padded to a multiple of 16 inside `prepared`; the i32 accumulators
 *    of the fixed-point products bound D).  The reference crashes for K < 16
 *    (quantization/quantization.py:506) and needs K <= 256 for byte output (:271).
 *
 * Numerics: bit-identical to oracle/mcq_oracle.c (see its header for the spec).  The
 * three inner-product tables of the path -- the logits, x.C and the Gram matrix of the
 * centers -- are EXACT fixed-point products ("fixdot": rows as 30-bit fixed point against
 * their own largest magnitude, ten 8-bit limb products on the i8 matrix cores, one defined
 * fp32 combination): nothing in them depends on a summation order.  Sums of squares are
 * wave64 butterfly reductions; the refinement passes read their inner products from the
 * Gram matrix kept in `prepared` and from one x.C product per call (the TABLE FORM).
 * Non-finite inputs are outside the contract (the reference returns arbitrary codes for them).
 */
#ifndef MCQ_H
#define MCQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCQ_EINVAL (-1)     /* bad shape / null pointer                         */
#define MCQ_EUNSUPPORTED (-2) /* outside the supported (K, N) domain             */
#define MCQ_EWORKSPACE (-3) /* workspace smaller than mcq_encode_workspace_bytes */

#define MCQ_ABI_VERSION 7   /* 7: no signature changed.  The shortlists of a refinement pass are SETS listed in ascending position (they were
                               listed by (value, position) until 6: oracle/mcq_oracle.c::select_smallest) -- results differ from ABI 6 only
                               where two later scores tie exactly; mcq_test_select hands the list over in that order and takes the layout
                               in the sign of per_lane; 16 codebooks of 16 entries run all passes of a call in one launch (k_tf_pass16);
                               6: the products of the path are formed from CENTERED rows and frames (`prepared` also holds the codebooks' own
                               means and the classifier rows' products with the data mean, Q and the Gram matrix are those of
                               C[n][k] - mu_n, the frame planes of the workspace those of x - mean: sizes changed, signatures did
                               not), mcq_profile_encode times the shipped launch sequence and
                               reports per-category launch counts, mcq_profile_category_name is new;
                               5: mcq_prepared_decode_bytes, 64 codebooks for every codebook size, and (additions) mcq_prepare_params,
                               mcq_logits_refine_codes, mcq_loss_head_tail; 4: fixed-point products: `prepared` holds limb planes of the centers and the classifier
                               (mcq_prepared_bytes changed), workspaces hold those of the frames (the workspace sizes
                               depend on D), mcq_logits takes a workspace, mcq_logits_workspace_bytes is new */
int mcq_abi_version(void);

/* D rounded up to the padded row length used inside `prepared` and workspaces. */
int mcq_padded_dim(int D);

/* ---- derived state -------------------------------------------------------
 * Replaces Quantizer.get_centers() (quantization/quantization.py:77-79, recomputed
 * on every call there) and the parameter reads of Quantizer._logits (:277-279).
 * `prepared` receives: scaled centers C[N][K][Dp] = cscale_exp * centers (what decode sums), the codebooks' own means
 * mu_n = mean_k C[n][k] and their sum (= get_data_mean(), :67-75), and -- when weight is given -- what the search reads:
 * the CENTERED rows C[n][k] - mu_n as 8-bit limb planes with their row exponents, their sums of squares Q[N][K] (:411),
 * the rows of to_logits.weight as limb planes and their products with the data mean (the frames of both products are centered: a
 * logit is ((fixdot(x - mean, W_r) + fixdot(mean, W_r)) * lscale) + bias_r), the bias, and the Gram matrix G[N*K][N*K] of the
 * centered rows (16 MB at 8 x 256; what the refinement passes read).  The search is invariant under this shift
 * (oracle/mcq_oracle.c, "CENTERING").
 * cscale_exp / lscale_exp = exp(10*centers_scale) / exp(10*logits_scale), formed
 * by the caller in fp32 exactly as the reference does (:78, :278).
 * weight/bias may be NULL when only decode is needed: `prepared` then receives the scaled centers
 * only and needs mcq_prepared_decode_bytes (no limb planes, no Gram matrix: 16 MB .. 1 GB less);
 * such a state serves mcq_decode and nothing else.                                              */
size_t mcq_prepared_bytes(int N, int K, int D);
size_t mcq_prepared_decode_bytes(int N, int K, int D);
/* byte offset inside `prepared` of float[mcq_padded_dim(D)]: get_data_mean() (:67-75) of the scaled centers,
 * sum_n mean_k C[n][k][:] (the scaled centers themselves are at offset 0, [N][K][mcq_padded_dim(D)])            */
size_t mcq_prepared_mean_offset(int N, int K, int D);
int mcq_prepare(const float *centers, float cscale_exp, const float *weight, const float *bias,
                int N, int K, int D, void *prepared, void *stream);

/* As mcq_prepare with the two scale factors read from DEVICE memory: scales_exp = float[2]
 * {exp(10*centers_scale), exp(10*logits_scale)}.  No host copy of the (trained) scale parameters is
 * needed, so a training loop never synchronises; the logits factor is kept inside `prepared` and
 * used by mcq_encode_ex when MCQ_ENCODE_LSCALE_FROM_PREPARED is set.                            */
int mcq_prepare_dev(const float *centers, const float *scales_exp, const float *weight, const float *bias,
                    int N, int K, int D, void *prepared, void *stream);

/* As mcq_prepare_dev with the scale PARAMETERS read from device memory: centers_scale / logits_scale are the two scalar
 * parameters themselves, speed = 10 (Quantizer.scale_speed); exp(speed * scale) is formed on the device (the expf of
 * mcq_scales_exp) in the first kernel of the chain.  scales_exp_out (may be NULL) receives float[2]
 * {exp(speed*centers_scale), exp(speed*logits_scale)}: what the backward kernels take as `sa` / `scale_dev`.      */
int mcq_prepare_params(const float *centers, const float *centers_scale, const float *logits_scale, float speed,
                       const float *weight, const float *bias, int N, int K, int D, void *prepared,
                       float *scales_exp_out, void *stream);

/* ---- index search ----------------------------------------------------------
 * Replaces Quantizer._compute_indexes (:281-305): learned-logit argmax followed
 * by `refine_iters` passes of Quantizer._refine_indexes (:308-547).
 * x: fp32 [B][D].  Exactly one of out_u8 / out_i64 is non-NULL:
 *   out_i64: int64 [B][N]            -- _compute_indexes / encode(as_bytes=False)
 *   out_u8 : uint8 [B][N / pack]     -- encode(as_bytes=True) (:266-272), where
 *            pack = 2 when K == 16 (low nibble = even codebook), else 1.
 * workspace: device scratch of at least mcq_encode_workspace_bytes(B, N, K, D)
 * bytes (the batch is processed in chunks that fit; any B >= 0 is accepted).   */
size_t mcq_encode_workspace_bytes(long B, int N, int K, int D);
int mcq_encode(const float *x, long B, const void *prepared, float lscale_exp, int N, int K, int D,
               int refine_iters, uint8_t *out_u8, int64_t *out_i64, void *workspace,
               size_t workspace_bytes, void *stream);

/* mcq_encode with options.  Fixed-point skipping is ON by default (mcq_encode, mcq_encode_ex,
 * mcq_refine_indexes): _refine_indexes is a deterministic map of (x, indexes), so a vector whose
 * indexes a pass leaves unchanged is already final; such vectors leave the active list, their codes
 * go straight to the caller's output, and later passes only process the rest.  The codes are
 * identical to those of running every pass, for every input; the cost becomes data dependent
 * (lower on trained states, where most vectors converge after two or three passes).
 * MCQ_ENCODE_ALL_PASSES: run every pass on every vector (the cost of a batch where nothing
 * converges; what mcq_profile_encode and the trainer entry mcq_logits_refine_codes time).
 * MCQ_ENCODE_SKIP_FIXED_POINTS: accepted, no effect (the default it once opted into).            */
#define MCQ_ENCODE_SKIP_FIXED_POINTS 1u
#define MCQ_ENCODE_ALL_PASSES 8u
#define MCQ_ENCODE_LSCALE_FROM_PREPARED 2u /* lscale_exp argument ignored: see mcq_prepare_dev */
/* x points to IEEE fp16 [B][D] (the reference's data helper yields fp16 frames that callers widen,
 * quantization/quantization.py:798): rows widen to fp32 in the kernels' load path.  Every fp16 value
 * is an fp32 value, so the codes equal those of the widened input bit for bit.                   */
#define MCQ_ENCODE_X_FP16 4u
/* The initial codes are the arg max of the classifier logits.  When a call wants codes only, six of the ten limb
 * products of each logit pick the winner wherever their error bound separates it from the runner-up, and the remaining
 * (frame, codebook) pairs are recomputed exactly: same codes, less work.  MCQ_ENCODE_EXACT_LOGITS forces the ten-product
 * kernel for every pair (the A/B switch of that path; the environment hook MCQ_EXACT_LOGITS=1 does the same per process). */
#define MCQ_ENCODE_EXACT_LOGITS 16u
int mcq_encode_ex(const float *x, long B, const void *prepared, float lscale_exp, int N, int K, int D,
                  int refine_iters, uint8_t *out_u8, int64_t *out_i64, void *workspace,
                  size_t workspace_bytes, void *stream, unsigned flags);

/* Replaces Quantizer._refine_indexes (:308-547) applied `refine_iters` times to caller-supplied
 * indexes: idx_in int64 [B][N] with entries in [0, K) -> idx_out int64 [B][N] (may alias idx_in).
 * Same workspace as mcq_encode.                                                               */
int mcq_refine_indexes(const float *x, long B, const void *prepared, int N, int K, int D, int refine_iters,
                       const int64_t *idx_in, int64_t *idx_out, void *workspace, size_t workspace_bytes,
                       void *stream);

/* ---- decode ----------------------------------------------------------------
 * Replaces Quantizer.decode + _maybe_separate_indexes (:117-148, :551-573).
 * codes: [B][codes_per_row] of uint8 (code_bytes == 1) or int64 (code_bytes == 8);
 * codes_per_row == N, or N / r with r in {2,4,8,16} for packed codes (each code
 * holds r base-K digits, least significant first).  out: fp32 [B][D],
 * out[b] = sum over n ascending of C[n][index(b, n)].                          */
int mcq_decode(const void *codes, int code_bytes, int codes_per_row, long B, const void *prepared,
               int N, int K, int D, float *out, void *stream);

/* Gradient of decode w.r.t. the scaled centers (what autograd derives from the gather + sum of
 * :142-147): gC[n][k][:] = sum over the vectors b with index(b, n) == k, b ascending, of
 * grad_out[b][:].  Deterministic (fixed summation order, no atomics).  idx: int64 [B][N];
 * grad_out: fp32 [B][D]; gC: fp32 [N][K][D], fully overwritten.                                */
int mcq_decode_backward(const float *grad_out, const int64_t *idx, long B, int N, int K, int D, float *gC,
                        void *stream);

/* ---- trainer pieces ------------------------------------------------------------
 * What QuantizerTrainer.step (:641-719) runs besides the index search: the loss of
 * Quantizer.compute_loss (:211-242) as batch SUMS (the caller forms the means and ratios, and in
 * data-parallel training all-reduces the sums first) and its gradient.  Every reduction has a
 * fixed order: results are bit-reproducible.
 *
 * mcq_logits_argmax: logits fp32 [B][N*K] of Quantizer._logits (:277-279) AND their per-codebook
 * first-maximum argmax int64 [B][N] (:301) from one GEMM; the indexes then go through
 * mcq_refine_indexes.  workspace >= mcq_logits_workspace_bytes(B, N, D).  flags: MCQ_ENCODE_LSCALE_FROM_PREPARED, MCQ_ENCODE_X_FP16. */
int mcq_logits_argmax(const float *x, long B, const void *prepared, float lscale_exp, int N, int K, int D,
                      float *logits_out, int64_t *argmax_out, void *workspace, size_t workspace_bytes,
                      void *stream, unsigned flags);

/* mcq_logits_argmax followed by mcq_refine_indexes in one call (what compute_loss needs, :211-219): logits_out as above,
 * idx_out int64 [B][N] = the indexes after `refine_iters` passes.  workspace as for mcq_encode.             */
int mcq_logits_refine(const float *x, long B, const void *prepared, float lscale_exp, int N, int K, int D,
                      int refine_iters, float *logits_out, int64_t *idx_out, void *workspace, size_t workspace_bytes,
                      void *stream, unsigned flags);
/* the same, and the indexes a second time as unpacked bytes codes_out uint8 [B][N] (may be NULL): what
 * mcq_decode_backward_u8(_ex) scans -- the trainer's step needs both and would otherwise convert one into the other */
int mcq_logits_refine_codes(const float *x, long B, const void *prepared, float lscale_exp, int N, int K, int D,
                            int refine_iters, float *logits_out, int64_t *idx_out, uint8_t *codes_out, void *workspace,
                            size_t workspace_bytes, void *stream, unsigned flags);

/* Log-softmax statistics of logits [B][N*K] against indexes int64 [B][N] (:221-240):
 *   lse[b][n] = logsumexp_k;  chosen_sum[n] = sum_b (logit[b][n][idx] - lse);
 *   prob_sum[n][k] = sum_b softmax;  count[n][k] = #{b: idx[b][n] == k}.                       */
size_t mcq_loss_workspace_bytes(long B, int N, int K);
int mcq_loss_fwd(const float *logits, const int64_t *idx, long B, int N, int K, float *lse, float *chosen_sum,
                 float *prob_sum, float *count, void *workspace, size_t workspace_bytes, void *stream);

/* Gradient w.r.t. the logits of  g_chosen * sum_n chosen_sum[n] + sum_{n,k} g_prob[n][k] * prob_sum[n][k];
 * g_chosen (float[1]) and g_prob (float[N][K]) are DEVICE pointers (no host copy of upstream gradients). */
int mcq_loss_bwd(const float *logits, const int64_t *idx, const float *lse, long B, int N, int K,
                 const float *g_chosen, const float *g_prob, float *grad_logits, void *stream);

/* The (N, K)-sized tail of compute_loss (:217-241) and of the trainer's total loss
 * rel + logprob + entropy_scale * logits_entropy (:682-683), on DEVICE floats:
 *   sums = {sum err^2, sum (x-mean)^2, sum_n chosen_sum[n], total batch size}  (all-reduced in DP training)
 *   losses[4] = rel_reconstruction, logprob, logits_entropy, index_entropy losses;
 *   g[2] = d total / d sums[0], d total / d sums[2];  g_prob[N][K] = d total / d prob_sum
 * (g[1] and g_prob feed mcq_loss_bwd; 2 * g[0] scales mcq_decode_backward(err)).
 * N is at most 64 here and in mcq_loss_head_tail (the per-codebook entropies live in shared memory): MCQ_EUNSUPPORTED
 * past that, before any pointer is looked at.                                                      */
int mcq_loss_tail(const float *sums, const float *prob_sum, const float *count, int N, int K, float entropy_scale,
                  float *losses, float *g, float *g_prob, void *stream);

/* Reconstruction pieces (:213-217): err[b] = decode(idx[b]) - x[b] (fp32 [B][D]); partial sums over
 * groups of 4 vectors of err^2 (num_part) and (x - mean)^2 (den_part), float[(B + 3) / 4] each, to be
 * summed by the caller; mean = get_data_mean() (:67-75), float[D].  d(sum err^2)/d(centers) is
 * 2 * mcq_decode_backward(err).                                                                   */
int mcq_recon_fwd(const float *x, const int64_t *idx, long B, const void *prepared, const float *mean, int N,
                  int K, int D, float *err, float *num_part, float *den_part, void *stream);


/* ---- parameter update of QuantizerTrainer.step (:708-715, :722-730) ------------------------
 * mcq_weight_grad: the autograd of Quantizer._logits (:277-279) w.r.t. to_logits: with G = dL/dlogits fp32 [B][M]
 *   (M = N*K, from mcq_loss_bwd) and the frames x fp32 [B][D]:  gW[M][D] = s * G^T x,  gb[M] = column sums of G,
 *   s = exp(10*logits_scale) read from DEVICE memory (scale_dev).  Splits of the batch whose partial tiles (workspace) are
 *   added in a fixed order; fp32 MFMA, or -- M and D multiples of 128, M >= 1024, B >= 2048 -- six bf16 piece products per
 *   multiply-add (each operand as three bf16 pieces: fp32-grade, 1e-6 of the largest entry against the fp64 product).
 *   Deterministic; not part of the bit-exact contract of the index search.
 * mcq_adam_step: torch.optim.Adam's update (weight decay as L2 term, no amsgrad) on one flat bucket of n floats:
 *   parameters p, gradients g, moments m / v; bias_correction1 = 1 - beta1^t and sqrt(1 - beta2^t) formed by the caller.
 * mcq_loss_head: head[4] = {sum num_part, sum den_part, sum chosen_n, batch}: mcq_loss_tail's `sums` from the
 *   partials of mcq_recon_fwd / mcq_loss_fwd without host or library reductions.
 * mcq_scales_exp: out2 = {exp(speed * centers_scale), exp(speed * logits_scale)} on the device (the `scales_exp`
 *   of mcq_prepare_dev).                                                                          */
size_t mcq_weight_grad_workspace_bytes(long B, int M, int D);   /* partial tiles of the batch splits */
int mcq_weight_grad(const float *G, const float *x, long B, int M, int D, const float *scale_dev, float *gW, float *gb,
                    void *workspace, size_t workspace_bytes, void *stream);
int mcq_adam_step(float *p, const float *g, float *m, float *v, long n, double lr, double beta1, double beta2, double eps,
                  double weight_decay, double bias_correction1, double bias_correction2_sqrt, void *stream);
int mcq_loss_head(const float *num_part, const float *den_part, long nparts, const float *chosen_n, int N, float batch,
                  float *head, void *stream);
int mcq_scales_exp(const float *centers_scale, const float *logits_scale, float speed, float *out2, void *stream);
/* mcq_loss_head followed by mcq_loss_tail in ONE launch (same results; for a single process, where no all-reduce of the
 * sums sits between the two) */
int mcq_loss_head_tail(const float *num_part, const float *den_part, long nparts, const float *chosen_n, int N, float batch,
                       float *head, const float *prob_sum, const float *count, int K, float entropy_scale, float *losses,
                       float *g, float *g_prob, void *stream);

/* The scalar gradients without library reductions.  mcq_decode_backward_u8_ex: mcq_decode_backward_u8 whose stored
 * rows are scaled by sa[0]*sb[0]*sc (device floats sa, sb; host float sc) and which also leaves, per wave, the share of
 * <unscaled sums, dotw> (dotw fp32 [N][K][D]) in dot_part[mcq_decode_backward_waves(N, K, D)].  mcq_loss_bwd_ex:
 * mcq_loss_bwd that also leaves sum grad * (logit - bias) per wave in dot_part[mcq_loss_bwd_waves(B, N, K)].
 * mcq_grad_tail reduces both partial arrays in a fixed order:
 *   out_c = (sum part_c) * sa[0]*sb[0]*sc * speed   (d/d centers_scale),   out_l = (sum part_l) * speed   (d/d logits_scale). */
long mcq_decode_backward_waves(int N, int K, int D);
int mcq_decode_backward_u8_ex(const float *grad_out, const uint8_t *codes, long B, int N, int K, int D, float *gC,
                              const float *sa, const float *sb, float sc, const float *dotw, float *dot_part, void *stream);
long mcq_loss_bwd_waves(long B, int N, int K);
int mcq_loss_bwd_ex(const float *logits, const int64_t *idx, const float *lse, long B, int N, int K, const float *g_chosen,
                    const float *g_prob, float *grad_logits, const float *bias, float *dot_part, void *stream);
int mcq_grad_tail(const float *part_c, long n_c, const float *sa, const float *sb, float sc, const float *part_l, long n_l,
                  float speed, float *out_c, float *out_l, void *stream);

/* ---- JointCodebookLoss pieces (quantization/prediction.py:9-82) ----------------------
 * The consumer of the codes: a predictor trained to predict codebook n from its input and the entries of
 * codebooks 0..n-1.  The GEMMs are library calls on the caller's side; these are the fused non-GEMM parts.
 *
 * mcq_jcl_prefix_fwd (:38-66): A[n][b][:] = relu(hp[b] + scale * sum_{m<n} emb[m*K + max(idx[b][m], 0)]),
 *   summed in codebook order (embedding * scale, cat, cumsum, relu); hp fp32 [B][H] (the output of linear1),
 *   emb fp32 [(N-1)*K][H], idx int64 [B][N], A fp32 [N][B][H].
 * mcq_jcl_prefix_bwd: from gA = dL/dA: g_hp [B][H] and gE [N-1][B][H], the gradient of the embedding row frame b
 *   chose for codebook n (to be scattered with mcq_scatter_rows).
 * mcq_scatter_rows: out[n][k][:] = sum over b ascending with idx[b*idx_stride + n] == k of
 *   grad[b*stride_b + n*stride_n + :D] -- mcq_decode_backward with per-(b, n) gradients; negative indexes
 *   (padding frames) match nothing.  The cross-entropy itself is mcq_loss_fwd / mcq_loss_bwd on [N*B][K] logits,
 *   whose negative targets contribute nothing (ignore_index, :78-81).                                   */
int mcq_jcl_prefix_fwd(const float *hp, const float *emb, const int64_t *idx, long B, int N, int K, int H,
                       float scale, float *A, void *stream);
int mcq_jcl_prefix_bwd(const float *A, const float *gA, long B, int N, int H, float scale, float *g_hp, float *gE,
                       void *stream);
int mcq_scatter_rows(const float *grad, long stride_b, long stride_n, const int64_t *idx, int idx_stride, long B,
                     int N, int K, int D, float *out, void *stream);

/* mcq_decode_backward on unpacked uint8 codes [B][N] (K <= 256): same sums in the same order; the kernel is
 * bound by scanning the index column, which is 8x smaller this way (what the trainer's step uses).      */
int mcq_decode_backward_u8(const float *grad_out, const uint8_t *codes, long B, int N, int K, int D, float *gC,
                           void *stream);

/* ---- search over stored codes ----------------------------------------------------
 * (not in the reference) Which stored vectors are nearest to a query, answered from the codes without decoding them.
 * The quantizer is additive, x^_b = sum_n C[n][code[b][n]], so
 *     |q - x^_b|^2 = |q|^2 + sum_n T_q[n][code[b][n]] + t_b,    T_q[n][k] = -2 <q, C[n][k]>,    t_b = |x^_b|^2:
 * one table of N*K floats per query, one float per stored vector (formed once per store), N additions per (query, candidate).
 * One-byte codes only: K <= 256 (MCQ_EUNSUPPORTED past that, as at the trainer's entry points), 1 <= k <= 64 (k > 64:
 * MCQ_EUNSUPPORTED), B <= 2^31 - 1.  `prepared` of either flavour (the decode-only state is enough).
 * The contract (the tests restate rules 1, 2, 3, 4 and 6 in numpy and compare bit for bit):
 *   1. tables[q][n*K + k] = -2 * sum_d q[d] * C[n][k][d]: one fp32 chain over d ascending (each product rounded, then added);
 *      fp16 queries widen to fp32 first.
 *   2. norms[b] = sum_d (sum_n C[n][code[b][n]][d])^2 in fp32: rows added n ascending, then 64 per-lane chains and the xor
 *      butterfly; a code digit is masked with K - 1 as mcq_decode does.
 *   3. score[q][b] = (((T[c_0] + T[c_1]) + ...) + T[c_{N-1}]) + norms[b]: fp32 additions in exactly this order.
 *   4. per query the k candidates smallest under "(score, b) ascending" -- the lower position wins a tie --, listed in that
 *      order; fewer than k candidates: the tail is (+inf, -1).
 *   5. no floating-point atomics: the same inputs give the same bits.  A non-finite query or norm neither faults nor hangs; its
 *      row of results is unspecified.
 * Inner product and cosine come from the same tables (mcq_search_scan_metric; rules 1, 2, 4 and 5 hold as they stand):
 *     <q, x^_b> = -1/2 * S,    cos(q, x^_b) = <q, x^_b> / (|q| |x^_b|),    S = ((T[c_0] + T[c_1]) + ...) + T[c_{N-1}] as in rule 3.
 *   3'. score[q][b] per metric, with the per-candidate array w (float[B]):
 *         MCQ_SEARCH_L2    w = norms                  score = S + w[b]      smaller = nearer (rule 3; this IS mcq_search_scan)
 *         MCQ_SEARCH_IP    w is ignored, may be NULL  score = S             smaller = larger inner product; nothing is loaded
 *         MCQ_SEARCH_COS   w = rnorms                 score = S * w[b]      smaller = larger cosine (|q| is constant per query);
 *                                                                           one fp32 multiplication
 *       The caller turns a score into a similarity: -0.5 * score (IP), -0.5 * score / |q| (cosine).
 *   6. rnorms[b] = 1.0f / sqrtf(norms[b]), both operations correctly rounded in fp32, and 0 where norms[b] == 0 (an all-zero
 *      reconstruction scores 0 under the cosine, never NaN).  mcq_code_rnorms forms norms[b] exactly as rule 2 says and converts;
 *      mcq_rnorms_from_norms converts norms a store already keeps: the two agree bit for bit.
 * mcq_search_tables: q fp32 or (q_is_fp16 != 0) IEEE fp16 [Q][D] -> tables_out float[Q][N*K].
 * mcq_code_norms: codes uint8 [B][N], one per codebook (unpacked) -> norms_out float[B].
 * mcq_search_scan: tables float[Q][N*K], codes uint8 [B][N] aligned to min(N, 16) bytes (MCQ_EINVAL otherwise), norms float[B]
 *   -> out_score float[Q][k], out_index int64[Q][k].  workspace >= mcq_search_workspace_bytes(Q, B, N, K, k): partial lists
 *   only (k entries per query and slice of the store); it does not depend on D and stops growing with B once the slice count
 *   reaches its cap.  Q == 0 or B == 0 return 0 after filling the outputs as rule 4 says.  Everything is rejected before
 *   anything touches the device.                                                                                       */
int mcq_search_tables(const void *q, int q_is_fp16, long Q, const void *prepared, int N, int K, int D, float *tables_out,
                      void *stream);
int mcq_code_norms(const uint8_t *codes, long B, const void *prepared, int N, int K, int D, float *norms_out, void *stream);
size_t mcq_search_workspace_bytes(long Q, long B, int N, int K, int k);
int mcq_search_scan(const float *tables, long Q, const uint8_t *codes, const float *norms, long B, int N, int K, int k,
                    float *out_score, int64_t *out_index, void *workspace, size_t workspace_bytes, void *stream);

/* The scan under a metric (rules 3' and 6 above).  Arguments, limits, workspace (mcq_search_workspace_bytes serves every metric)
 * and the order of the lists are those of mcq_search_scan; an unknown metric is MCQ_EINVAL, and so is w == NULL with
 * MCQ_SEARCH_L2 or MCQ_SEARCH_COS when B > 0.  Fewer than k candidates: the tail is (+inf, -1) under every metric (scores
 * ascend; a caller that reports similarities shows it as (-inf, -1)).
 * mcq_code_rnorms: as mcq_code_norms, rnorms_out float[B].  mcq_rnorms_from_norms: norms float[B] -> rnorms_out float[B]
 * (B > 2^31 - 1: MCQ_EUNSUPPORTED; in place is fine).                                                                    */
#define MCQ_SEARCH_L2 0
#define MCQ_SEARCH_IP 1
#define MCQ_SEARCH_COS 2
int mcq_search_scan_metric(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K, int k,
                           int metric, float *out_score, int64_t *out_index, void *workspace, size_t workspace_bytes,
                           void *stream);
int mcq_code_rnorms(const uint8_t *codes, long B, const void *prepared, int N, int K, int D, float *rnorms_out, void *stream);
int mcq_rnorms_from_norms(const float *norms, long B, float *rnorms_out, void *stream);

/* ---- range search over stored codes -----------------------------------------------
 * Every stored vector within a threshold of a query, instead of the k best.  Same tables, same codes, same per-candidate
 * array w and the same score[q][b] as rule 3' defines it under the metric (L2 S + w[b], IP S, cosine S * w[b]); rules 1, 2,
 * 3, 3' and 6 hold as they stand, no k appears anywhere.  The contract continues (the tests restate rules 7 and 8 in numpy
 * and compare bit for bit):
 *   7. stored vector b is LISTED for query q iff score[q][b] <= thr[q]: one fp32 comparison, inclusive.  A NaN on either side
 *      lists nothing.  thr is float[Q], one threshold per query, in the score domain of the scan (smaller = nearer under all
 *      three metrics: an inner product >= s is thr = -2 s, a cosine >= c is thr = -2 c |q|, a squared distance <= r is
 *      thr = r - |q|^2).
 *   8. the output is CSR.  lims is int64[Q + 1], lims[0] = 0, lims[q+1] - lims[q] = the number of b listed for q.  The entries
 *      of query q occupy [lims[q], lims[q+1]) IN ASCENDING POSITION b, as (score fp32, position int64).  The output is a
 *      function of scores and thresholds alone: the same inputs give the same bits (rule 5; the only sums are of integers).
 *   9. Q == 0 or B == 0: lims is all zeros and nothing else is written (lims itself is always needed).  Every argument is
 *      rejected before anything touches the device, with the status codes and the domain of mcq_search_scan_metric: one-byte
 *      codes (K <= 256), N a power of two <= 64, B <= 2^31 - 1 (MCQ_EUNSUPPORTED past these), codes aligned to min(N, 16)
 *      bytes, w == NULL only with MCQ_SEARCH_IP, an unknown metric MCQ_EINVAL, a short workspace MCQ_EWORKSPACE.
 * The size of the result depends on the data, so the call is split where the caller allocates:
 *   count  -> lims (device memory, int64[Q + 1]), and per-(query, slice, wave) start offsets in the workspace;
 *   the caller reads lims[Q] (one synchronisation), allocates out_score float[total] and out_index int64[total];
 *   fill   with the SAME arguments, the same lims and the same, untouched workspace -> the entries.
 * fill stores no entry whose slot is outside [0, capacity): whatever lims and the workspace hold, nothing is written out of
 * bounds (a caller with less room than lims[Q] gets a truncated, otherwise correct CSR).  capacity == 0 writes nothing.
 * Both sweeps compute a score with one and the same routine, so they agree about every borderline candidate.
 * workspace >= what the size query below returns for (Q, B, N, K): 8 bytes per (query, slice of the store, wave); it does
 * not depend on D nor on the number of results, and stops growing with B once the slice count reaches its cap.            */
size_t mcq_search_range_workspace_bytes(long Q, long B, int N, int K);
int mcq_search_range_count(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K, int metric,
                           const float *thr, int64_t *lims, void *workspace, size_t workspace_bytes, void *stream);
int mcq_search_range_fill(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K, int metric,
                          const float *thr, const int64_t *lims, float *out_score, int64_t *out_index, long capacity,
                          void *workspace, size_t workspace_bytes, void *stream);

/* ---- search under a filter: a bitmask over the store -------------------------------
 * Deleted rows, rows of another tenant, rows that fail a predicate: the scan and the two sweeps take a mask and look at the
 * stored vectors whose bit is set, without a second copy of the store.  The contract continues (the tests restate rules 10
 * and 11 in numpy and compare bit for bit):
 *  10. a mask is uint64_t mask[(B + 63) / 64], 8-byte aligned (MCQ_EINVAL otherwise), in device memory.  Stored vector b is a
 *      CANDIDATE iff bit b & 63 of word b >> 6 is set; read as bytes that is numpy.packbits(keep, bitorder="little").  Bits at
 *      positions >= B of the last word are ignored, whatever they hold.  One mask serves all queries of a call.
 *  11. rules 3, 3', 4, 7 and 8 hold as they stand over the set of candidates.  The score of a candidate is the same bits as
 *      without a mask; the order is (score, b) ascending with b the ORIGINAL position, and original positions are reported;
 *      top-k with fewer than k candidates (none included) has the tail (+inf, -1); the range search lists b iff its bit is
 *      set and score[q][b] <= thr[q].  So the output equals, bit for bit, that of the unmasked call over the compacted store
 *      codes[keep], w[keep] with its positions mapped through nonzero(keep) (an increasing map: the order carries over).
 *  12. mask == NULL is the call without a mask.  A non-finite w or score behind a cleared bit changes no result, and a cleared
 *      bit never makes a load go out of bounds.
 * mcq_search_pack_mask: flags uint8 [B], one byte per stored vector, non-zero = keep -> mask_out, (B + 63) / 64 words, the
 *   bits past B zero.  B == 0 returns 0 and writes nothing; B > 2^31 - 1 is MCQ_EUNSUPPORTED.  A store may as well keep the
 *   words itself and flip bits (a delete clears one).
 * mcq_search_scan_masked, mcq_search_range_count_masked, mcq_search_range_fill_masked: the unmasked calls' arguments with
 *   `mask` after `metric`; their limits, status codes and the order of their checks (nothing touches the device before every
 *   argument passed); their workspaces, sized by the same two queries.  A call with Q == 0 or B == 0 looks at no input, the
 *   mask included.  fill takes the mask count took, like every other argument.  A step of 64 candidates whose mask word is
 *   zero costs no load of codes: a selective mask makes the call cheaper.                                                   */
int mcq_search_pack_mask(const uint8_t *flags, long B, uint64_t *mask_out, void *stream);
int mcq_search_scan_masked(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K, int k,
                           int metric, const uint64_t *mask, float *out_score, int64_t *out_index, void *workspace,
                           size_t workspace_bytes, void *stream);
int mcq_search_range_count_masked(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K,
                                  int metric, const uint64_t *mask, const float *thr, int64_t *lims, void *workspace,
                                  size_t workspace_bytes, void *stream);
int mcq_search_range_fill_masked(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K,
                                 int metric, const uint64_t *mask, const float *thr, const int64_t *lims, float *out_score,
                                 int64_t *out_index, long capacity, void *workspace, size_t workspace_bytes, void *stream);

/* ---- search list by list: an inverted file over the store ---------------------------
 * Every call above is a scan: each query meets each stored vector.  An inverted file keeps the store IN LIST ORDER by a coarse
 * partition, and a query is scored against the few lists it probes and no others.  The candidate sets differ per query,
 * which the one mask of rules 10-12 cannot say.  The contract continues (the tests restate rules 13-15 in numpy and compare
 * bit for bit):
 *  13. the store is in list order.  list_offsets is int64[L + 1] in device memory, non-decreasing, with
 *      0 <= list_offsets[0] and list_offsets[L] <= B.  List l is the positions [list_offsets[l], list_offsets[l + 1]); an empty
 *      list is legal, and positions outside every list belong to none.  probes is int32[Q][P] in device memory: an entry in
 *      [0, L) names a list, any other value names none (-1 is the documented padding).  The CANDIDATES of query q are the
 *      union of the lists its row names.  A row holds distinct list numbers; a repeated number leaves that query's row of
 *      results unspecified (it may list a position twice) and neither faults nor hangs.
 *  14. rules 3, 3' and 4 hold as they stand over a query's candidates.  The score of a candidate is the same bits as in
 *      mcq_search_scan_metric; the order is (score, b) ascending with b the position in the store, and positions in the
 *      store are reported; fewer than k candidates (none included): the tail is (+inf, -1).  So row q equals, bit for bit,
 *      row 0 of mcq_search_scan_masked called with that one query and a mask whose set bits are the union of its probed
 *      lists; and with every list probed and the lists covering [0, B) it equals row q of mcq_search_scan_metric, whatever
 *      the order of the probes in the row.
 *  15. mask != NULL (rule 10's words): b is a candidate iff it lies in a probed list AND its bit is set.  Lists do not start
 *      at multiples of 64, so every lane tests its own bit; that steps without a candidate are skipped is not promised here.
 *      mask == NULL reads no mask.
 *  16. limits and the order of the checks; everything is checked before anything touches the device.  First the limits of
 *      mcq_search_scan_masked with its status codes: one-byte codes (K <= 256), N a power of two <= 64, 1 <= k <= 64,
 *      B <= 2^31 - 1, an unknown metric.  Then P < 0 or L < 0: MCQ_EINVAL; P > 4096: MCQ_EUNSUPPORTED (a query's per-probe
 *      step counts and their prefix sums live in on-chip memory beside its tables).  Q == 0 returns 0 and looks at no input.
 *      B == 0, L == 0 or P == 0 return 0 after filling the outputs with (+inf, -1), and look at no other input.  Then the
 *      pointers: tables, codes, workspace, list_offsets, probes non-NULL, w == NULL only under MCQ_SEARCH_IP, codes aligned
 *      to min(N, 16) bytes, mask and list_offsets to 8, probes to 4 (MCQ_EINVAL); last a short workspace, MCQ_EWORKSPACE.
 *      The workspace holds partial lists only, k entries per (query, part of its candidates): its size is a function of
 *      (Q, P, N, K, k) and depends on neither B nor L, and not on D.  The call reads nothing back from the device and does
 *      not synchronise: the offsets are read by the kernel, never by the host.
 * Defence, not contract: the kernel clamps every list's range to [0, B] and treats begin >= end as empty, so offsets that
 * break rule 13 give wrong answers but can never make a load go out of bounds (as a cleared bit cannot under rule 12).      */
size_t mcq_search_lists_workspace_bytes(long Q, int P, int N, int K, int k);
int mcq_search_scan_lists(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K, int k,
                          int metric, const uint64_t *mask /* may be NULL */,
                          const int64_t *list_offsets, long L, const int32_t *probes, int P,
                          float *out_score, int64_t *out_index, void *workspace, size_t workspace_bytes, void *stream);

/* ---- range search list by list: every hit within a threshold in the probed lists -----
 * The range search of rules 7-9 over the candidates of rules 13 and 15: per query every stored vector of the lists its row
 * of probes names whose score does not exceed its threshold, as CSR.  Tables, codes, w, thr and the metric are those of
 * mcq_search_range_count_masked; mask (may be NULL), list_offsets, L, probes and P those of mcq_search_scan_lists.  The
 * contract continues (the tests restate rules 17 and 18 in numpy and compare bit for bit):
 *  17. listing.  b is LISTED for q iff it is a candidate of q under rules 13 and 15 (it lies in a list row q names and, under
 *      a mask, its bit is set) and score[q][b] <= thr[q] under rule 7: one fp32 comparison, inclusive, and a NaN on either
 *      side lists nothing.  The score of a candidate is the same bits as everywhere else (rules 3 and 3').
 *  18. layout and order.  The output is CSR as in rule 8: lims int64[Q + 1], lims[0] = 0, entries (score fp32, position
 *      int64) with positions those of the store.  The entries of query q come IN THE ORDER OF ITS PROBE ROW: the hits of the
 *      list slot 0 names first, then slot 1's, and within a list in ascending position.  When the named lists of a row
 *      ascend this is ascending position, and row q then equals, bit for bit, what mcq_search_range_count_masked and
 *      mcq_search_range_fill_masked give when called with that one query and a mask whose set bits are the union of its
 *      lists (under `mask`, the union intersected with it).  With every list named in ascending order and the lists covering
 *      [0, B) it equals row q of mcq_search_range_count / _fill (under `mask`, of the masked calls).  A list named twice is
 *      listed twice, its second block where the second naming stands: count and fill agree on this, and it neither faults
 *      nor hangs.  The same inputs give the same bits (the only sums are of integers; no atomics).
 *  19. empty calls and the order of the checks.  First the limits of rule 16 without k, with its status codes: one-byte
 *      codes (K <= 256), N a power of two <= 64, Q and B not negative, an unknown metric, B <= 2^31 - 1, then P < 0 or
 *      L < 0: MCQ_EINVAL; P > 4096: MCQ_EUNSUPPORTED.  lims is always needed (MCQ_EINVAL without it).  Q, B, L or P equal to
 *      0: lims is all zeros, nothing else is written and no other input is looked at (fill returns 0 and writes nothing).
 *      Otherwise the pointers of rule 16 (tables, codes, workspace, list_offsets, probes non-NULL, w == NULL only under
 *      MCQ_SEARCH_IP, codes aligned to min(N, 16) bytes, mask and list_offsets to 8, probes to 4), then thr non-NULL, all
 *      MCQ_EINVAL, and last a short workspace, MCQ_EWORKSPACE.  Nothing touches the device before every check has passed.
 *  20. fill takes the SAME arguments, the same lims and the same, untouched workspace, after the caller has read lims[Q]
 *      and allocated out_score float[total] and out_index int64[total].  It stores no entry whose slot is outside
 *      [0, capacity), whatever lims and the workspace hold (capacity < 0 is MCQ_EINVAL, capacity == 0 writes nothing; with
 *      room for an entry, out_score and out_index non-NULL).  The workspace is 8 bytes per (query, part of its candidates,
 *      wave): a function of (Q, P, N, K) that depends on neither B, L, D nor the number of results.  The host reads nothing
 *      back inside either call, and neither synchronises.
 * Defence, not contract: list ranges are clamped to [0, B] and begin >= end is empty, as in rule 16's footnote.              */
size_t mcq_search_range_lists_workspace_bytes(long Q, int P, int N, int K);
int mcq_search_range_lists_count(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K,
                                 int metric, const uint64_t *mask /* may be NULL */,
                                 const int64_t *list_offsets, long L, const int32_t *probes, int P,
                                 const float *thr, int64_t *lims, void *workspace, size_t workspace_bytes, void *stream);
int mcq_search_range_lists_fill(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K,
                                int metric, const uint64_t *mask /* may be NULL */,
                                const int64_t *list_offsets, long L, const int32_t *probes, int P,
                                const float *thr, const int64_t *lims, float *out_score, int64_t *out_index, long capacity,
                                void *workspace, size_t workspace_bytes, void *stream);

/* ---- residual codes list by list: include/mcq_residual.h -----------------------------
 * An inverted file whose lists keep the codes of x - centroid takes one more operand per (query, probe slot) and norms
 * formed over a base row.  Those entry points -- the list-by-list calls of rules 13-20 with a probe_bias argument, and the
 * code norms with a base row -- and rules 21-23 of the contract are declared in include/mcq_residual.h, which includes this
 * header.  Nothing declared here changes: MCQ_ABI_VERSION stays 7.                                                         */

/* ---- test / profiling hooks -------------------------------------------------
 * Logits of Quantizer._logits (:277-279) for a batch, fp32 [B][N*K]; used by the
 * parity tests to localise a divergence.                                       */
size_t mcq_logits_workspace_bytes(long B, int N, int D);   /* also what mcq_logits_argmax needs */
int mcq_logits(const float *x, long B, const void *prepared, float lscale_exp, int N, int K, int D,
               float *out, void *workspace, size_t workspace_bytes, void *stream);

/* Where every array of `prepared` starts (host only; what the tests of the fixed-point products read the blob by).
 * offsets_out[i], i < min(cap, 13), receive the byte offsets in this fixed order:
 *    0 C       fp32 [N][K][mcq_padded_dim(D)]   scaled centers          7 bias    fp32 [N*K]
 *    1 Q       fp32 [N*K]   |C[n][k] - mu_n|^2                          8 scales  fp32 [2]  (mcq_prepare_dev / _params)
 *    2 Cf      int8 limb planes of the centered rows                     9 mean    fp32 [mcq_padded_dim(D)]
 *    3 Ce      int32 [Rp]   their row exponents                         10 cmean   fp32 [N][mcq_padded_dim(D)]  mu_n
 *    4 Wf      int8 limb planes of to_logits.weight                     11 G       fp32 [N*K][N*K]
 *    5 We      int32 [Rp]   their row exponents                         12 total   = mcq_prepared_bytes(N, K, D)
 *    6 wmu     fp32 [N*K]   fixdot(W_r, mean)
 * Rp = N*K rounded up to 128 rows; a plane set holds Rp rows of D rounded up to 128 columns, byte ((c * 4 + l) * Rp + row) * 16 + k % 16
 * for column 16 c + k % 16 and limb l (most significant first).  Returns 13; a shape outside the domain MCQ_EUNSUPPORTED or
 * MCQ_EINVAL as mcq_prepare does; offsets_out == NULL or cap < 0 MCQ_EINVAL.                                          */
int mcq_test_prepared_layout(int N, int K, int D, size_t *offsets_out, int cap);

/* The x.C product of the index search on its own: out[b][r] = fixdot(x_b - mean, C_r - mu_n), fp32 [B][N*K], r = n*K + k.
 * Launches exactly what the encode does for a chunk (the frames less the data mean to limb planes, then the product against the
 * centered rows of `prepared`).  workspace >= mcq_logits_workspace_bytes(B, N, D); flags: MCQ_ENCODE_X_FP16 or 0 (anything
 * else MCQ_EINVAL); the argument checks are those of mcq_logits, in its order.                                         */
int mcq_test_xc(const float *x, long B, const void *prepared, int N, int K, int D, float *out, void *workspace,
                size_t workspace_bytes, void *stream, unsigned flags);

/* The wave-level selection of the search on its own: `cases` independent problems of 64 * per_lane scores each
 * (per_lane 1, 4 or 16: key i of lane l at position per_lane * l + i; -4 / -16: the slot-major layout, position 64 * i + l; -1004:
 * four keys per lane handled as positions in no particular order); out_v / out_p [cases][64] receive the cnt smallest by
 * (value, position) LISTED IN ASCENDING POSITION (a list that runs out of candidates is padded with (INF, M - 1)).
 * Test hook for the selection's paths (ties, clustered survivors).                                                       */
int mcq_test_select(const float *scores, int cases, int per_lane, int cnt, float *out_v, int *out_p, void *stream);

/* Name and launch count of the kernels enqueued by the last mcq_encode on this
 * thread (for bench.py's per-kernel HIP-event timing); returns the count.      */
int mcq_last_encode_launches(void);

/* Measurement tool (bench.py): runs the encode exactly as mcq_encode enqueues it -- the same launches, nothing switched off --
 * once per category of launch, with HIP events on `stream` round the launches of that category only (events round every launch of
 * one encode stretch it by a tenth); synchronises and allocates the output of those encodes.  A batch that mcq_encode runs on two
 * lanes is timed as the same chunks on the same workspace shares, one after the other on `stream`: the launches are the shipped
 * ones, their overlap across lanes is not part of what is timed.
 * ms_out[c] / launches_out[c] (c < cap) receive the summed milliseconds and the number of timed intervals of category c,
 * mcq_profile_category_name(c) its name (NULL past the last one).  Returns the number of categories, or an error code.   */
int mcq_profile_encode(const float *x, long B, const void *prepared, float lscale_exp, int N, int K,
                       int D, int refine_iters, void *workspace, size_t workspace_bytes, void *stream,
                       float *ms_out, int *launches_out, int cap);
const char *mcq_profile_category_name(int category);

#ifdef __cplusplus
}
#endif
#endif /* MCQ_H */
