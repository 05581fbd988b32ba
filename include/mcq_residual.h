/* mcq_residual.h -- libmcq_hip.so: the search list by list over RESIDUAL codes.
 *
 * A companion of include/mcq.h (which it includes): the same library, the same conventions -- borrowed device pointers, calls
 * that enqueue on the given stream and return, 0 / MCQ_E* / hipError_t as the return value --, and the same ABI version.  It
 * holds the entry points an inverted file over residual codes needs beside those of mcq.h's sections "search list by list"
 * and "range search list by list", and rules 21-23 of the contract that mcq.h numbers 1-20.
 * quantization_amd/_lib.py binds these entries in RESIDUAL_SIGNATURES, beside the SIGNATURES of mcq.h.                      */
#ifndef MCQ_RESIDUAL_H
#define MCQ_RESIDUAL_H

#include "mcq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- residual codes list by list: a bias per probe slot, norms over a base row -------
 * An inverted file over quantized vectors keeps, for vector b of list l, the code of its RESIDUAL x_b - c_l against the list's
 * coarse centroid: the bytes spend their precision inside the cell.  With x^_b = c_l + r^_b, r^_b the decode of the stored code,
 *     |q - x^_b|^2 = |q|^2 + S + bias + |c_l + r^_b|^2,    <q, x^_b> = -1/2 (S + bias),    bias = -2 <q, c_l>,
 * S the table sum of rule 3 over the residual's code.  Tables, codes, mask, lists and probes are those of rules 13-20 of
 * include/mcq.h, whose numbering of the contract continues here (the tests restate rules 21 and 22 in numpy and compare bit for bit):
 *  21. probe_bias is float[Q][P] in device memory, one value per (query, probe slot), formed by the caller (for residual codes
 *      -2 <q, c_{probes[q][p]}>; any finite values will do).  The score of candidate b of the list that slot p of row q names is
 *          score[q][b] = finish((S + probe_bias[q*P + p]), w[b]):   S as rule 3 leaves it, then exactly ONE more fp32 addition,
 *      then the metric's finishing operation of rule 3': L2 (S + bias) + w[b], IP S + bias, cosine (S + bias) * w[b].  Rules 4,
 *      13-15 and 17-18 hold as they stand over these scores.  The value of a slot that names no list (or an empty one) is
 *      never read.  A list named twice in a row takes, at each naming, the value of that naming's slot.
 *  22. the per-candidate array of a store of residual codes: norms[b] = sum_d (base[assign[b]][d] + sum_n C[n][code[b][n]][d])^2
 *      in fp32.  Per feature the codebook rows are added n ascending as in rule 2 (N - 1 additions), THEN the base element
 *      (one more); then the 64 per-lane chains and the xor butterfly of rule 2.  base is float[L][D] with row stride D (not
 *      the padded dim), 4-byte aligned; assign is int32[B]; assign[b] outside [0, L) adds no base row (the value is then
 *      rule 2's), and never makes a load go out of bounds.  rnorms follow by rule 6.
 *  23. mcq_search_scan_lists_bias, mcq_search_range_lists_bias_count and _fill take the arguments of mcq_search_scan_lists,
 *      mcq_search_range_lists_count and _fill with probe_bias after P.  probe_bias == NULL IS the call without one: the same
 *      kernels are launched and the same bits come back.  Limits, status codes, the order of the checks, empty calls and
 *      workspaces are those of rules 16, 19 and 20 (the two size queries of those entries serve: a bias takes no workspace);
 *      probe_bias is 4-byte aligned (MCQ_EINVAL, checked after the alignments of rule 16 and before thr and the size of the
 *      workspace) and is looked at by the kernel only.  count and fill take the same probe_bias, like every other argument.
 * mcq_code_norms_based / mcq_code_rnorms_based: the domain and the checks of mcq_code_norms (one-byte codes, B < 0
 *   MCQ_EINVAL, B > 2^31 - 1 MCQ_EUNSUPPORTED), then L < 0: MCQ_EINVAL; B == 0 returns 0 and looks at nothing; then codes,
 *   prepared, out, base and assign non-NULL, base and assign 4-byte aligned (MCQ_EINVAL).                                    */
int mcq_search_scan_lists_bias(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K, int k,
                               int metric, const uint64_t *mask /* may be NULL */,
                               const int64_t *list_offsets, long L, const int32_t *probes, int P,
                               const float *probe_bias /* [Q][P], may be NULL */,
                               float *out_score, int64_t *out_index, void *workspace, size_t workspace_bytes, void *stream);
int mcq_search_range_lists_bias_count(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K,
                                      int metric, const uint64_t *mask /* may be NULL */,
                                      const int64_t *list_offsets, long L, const int32_t *probes, int P,
                                      const float *probe_bias /* [Q][P], may be NULL */,
                                      const float *thr, int64_t *lims, void *workspace, size_t workspace_bytes, void *stream);
int mcq_search_range_lists_bias_fill(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K,
                                     int metric, const uint64_t *mask /* may be NULL */,
                                     const int64_t *list_offsets, long L, const int32_t *probes, int P,
                                     const float *probe_bias /* [Q][P], may be NULL */,
                                     const float *thr, const int64_t *lims, float *out_score, int64_t *out_index, long capacity,
                                     void *workspace, size_t workspace_bytes, void *stream);
int mcq_code_norms_based(const uint8_t *codes, long B, const void *prepared, int N, int K, int D, const float *base, long L,
                         const int32_t *assign /* int32[B] */, float *norms_out, void *stream);
int mcq_code_rnorms_based(const uint8_t *codes, long B, const void *prepared, int N, int K, int D, const float *base, long L,
                          const int32_t *assign /* int32[B] */, float *rnorms_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MCQ_RESIDUAL_H */
