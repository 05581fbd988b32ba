/* mcq_code16.h -- libmcq_hip.so: the search over stores of TWO-BYTE codes, for codebooks of 512 and 1,024 entries.
 *
 * A companion of include/mcq.h, include/mcq_residual.h, include/mcq_wide.h and include/mcq_rerank.h (which it includes): the
 * same library, the same conventions -- borrowed device pointers, calls that enqueue on the given stream and return, 0 /
 * MCQ_E* / hipError_t as the return value --, and the same ABI version.  Every search entry of those headers reads one-byte
 * codes and goes on answering MCQ_EUNSUPPORTED for K > 256; a digit of a 512- or 1,024-entry codebook takes 9 or 10 bits.
 * These entries read a store of uint16 digits and are otherwise the entries the other headers describe: rules 32-35 continue
 * the contract they number 1-31.  quantization_amd/_lib.py binds them in CODE16_SIGNATURES.
 *
 *  32. the store is uint16 [B][N], rows contiguous, and digit n of stored vector b is codes[b*N + n] & (K - 1).  The upper
 *      bits of an element are ignored, whatever they hold: a store whose elements carry other bits above the digit gives the
 *      bits of the results of the clean store, and no address outside a table is ever formed from an element.
 *  33. the domain: K a power of two in [16, 1024] -- the sizes below 512 are admitted on purpose, so that a store can be held
 *      against the one-byte entries bit for bit --, N a power of two in [1, 64], and N*K <= 16,384: the table of a query is
 *      N*K floats, and 64 KiB is what the kernels carry beside the probe ranges of a query.  N*K above that (32 x 1,024,
 *      64 x 512), K outside [16, 1024] or N > 64 is MCQ_EUNSUPPORTED, any other N or K MCQ_EINVAL, answered where the one-byte
 *      entries answer their domain.  1 <= k <= 1,024 for every top-k call (rule 24), and every other limit -- Q, B, P, D --
 *      is that of the one-byte entries.
 *  34. `codes` is aligned to min(2 N, 16) bytes in the searches (a candidate's digits are loaded as vectors of that size) and
 *      to 2 bytes in mcq_code_norms_u16; otherwise MCQ_EINVAL, checked where rule 5 checks the alignment of one-byte codes.
 *  35. everything else is, word for word, the rules of the one-byte entries, by the same device code with another element
 *      type: tables rule 1 (mcq_search_tables_u16 is mcq_search_tables behind the domain of rule 33); norms and reciprocal
 *      roots rules 2, 6 and 22 (mcq_code_norms_u16: rnorm != 0 gives r[b]; base and assign both NULL gives rule 2, both
 *      there rule 22, one of them MCQ_EINVAL); scores rules 3, 3' and 21; the top-k result rules 4, 24-26; the range
 *      result rules 7-9 and 17-20; masks rules 10-12; lists rules 13-16; the bias rules 21 and 23; the checks, their order,
 *      their status codes and the empty calls rules 5, 9, 16, 19, 23 and 24; the workspaces rules 19 and 27.
 *      mcq_search_topk_u16 takes the arguments of mcq_search_wide_lists, and mcq_search_range_u16_count / _fill those of
 *      mcq_search_range_lists_bias_count / _fill; mask, probes and probe_bias may each be NULL.  probes == NULL is the call
 *      over the WHOLE store, treated as one list [0, B) (rule 25): list_offsets, L, P and probe_bias are then not looked at,
 *      and a range call lists the hits of a query in ascending position (rule 8).  There is one top-k entry for every k: at
 *      k <= 64 its result has the bits the narrow one-byte entries give on the same digits (rule 26).  The workspace queries
 *      take P, the probes per query, 1 for a call over the whole store; they are functions of the call's shape alone and
 *      answer 256 outside the domain.   */
#ifndef MCQ_CODE16_H
#define MCQ_CODE16_H

#include "mcq_rerank.h"

#ifdef __cplusplus
extern "C" {
#endif

int mcq_search_tables_u16(const void *q, int q_is_fp16, long Q, const void *prepared, int N, int K, int D, float *tables_out,
                          void *stream);
int mcq_code_norms_u16(const uint16_t *codes, long B, const void *prepared, int N, int K, int D, int rnorm,
                       const float *base /* [L][D], may be NULL */, long L, const int32_t *assign /* [B], may be NULL */,
                       float *out, void *stream);
size_t mcq_search_topk_u16_workspace_bytes(long Q, int P, int N, int K, int k);
int mcq_search_topk_u16(const float *tables, long Q, const uint16_t *codes, const float *w, long B, int N, int K, int k, int metric,
                        const uint64_t *mask /* may be NULL */,
                        const int64_t *list_offsets, long L, const int32_t *probes /* NULL: the whole store */, int P,
                        const float *probe_bias /* [Q][P], may be NULL */,
                        float *out_score, int64_t *out_index, void *workspace, size_t workspace_bytes, void *stream);
size_t mcq_search_range_u16_workspace_bytes(long Q, int P, int N, int K);
int mcq_search_range_u16_count(const float *tables, long Q, const uint16_t *codes, const float *w, long B, int N, int K, int metric,
                               const uint64_t *mask /* may be NULL */,
                               const int64_t *list_offsets, long L, const int32_t *probes /* NULL: the whole store */, int P,
                               const float *probe_bias /* [Q][P], may be NULL */,
                               const float *thr, int64_t *lims, void *workspace, size_t workspace_bytes, void *stream);
int mcq_search_range_u16_fill(const float *tables, long Q, const uint16_t *codes, const float *w, long B, int N, int K, int metric,
                              const uint64_t *mask /* may be NULL */,
                              const int64_t *list_offsets, long L, const int32_t *probes /* NULL: the whole store */, int P,
                              const float *probe_bias /* [Q][P], may be NULL */,
                              const float *thr, const int64_t *lims, float *out_score, int64_t *out_index, long capacity,
                              void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MCQ_CODE16_H */
