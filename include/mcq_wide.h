/* mcq_wide.h -- libmcq_hip.so: the top-k search past 64 neighbours, result lists of up to 1,024 entries per query.
 *
 * A companion of include/mcq.h and include/mcq_residual.h (which it includes): the same library, the same conventions --
 * borrowed device pointers, calls that enqueue on the given stream and return, 0 / MCQ_E* / hipError_t as the return value --,
 * and the same ABI version.  mcq_search_scan* of those headers stop at k = 64 (one list entry per lane of a wave) and go on
 * answering MCQ_EUNSUPPORTED beyond; a search over short codes is lossy, and its usual task is to hand a shortlist of 100 to
 * 1,000 candidates to an exact re-ranker.  These entries serve that, and rules 24-27 continue the contract the two headers
 * number 1-23.  quantization_amd/_lib.py binds them in WIDE_SIGNATURES.
 *
 *  24. mcq_search_wide takes the arguments of mcq_search_scan_masked (mask == NULL: the whole store, rule 12) and
 *      mcq_search_wide_lists those of mcq_search_scan_lists_bias (mask and probe_bias may each be NULL, rule 23), with
 *      1 <= k <= 1,024.  k > 1,024 is MCQ_EUNSUPPORTED, answered where those entries answer k > 64; every other check, its
 *      place in the order, its status code and the empty calls are those of rules 5, 12, 16 and 23.  Every (N, K, P) that
 *      mcq_search_scan_lists accepts is accepted for every such k.  Nothing touches the device before the checks have passed,
 *      and nothing is ever read back to the host.
 *  25. a score is exactly rule 3's (rule 21's with a bias): the same additions in the same order, the same finishing operation,
 *      by the same device code.  The candidates are those of rules 10-15; a call over the whole store treats it as ONE list
 *      [0, B).  A call without a bias adds -0.0 where rule 21 adds the bias: (S + -0.0) has the bits of S for every S.
 *  26. the result is rule 4's with the larger k: the k smallest under "(s, b) ascending", listed in that order, by the one
 *      comparison of rule 4.  -0.0 and +0.0 are equal scores, ordered by position; a reported score keeps its own bits; a NaN
 *      score is never listed; +inf is listed behind every finite score; with fewer than k candidates the tail is (+inf, -1),
 *      and that is the whole result of a call without a candidate.  There are no floating-point atomics and no integer keys:
 *      the order is strict and total over (score, position), so the result is a function of scores and positions alone --
 *      not of the launch, of the number of parts, or of the order in which candidates arrive.  At k <= 64 the result has
 *      the bits of the older entries' result.
 *  27. the workspace: mcq_search_wide_workspace_bytes(Q, B, N, K, k) and mcq_search_wide_lists_workspace_bytes(Q, P, N, K, k),
 *      functions of the call's shape alone, 256 outside the domain (as rules 5 and 16 have it, with k up to 1,024); a
 *      workspace smaller than that is MCQ_EWORKSPACE, checked last.  It holds k (score, position) pairs per query and part.   */
#ifndef MCQ_WIDE_H
#define MCQ_WIDE_H

#include "mcq_residual.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t mcq_search_wide_workspace_bytes(long Q, long B, int N, int K, int k);
int mcq_search_wide(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K, int k, int metric,
                    const uint64_t *mask /* may be NULL */,
                    float *out_score, int64_t *out_index, void *workspace, size_t workspace_bytes, void *stream);
size_t mcq_search_wide_lists_workspace_bytes(long Q, int P, int N, int K, int k);
int mcq_search_wide_lists(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K, int k,
                          int metric, const uint64_t *mask /* may be NULL */,
                          const int64_t *list_offsets, long L, const int32_t *probes, int P,
                          const float *probe_bias /* [Q][P], may be NULL */,
                          float *out_score, int64_t *out_index, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MCQ_WIDE_H */
