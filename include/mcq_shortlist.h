/* mcq_shortlist.h -- libmcq_hip.so: the search over a SHORTLIST -- score the candidates a per-query shortlist names against
 * the stored codes (nothing is decoded, no raw vector is touched) and keep the k best.
 *
 * A companion of include/mcq.h, include/mcq_residual.h, include/mcq_wide.h, include/mcq_rerank.h and include/mcq_code16.h
 * (which it includes): the same library, the same conventions -- borrowed device pointers, calls that enqueue on the given
 * stream and return, 0 / MCQ_E* / hipError_t as the return value --, and the same ABI version.  The other searches scan a
 * whole store or the lists a query probes; mcq_rerank scores a shortlist against the RAW vectors.  These entries score a
 * shortlist against the CODES: the second stage of a two-stage quantisation (coarse codes find 300 to 1,000 candidates, a
 * finer quantizer's codes over the same vectors rescore them), the scorer behind a graph index or any other candidate
 * generator, and a per-query filter given as a list of ids.  Rules 36-39 continue the contract the other headers number
 * 1-35.  quantization_amd/_lib.py binds the entries in SHORTLIST_SIGNATURES.
 *
 *  36. domain and checks.  tables, codes and w are mcq_search_wide's: tables fp32 [Q][N][K] (rule 1), codes uint8 [B][N]
 *      (uint16 [B][N], rule 32, for mcq_search_shortlist_u16), w fp32 [B] by rule 3' -- t[b] under L2, r[b] under the cosine,
 *      NULL or ignored under IP.  The accepted (N, K) and the alignment of the codes are mcq_search_wide's for the one-byte
 *      entry (rule 5; K <= 256) and mcq_search_topk_u16's for the two-byte entry (rules 33 and 34; N*K <= 16,384).
 *      shortlist is int64 [Q][S]; row_of is NULL or int64 [Bs] (Bs is not looked at without it: B takes its place); they
 *      follow rule 28 verbatim: entry p of a shortlist row names a candidate iff 0 <= p < Bs and, with row_of,
 *      0 <= row_of[p] < B; the candidate is scored with row row_of[p] of codes and w (row p without row_of) and REPORTED as
 *      p.  Every other entry names none (-1 is the padding of the searches), and a position named twice is a candidate
 *      twice.  bias is NULL or fp32 [Q][S], one value per shortlist SLOT.
 *      1 <= k <= 1,024, a metric of rule 1, and Q, S, B, Bs in [0, 2^31 - 1).  In this order, before any pointer is looked
 *      at: an (N, K) outside the domain is MCQ_EUNSUPPORTED or MCQ_EINVAL as rules 5 and 33 say, and k > 1,024 is
 *      MCQ_EUNSUPPORTED; k < 1 or a negative Q, S, B, Bs is MCQ_EINVAL; an unknown metric is MCQ_EINVAL; Q, S, B or
 *      Bs >= 2^31 - 1 is MCQ_EUNSUPPORTED; missing outputs (Q > 0) are MCQ_EINVAL.  Q == 0 then does nothing and returns 0.
 *      A call whose rows cannot hold a candidate (S, B or Bs is 0) looks at no input and writes k entries of (+inf, -1) per
 *      query, as does every row without a candidate.  Otherwise a NULL tables, codes, shortlist or workspace, and a NULL w
 *      under L2 or the cosine, is MCQ_EINVAL; then the alignments: codes by rule 5 or 34, shortlist and row_of to 8, bias
 *      to 4; MCQ_EWORKSPACE is checked last.  Nothing touches the device before the checks have passed and nothing is ever
 *      read back to the host.  Whatever shortlist and row_of hold, no address outside codes[0 .. B*N), w[0 .. B),
 *      row_of[0 .. Bs), the shortlist, the bias and the tables is ever formed into a load: a lane without a candidate
 *      re-reads row 0 of the store, which exists, and offers nothing.
 *  37. the score is exactly rule 21's: score_finish((S_table + bias[q][j]), w[row], metric) for the entry in slot j of row
 *      q, S_table the chain of N table additions of rule 3 -- the same device code as every other search.  bias == NULL adds
 *      -0.0, and (S + -0.0) has the bits of S.  The bias of a slot whose entry names no candidate does not matter.  The score
 *      of a (query, row, bias) triple does not depend on Q, S, k, the slot, the number of parts or the launch: it has the
 *      bits mcq_search_wide reports for the same query and row (with a bias, mcq_search_wide_lists with that probe_bias).
 *  38. the result is rule 26's over these candidates, the function of (score, position) that rule 30 describes: the k
 *      smallest under "(score, position) ascending", listed in that order; -0.0 and +0.0 are equal scores, ordered by
 *      position, and keep their bits; a NaN score is never listed; +inf is listed behind every finite score; the tail of a
 *      row with fewer than k candidates is (+inf, -1); a position named twice is listed twice where both fit.  No
 *      floating-point atomics.  The result does not depend on the number of parts a row is cut into or on the order in which
 *      the candidates stand in the row (given equal biases).
 *  39. the workspace: mcq_search_shortlist_workspace_bytes(Q, S, N, K, k), a function of those five alone and the same for
 *      both entries; 256 outside the domain of rule 36 (that of the two-byte entry, which contains the other) or where Q or
 *      S is 0; a workspace smaller than that is MCQ_EWORKSPACE.  It holds k (score, position) pairs per query and part.   */
#ifndef MCQ_SHORTLIST_H
#define MCQ_SHORTLIST_H

#include "mcq_code16.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t mcq_search_shortlist_workspace_bytes(long Q, long S, int N, int K, int k);
int mcq_search_shortlist(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K,
                         int k, int metric, const int64_t *shortlist, long S,
                         const int64_t *row_of /* may be NULL */, long Bs, const float *bias /* [Q][S], may be NULL */,
                         float *out_score, int64_t *out_index, void *workspace, size_t workspace_bytes, void *stream);
int mcq_search_shortlist_u16(const float *tables, long Q, const uint16_t *codes, const float *w, long B, int N, int K,
                             int k, int metric, const int64_t *shortlist, long S,
                             const int64_t *row_of /* may be NULL */, long Bs, const float *bias /* [Q][S], may be NULL */,
                             float *out_score, int64_t *out_index, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MCQ_SHORTLIST_H */
