/* mcq_rerank.h -- libmcq_hip.so: the exact re-ranking of a shortlist -- gather the raw rows a shortlist names, score them
 * against the query in fp32 and keep the k best, in one pass over the rows.
 *
 * A companion of include/mcq.h, include/mcq_residual.h and include/mcq_wide.h (which it includes): the same library, the same
 * conventions -- borrowed device pointers, calls that enqueue on the given stream and return, 0 / MCQ_E* / hipError_t as the
 * return value --, and the same ABI version.  mcq_search_wide and mcq_search_wide_lists end in a shortlist of up to 1,024
 * positions per query; this entry is the step after them, and it needs no quantizer: queries, the raw store, the shortlist.
 * Rules 28-31 continue the contract the other headers number 1-27.  quantization_amd/_lib.py binds the entries in
 * RERANK_SIGNATURES.
 *
 *  28. domain and checks.  queries is [Q][D] and vectors [B][D], rows contiguous, each fp32 (its _half flag 0) or fp16 (any
 *      other value); shortlist is int64 [Q][S]; row_of is NULL or int64 [Bs] (Bs is not looked at without it: B takes its
 *      place).  Entry p of a shortlist row names a candidate iff 0 <= p < Bs and, with row_of, 0 <= row_of[p] < B; the
 *      candidate is scored against row row_of[p] of vectors (row p without row_of) and REPORTED as p.  Every other entry
 *      names none (-1 is the padding of the searches), and a position named twice is a candidate twice.
 *      1 <= D <= 16,384, 1 <= k <= 1,024, a metric of rule 1, and Q, S, B, Bs in [0, 2^31 - 1).  In this order, before any
 *      pointer is looked at: D > 16,384 or k > 1,024 is MCQ_EUNSUPPORTED; D < 1, k < 1 or a negative Q, S, B, Bs is
 *      MCQ_EINVAL; an unknown metric is MCQ_EINVAL; Q, S, B or Bs >= 2^31 - 1 is MCQ_EUNSUPPORTED; missing outputs (Q > 0)
 *      are MCQ_EINVAL.  Q == 0 then does nothing and returns 0.  A call whose rows cannot hold a candidate (S, B or Bs is 0)
 *      looks at no input and writes k entries of (+inf, -1) per query, as does every row without a candidate.  Otherwise a
 *      NULL queries, vectors, shortlist or workspace is MCQ_EINVAL; then the alignments: queries and vectors to their
 *      element (4 or 2 bytes), shortlist and row_of to 8; MCQ_EWORKSPACE is checked last.  Nothing touches the device
 *      before the checks have passed, nothing is ever read back to the host, and whatever the shortlist and row_of hold no
 *      address outside vectors[0 .. B*D), shortlist, row_of[0 .. Bs) and queries is ever formed into a load.
 *  29. the score.  Operands are widened to fp32 (exact); all arithmetic is fp32, one rounding per operation, no contraction.
 *      The score is a function of the query row, the vector row, D and the metric alone: not of Q, S, k, the slot in the
 *      shortlist, the pairing of dtypes beyond the widened values, the alignment of a pointer, or the launch.  The order of
 *      the additions: element e belongs to lane (e / 4) % 64 -- groups of four consecutive elements dealt round-robin to 64
 *      lanes, 256 elements a trip; a lane adds its terms in ascending e, one at a time, into one accumulator that starts at
 *      +0.0; the 64 lane sums are combined by the butterfly v[l] = v[l] + v[l ^ m] for m = 32, 16, 8, 4, 2, 1.  The terms:
 *      L2 fl(d * d) with d = fl(q_e - x_e); IP and COS fl(q_e * x_e), and COS a second sum, of fl(x_e * x_e), in the same
 *      order.  The scores, ascending like those of rule 3: L2 the sum; IP its negation; COS -fl(dot * r) with r = 0 for
 *      xx == 0 and fl(1 / fl(sqrt(xx))) otherwise (rnorm_of, the r[b] of rule 3').  They are |q - x|^2, -<q, x> and
 *      -|q| cos(q, x): the caller negates, and under COS divides by |q|.
 *  30. the result is rule 26's over these candidates: the k smallest under "(score, position) ascending" by the one
 *      comparison of rule 4, listed in that order.  -0.0 and +0.0 are equal scores, ordered by position, and keep their
 *      bits; a NaN score is never listed; +inf is listed behind every finite score; the tail of a row with fewer than k
 *      candidates is (+inf, -1).  No floating-point atomics.  The result is a function of the scores and positions alone,
 *      not of the number of parts a row is cut into or of the order in which candidates arrive (two entries that name one
 *      position have one score, so which of them is listed first cannot be told).
 *  31. the workspace: mcq_rerank_workspace_bytes(Q, S, D, k), a function of those four alone, 256 outside the domain of
 *      rule 28 or where Q or S is 0; a workspace smaller than that is MCQ_EWORKSPACE.  It holds k (score, position) pairs
 *      per query and part.   */
#ifndef MCQ_RERANK_H
#define MCQ_RERANK_H

#include "mcq_wide.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t mcq_rerank_workspace_bytes(long Q, long S, int D, int k);
int mcq_rerank(const void *queries, int queries_half, long Q, const void *vectors, int vectors_half, long B, int D,
               const int64_t *shortlist, long S, const int64_t *row_of /* may be NULL */, long Bs,
               int k, int metric, float *out_score, int64_t *out_index,
               void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MCQ_RERANK_H */
