/* mcq_coarse.h -- libmcq_hip.so: the coarse probes -- score every query against every coarse centroid on the fp32 matrix cores
 * and keep the P best per query, exactly; with them the per-probe bias a store of residual codes takes; and, at P = 1, the
 * assignment of a store to its cells.
 *
 * A companion of include/mcq.h and its other companions (it includes include/mcq_shortlist.h): the same library, the same
 * conventions -- borrowed device pointers, calls that enqueue on the given stream and return, 0 / MCQ_E* / hipError_t as the
 * return value --, and the same ABI version.  What it returns is what mcq_search_scan_lists and its kin take as probes and
 * probe_bias.  Rules 40-43 continue the contract the other headers number 1-39.  quantization_amd/_lib.py binds the entries
 * in COARSE_SIGNATURES.
 *
 *  40. domain and checks.  queries is [Q][D] and centroids [L][D], fp32, rows contiguous.  1 <= D <= 16,384, 1 <= P <= 128, a
 *      metric of rule 1, and Q, L in [0, 2^31 - 1).  In this order, before any pointer is looked at: D > 16,384 or P > 128 is
 *      MCQ_EUNSUPPORTED; D < 1, P < 1 or a negative Q or L is MCQ_EINVAL; an unknown metric is MCQ_EINVAL; Q or L >= 2^31 - 1
 *      is MCQ_EUNSUPPORTED; a missing out_list or out_score (Q > 0) is MCQ_EINVAL.  Q == 0 then does nothing and returns 0.
 *      L == 0 looks at no input and at no part buffer and writes P entries of the tail per query.  Otherwise: `parts` outside
 *      [1, ceil(L / 128)] is MCQ_EINVAL, and ceil(Q / 32) * parts >= 2^31 - 1 is MCQ_EUNSUPPORTED; a NULL queries, centroids,
 *      part_score or part_list, and a NULL terms unless the metric is IP, is MCQ_EINVAL; then the alignments, every pointer
 *      to 4 bytes.  Nothing touches the device before the checks have passed, nothing is ever read back to the host, inputs
 *      are never written, and a refused call writes nothing.
 *      `parts` is the CALLER'S choice: the centroid tiles of 128 rows are cut into that many parts by count, one workgroup
 *      per (32 queries, part).  Any value of the range is valid and the result does not depend on it.  mcq_coarse_parts(Q,
 *      L, D, P) recommends one: 1 where the query tiles alone fill the chip (256 of them), else enough for about two
 *      workgroups per compute unit, never more than there are centroid tiles, and 1 outside the domain.
 *      part_score is [Q][parts][P] fp32 and part_list [Q][parts][P] int32, exactly: after the call part s of query q holds the
 *      P best of its centroids, ascending under rule 42's order, the tail (+inf, -1).  They are written before they are read.
 *  41. the score.  dot(q, c) is an fp32 accumulation on v_mfma_f32_32x32x2_f32: step t multiplies elements 2 t and 2 t + 1 of
 *      the two rows and adds both products to the accumulator, t ascending from 0 to ceil(D / 32) * 16 - 1, the rows padded
 *      with +0.0, one accumulator that starts at +0.0; no split over D, and the same instruction sequence for every pair.
 *      The scores ascend like those of rule 3: L2 fl(h[l] - dot), IP -dot, COS -fl(dot * r[l]), with the terms
 *      mcq_coarse_terms computes once per centroid set: h[l] = fl(0.5 * |c_l|^2), r[l] = rnorm_of(|c_l|^2) as in rule 3' (0
 *      for a zero row), the sum of squares in rule 29's order (element e to lane (e / 4) % 64, ascending within a lane, the
 *      butterfly); under IP nothing is written and terms may be NULL.  The L2 score is 0.5 * (|q - c|^2 - |q|^2): what orders
 *      the centroids of one query.  The score of a (query row, centroid row) pair is a function of the two rows, D and the
 *      metric alone: not of Q, L, P, `parts`, the alignment of a pointer, or where in a tile or the grid the pair lands.
 *  42. the result is the P smallest under "(score, list) ascending" by the one comparison of rule 4, listed in that order:
 *      out_list [Q][P] int32 and out_score [Q][P].  -0.0 and +0.0 are equal scores, ordered by list; a NaN score is never
 *      listed; +inf is listed behind every finite score; the tail of a row with fewer than P listed centroids is (-1, +inf,
 *      bias 0).  The only atomics are integer counters in LDS.  The result is a function of the scores alone.
 *  43. the bias.  out_bias may be NULL; otherwise out_bias[q][p] = fl(-2 * dot') for the listed centroid, where dot' is
 *      recomputed for the P winners alone as a plain fp32 dot in rule 29's order (the inner-product terms of that rule).  It is
 *      a function of the two rows and D alone.  It is NOT the matrix-core dot of rule 41 and need not share its bits: it is
 *      the value rule 21 adds, held to rule 29's statement, and the order of the probes is rule 41's.
 */
#ifndef MCQ_COARSE_H
#define MCQ_COARSE_H

#include "mcq_shortlist.h"

#ifdef __cplusplus
extern "C" {
#endif

int mcq_coarse_terms(const float *centroids, long L, int D, int metric, float *terms /* [L]; may be NULL under IP */,
                     void *stream);
long mcq_coarse_parts(long Q, long L, int D, int P);
int mcq_coarse_probe(const float *queries, long Q, const float *centroids, long L, int D,
                     const float *terms /* may be NULL under IP */, int P, int metric, long parts,
                     int32_t *out_list, float *out_score, float *out_bias /* may be NULL */,
                     float *part_score, int32_t *part_list, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MCQ_COARSE_H */
