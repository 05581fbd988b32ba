/* mcq_coarse_half.h -- libmcq_hip.so: the coarse probes of include/mcq_coarse.h for fp16 queries -- score every fp16 query against
 * every coarse centroid on the f16 matrix cores, against the two fp16 planes of the fp32 centroids, and keep the P best per query,
 * exactly; with them the per-probe bias a store of residual codes takes.  No fp32 copy of the queries is made and nothing of
 * size (Q, L).
 *
 * A companion of include/mcq.h and its other companions (it includes include/mcq_half.h): the same library, the same
 * conventions, the same ABI version.  Rules 52-55 continue the contract the other headers number 1-51.
 * quantization_amd/_lib.py binds the entries in COARSE_HALF_SIGNATURES; quantization_amd/half.py has coarse_planes and
 * coarse_probe_half.  As in mcq_half.h: the checks come in the stated order before any pointer is looked at, nothing touches the
 * device before they have passed, nothing is ever read back to the host, inputs are never written, a refused call writes
 * nothing, and scratch buffers are typed arguments that are written before they are read.  Queries and planes are IEEE binary16
 * as uint16_t; centroids, terms, scores and biases are fp32.
 *
 *  52. domain and checks.  queries is [Q][D] fp16 and centroids [L][D] fp32, rows contiguous; terms is [L], what
 *      mcq_coarse_terms makes from the centroids under the metric (NULL is allowed under IP).  planes holds
 *      mcq_kmeans_half_planes(L, D) elements in rule 49's split: the hi rows [L][Dp], then the lo rows [L][Dp], Dp = 32 *
 *      ceil(D / 32), an element past D +0.0.  mcq_coarse_half_split(centroids, L, D, planes) writes exactly that, ONCE per
 *      centroid set: for the probe the planes are a const input.  Its checks: D > 16,384 is MCQ_EUNSUPPORTED; D < 1 or L < 0
 *      MCQ_EINVAL; L >= 2^31 - 1 MCQ_EUNSUPPORTED; L == 0 does nothing; a NULL pointer, centroids off 4 bytes or planes off 16
 *      MCQ_EINVAL.
 *      mcq_coarse_probe_half, in this order: D > 16,384 or P > 128 is MCQ_EUNSUPPORTED; D < 1, P < 1 or a negative Q or L is
 *      MCQ_EINVAL; an unknown metric (rule 1) is MCQ_EINVAL; Q or L >= 2^31 - 1 is MCQ_EUNSUPPORTED; a missing out_list or
 *      out_score (Q > 0) is MCQ_EINVAL.  Q == 0 then does nothing and returns 0.  L == 0 looks at no input and at no part
 *      buffer and writes P entries of the tail per query.  Otherwise: `parts` outside [1, ceil(L / 64)] is MCQ_EINVAL, and
 *      ceil(Q / 64) * parts >= 2^31 - 1 is MCQ_EUNSUPPORTED; a NULL queries, centroids, planes, part_score or part_list, and a
 *      NULL terms unless the metric is IP, is MCQ_EINVAL; then the alignments: queries to 2 bytes, planes to 16, every other
 *      pointer to 4.
 *      `parts` is the CALLER'S choice: the centroid tiles of 64 rows are cut into that many parts by count, one workgroup per
 *      (64 queries, part).  Any value of the range is valid and the result does not depend on it.  mcq_coarse_half_parts(Q,
 *      L, D, P) recommends one: 1 where the query tiles alone fill the chip (512 of them for P <= 16, where two workgroups share
 *      a compute unit, 256 beyond), else enough to reach that number, never more than there are centroid tiles, and 1 outside
 *      the domain.  part_score is [Q][parts][P] fp32 and part_list [Q][parts][P] int32, exactly, as in rule 40.
 *  53. the score: rule 49's dot under the three metrics.  Two fp32 accumulators per (query, centroid) pair start at +0.0, A_hi
 *      and A_lo.  Step t covers elements [16 t, 16 t + 16), t ascending, the rows padded with +0.0: one
 *      v_mfma_f32_32x32x16_f16 of the query fragment with the hi fragment into A_hi and one with the lo fragment into A_lo.
 *      There is no split over D and every pair sees the same instruction sequence.  dot = fl(A_hi + fl(A_lo * 2^-11)).  The
 *      scores: L2 fl(h[l] - dot), IP -dot, COS -fl(dot * r[l]), h and r from mcq_coarse_terms.  The score of a pair is a
 *      function of the two rows, D and the metric alone: not of Q, L, P, `parts`, the alignment of a pointer, or where in a
 *      tile or the grid the pair lands.  Under L2 it is, bit for bit, the score mcq_kmeans_assign_half gives the same pair.
 *  54. the result is rule 42's: the P smallest under "(score, list) ascending" by the one comparison of rule 4, listed in
 *      that order in out_list [Q][P] int32 and out_score [Q][P]; -0.0 and +0.0 are equal scores, ordered by list; a NaN score
 *      is never listed; +inf is listed behind every finite score; the tail is (-1, +inf, bias 0).  The only atomics are
 *      integer counters in LDS.  The result is a function of the scores alone: not of `parts`, and not of the order in which
 *      the centroids come -- a set in which every centroid beats all before it is selected like any other.
 *  55. the bias is rule 43's.  out_bias may be NULL; otherwise out_bias[q][p] = fl(-2 * dot') for the listed centroid, where
 *      dot' is rule 29's plain fp32 dot of the query, every element widened exactly to fp32, with the fp32 centroid row (not
 *      its planes), recomputed for the P winners alone.  For a listed pair these are the bits mcq_coarse_probe reports on the
 *      widened query.
 */
#ifndef MCQ_COARSE_HALF_H
#define MCQ_COARSE_HALF_H

#include "mcq_half.h"

#ifdef __cplusplus
extern "C" {
#endif

long mcq_coarse_half_parts(long Q, long L, int D, int P);
int mcq_coarse_half_split(const float *centroids, long L, int D, uint16_t *planes, void *stream);
int mcq_coarse_probe_half(const uint16_t *queries, long Q, const float *centroids, const uint16_t *planes, long L, int D,
                          const float *terms /* may be NULL under IP */, int P, int metric, long parts,
                          int32_t *out_list, float *out_score, float *out_bias /* may be NULL */,
                          float *part_score, int32_t *part_list, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MCQ_COARSE_HALF_H */
