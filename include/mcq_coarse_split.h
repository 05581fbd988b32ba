/* mcq_coarse_split.h -- libmcq_hip.so: the coarse probes of include/mcq_coarse.h for fp32 queries on the bf16 matrix cores --
 * score every fp32 query against every coarse centroid from six products of bf16 planes, both rows split three ways, with an
 * fp32-grade score, and keep the P best per query, exactly, in a bounded heap per query; with them the per-probe bias a store of
 * residual codes takes.  It stands beside mcq_coarse_probe, whose score bits it does not promise; nothing of size (Q, L).
 *
 * A companion of include/mcq.h and its other companions (it includes include/mcq_split.h and include/mcq_coarse.h): the same
 * library, the same conventions, the same ABI version.  Rules 64-67 continue the contract the other headers number 1-63.
 * quantization_amd/_lib.py binds the entries in COARSE_SPLIT_SIGNATURES; quantization_amd/split.py has coarse_planes_split and
 * coarse_probe_split.  As in mcq_coarse_half.h: the checks come in the stated order before any pointer is looked at, nothing
 * touches the device before they have passed, nothing is ever read back to the host, inputs are never written, a refused call
 * writes nothing, and scratch buffers are typed arguments that are written before they are read.  Queries, centroids, terms,
 * scores and biases are fp32; planes are bfloat16 (the upper 16 bits of an IEEE binary32) as uint16_t.
 *
 *  64. domain and checks.  queries is [Q][D] fp32 and centroids [L][D] fp32, rows contiguous; terms is [L], what
 *      mcq_coarse_terms makes from the centroids under the metric (NULL is allowed under IP).  planes holds
 *      mcq_kmeans_split_planes(L, D) elements in rule 57's split: the hi rows [L][Dp], then the mid rows, then the lo rows,
 *      Dp = 32 * ceil(D / 32), an element past D +0.0.  mcq_coarse_split_planes(rows, R, D, planes) writes exactly that for R
 *      rows, mcq_kmeans_split_planes(R, D) elements, ONCE per centroid set: for the probe the centroids' planes are a const
 *      input.  Its checks are those of mcq_coarse_half_split: D > 16,384 is MCQ_EUNSUPPORTED; D < 1 or R < 0 MCQ_EINVAL;
 *      R >= 2^31 - 1 MCQ_EUNSUPPORTED; R == 0 does nothing; a NULL pointer, rows off 4 bytes or planes off 16 MCQ_EINVAL.
 *      mcq_coarse_probe_split, in rule 52's order and with its return codes: D > 16,384 or P > 128 is MCQ_EUNSUPPORTED;
 *      D < 1, P < 1 or a negative Q or L is MCQ_EINVAL; an unknown metric (rule 1) is MCQ_EINVAL; Q or L >= 2^31 - 1 is
 *      MCQ_EUNSUPPORTED; a missing out_list or out_score (Q > 0) is MCQ_EINVAL.  Q == 0 then does nothing and returns 0.
 *      L == 0 looks at no input, at no part buffer and not at query_planes and writes P entries of the tail per query.
 *      Otherwise: `parts` outside [1, ceil(L / 128)] is MCQ_EINVAL, and (query tiles) * parts >= 2^31 - 1 is MCQ_EUNSUPPORTED,
 *      a query tile being 128 queries for P <= 64 and 64 beyond; a NULL queries, centroids, planes, part_score, part_list or
 *      query_planes, and a NULL terms unless the metric is IP, is MCQ_EINVAL; then the alignments: planes and query_planes to
 *      16 bytes, queries and every other pointer to 4.
 *      `parts` is the CALLER'S choice: the centroid tiles of 128 rows are cut into that many parts by count, one workgroup per
 *      (query tile, part).  Any value of the range is valid and the result does not depend on it.  mcq_coarse_split_parts(Q,
 *      L, D, P) recommends one in rule 52's form with this kernel's tile: 1 where the query tiles alone fill the chip (256 of
 *      them: one workgroup per compute unit in every class of P), else enough to reach that number, never more than there are
 *      centroid tiles, and 1 outside the domain.  part_score is [Q][parts][P] fp32 and part_list [Q][parts][P] int32, exactly,
 *      as in rule 40.  query_planes is scratch of mcq_kmeans_split_planes(Q, D) uint16 elements: the entry splits the queries
 *      into it once per call, as rule 57 splits a centroid, and writes all of it before it reads any of it.
 *  65. the score: rule 61's accumulator, unchanged, under the three metrics.  A pair has ONE fp32 accumulator A that starts at
 *      +0.0.  Step t covers elements [16 t, 16 t + 16), t ascending, the rows padded with +0.0 to Dp: six
 *      v_mfma_f32_32x32x16_bf16 into A, in this fixed order (query plane . centroid plane): lo.hi, mid.mid, hi.lo, mid.hi,
 *      hi.mid, hi.hi.  There is no split over D and every pair sees the same instruction sequence.  The scores are finished as
 *      rule 53 finishes its dot: L2 fl(h[l] - A), IP -A, COS -fl(A * r[l]), h and r from mcq_coarse_terms.  The score of a pair
 *      is a function of the two rows, D and the metric alone: not of Q, L, P, `parts`, the alignment of a pointer, or where in
 *      a tile or the grid the pair lands.  Rule 61 splits a vector exactly as rule 57 splits a centroid, so under L2 the score
 *      of a pair is, bit for bit, the score mcq_kmeans_assign_split gives the same pair.  Rule 62's caveats carry over: an
 *      infinite element, or a finite one that rounds to an infinite hi, gives a NaN mid and hence NaN scores, which are never
 *      listed; pairs that hold subnormal bf16 pieces, in a plane of either row, are outside the bit-exact promise.
 *  66. the result is rule 42's, as in rule 54: the P smallest under "(score, list) ascending" by the one comparison of rule 4,
 *      listed in that order in out_list [Q][P] int32 and out_score [Q][P]; -0.0 and +0.0 are equal scores, ordered by list; a
 *      NaN score is never listed; +inf is listed behind every finite score; the tail is (-1, +inf, bias 0).  There is no
 *      atomic.  The result is a function of the scores alone: not of `parts`, and not of the order in which the centroids come
 *      -- a set in which every centroid beats all before it is selected like any other.
 *  67. the bias is rule 43's, by the kernel that finishes mcq_coarse_probe, on the fp32 queries as they are.  out_bias may be
 *      NULL; otherwise out_bias[q][p] = fl(-2 * dot') for the listed centroid, where dot' is rule 29's plain fp32 dot of the
 *      fp32 query with the fp32 centroid row (not their planes), recomputed for the P winners alone.  For a listed pair these
 *      are the bits mcq_coarse_probe reports.
 */
#ifndef MCQ_COARSE_SPLIT_H
#define MCQ_COARSE_SPLIT_H

#include "mcq_split.h"
#include "mcq_coarse.h"

#ifdef __cplusplus
extern "C" {
#endif

long mcq_coarse_split_parts(long Q, long L, int D, int P);
int mcq_coarse_split_planes(const float *rows, long R, int D, uint16_t *planes, void *stream);
int mcq_coarse_probe_split(const float *queries, long Q, const float *centroids, const uint16_t *planes, long L, int D,
                           const float *terms /* may be NULL under IP */, int P, int metric, long parts,
                           int32_t *out_list, float *out_score, float *out_bias /* may be NULL */,
                           float *part_score, int32_t *part_list, uint16_t *query_planes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MCQ_COARSE_SPLIT_H */
