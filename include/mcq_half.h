/* mcq_half.h -- libmcq_hip.so: the Lloyd step of include/mcq_kmeans.h over an fp16 raw store -- the nearest centroid of every
 * fp16 training vector on the f16 matrix cores, against fp32 centroids split into two fp16 planes, and the members' mean per
 * list gathered from the fp16 rows where they lie.  No fp32 copy of the store is made and nothing of size (B, L).
 *
 * A companion of include/mcq.h and its other companions (it includes include/mcq_kmeans.h): the same library, the same
 * conventions, the same ABI version.  Rules 48-51 continue the contract the other headers number 1-47.
 * quantization_amd/_lib.py binds the entries in HALF_SIGNATURES; quantization_amd/half.py is the step and the trainer.
 * As in mcq_kmeans.h: the checks come in the stated order before any pointer is looked at, nothing touches the device before
 * they have passed, nothing is ever read back to the host, inputs are never written, a refused call writes nothing, and scratch
 * buffers are typed arguments that are written before they are read.  Vectors are IEEE binary16 as uint16_t; centroids, terms,
 * scores and the new centroids stay fp32.
 *
 *  48. mcq_kmeans_assign_half, domain and checks.  vectors is [B][D] fp16 and centroids [L][D] fp32, rows contiguous; terms is
 *      [L], what mcq_coarse_terms makes from the fp32 centroids under MCQ_SEARCH_L2.  L2 only.  The checks, their order and
 *      their return codes are rule 44's, with `planes` beside part_score and part_list among the pointers that must not be
 *      NULL, and these alignments: vectors to 2 bytes, planes to 16, every other pointer to 4.  B == 0 writes 0 to changed
 *      (where prev_assign is given) and nothing else.  `parts` is the caller's choice within [1, ceil(L / 128)] as in rule 44
 *      and the result does not depend on it; mcq_kmeans_half_parts(B, L, D) recommends one by rule 44's formula.  planes is
 *      scratch of mcq_kmeans_half_planes(L, D) uint16 elements, which is 2 * L * 32 * ceil(D / 32), and 0 outside the domain:
 *      the entry writes all of it before it reads any of it.
 *  49. mcq_kmeans_assign_half, the score: a function of the two rows and D alone.  Each centroid element c is split once per
 *      call into hi = f16(c), round to nearest even, and lo = f16((c - f32(hi)) * 2^11); the factor keeps lo out of the fp16
 *      subnormals, and |lo| <= 2^15 cannot overflow where hi is finite.  dot_h(v, c) has two fp32 accumulators that start at
 *      +0.0, A_hi and A_lo.  Step t covers elements [16 t, 16 t + 16), t ascending, the rows padded with +0.0: one
 *      v_mfma_f32_32x32x16_f16 of the vector fragment with the hi fragment into A_hi and one with the lo fragment into A_lo.
 *      There is no split over D and every pair sees the same instruction sequence.  dot = fl(A_hi + fl(A_lo * 2^-11)) and
 *      score = fl(h[l] - dot).  So the score does not depend on B, L, `parts`, the alignment of a pointer or where in a tile
 *      a pair lands.  A centroid element outside the fp16 range has an infinite hi, and its scores are NaN or infinite: rule
 *      42 orders them as it orders any other; nothing detects it.
 *  50. mcq_kmeans_assign_half, the result.  assign[b] and score[b] are the least pair under rule 42's order, ties to the lower
 *      list; a vector whose every score is NaN gets (-1, +inf).  changed, prev_assign, part_score and part_list ([B][parts],
 *      exactly) are rule 45's.
 *  51. mcq_kmeans_update_half is mcq_kmeans_update (rules 46 and 47) with vectors [B][D] fp16, checked to 2 bytes: the same
 *      checks in the same order, the same scratch (block_first [L + 1], block_sums [mcq_kmeans_blocks(B, L, D)]), the same
 *      tree.  Every fp16 element widens exactly to fp32 and to float64, so on rows v it gives, bit for bit, centroids_out and
 *      counts that mcq_kmeans_update gives on the rows widened to fp32.
 */
#ifndef MCQ_HALF_H
#define MCQ_HALF_H

#include "mcq_kmeans.h"

#ifdef __cplusplus
extern "C" {
#endif

long mcq_kmeans_half_parts(long B, long L, int D);
long mcq_kmeans_half_planes(long L, int D);
int mcq_kmeans_assign_half(const uint16_t *vectors, long B, const float *centroids, long L, int D, const float *terms, long parts,
                           const int32_t *prev_assign /* may be NULL */, int32_t *assign, float *score,
                           int32_t *changed /* [1]; with prev_assign */, float *part_score, int32_t *part_list,
                           uint16_t *planes, void *stream);
int mcq_kmeans_update_half(const uint16_t *vectors, long B, int D, const int64_t *order, const int64_t *list_offsets, long L,
                           const float *centroids_in, float *centroids_out, int32_t *counts, int64_t *block_first,
                           double *block_sums, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MCQ_HALF_H */
