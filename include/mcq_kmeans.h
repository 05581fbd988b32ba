/* mcq_kmeans.h -- libmcq_hip.so: one Lloyd step over the coarse centroids of an inverted file -- the nearest centroid of every
 * training vector on the fp32 matrix cores, and the members' mean per list as a float64 sum over a fixed tree.
 *
 * A companion of include/mcq.h and its other companions (it includes include/mcq_coarse.h): the same library, the same
 * conventions -- borrowed device pointers, calls that enqueue on the given stream and return, 0 / MCQ_E* / hipError_t as the
 * return value --, and the same ABI version.  Rules 44-47 continue the contract the other headers number 1-43.
 * quantization_amd/_lib.py binds the entries in KMEANS_SIGNATURES; quantization_amd/kmeans.py is the step and the trainer.
 * Common to both entries: the checks come in the stated order before any pointer is looked at, nothing touches the device before
 * they have passed, nothing is ever read back to the host, inputs are never written, a refused call writes nothing, and
 * scratch buffers are typed arguments that are written before they are read.
 *
 *  44. mcq_kmeans_assign, domain and checks.  vectors is [B][D] and centroids [L][D], fp32, rows contiguous; terms is [L], what
 *      mcq_coarse_terms makes under MCQ_SEARCH_L2.  L2 only.  In this order: D > 16,384 is MCQ_EUNSUPPORTED; D < 1, B < 0 or
 *      L < 1 is MCQ_EINVAL; B or L >= 2^31 - 1 is MCQ_EUNSUPPORTED; a missing assign or score (B > 0), and a missing changed
 *      beside a prev_assign, is MCQ_EINVAL.  B == 0 then writes 0 to changed (where prev_assign is given) and nothing else.
 *      Otherwise: `parts` outside [1, ceil(L / 128)] is MCQ_EINVAL, and ceil(B / 128) * parts >= 2^31 - 1 is
 *      MCQ_EUNSUPPORTED; a NULL vectors, centroids, terms, part_score or part_list is MCQ_EINVAL; then the alignments, every
 *      pointer to 4 bytes.
 *      `parts` is the CALLER'S choice: the centroid tiles of 128 rows are cut into that many parts by count, one workgroup
 *      per (128 vectors, part).  Any value of the range is valid and the result does not depend on it.  mcq_kmeans_parts(B,
 *      L, D) recommends one: 1 where the vector tiles alone fill the chip (512 of them), else enough for 512 workgroups,
 *      never more than there are centroid tiles, and 1 outside the domain.  part_score and part_list are [B][parts], exactly.
 *  45. mcq_kmeans_assign, the result.  The score of a (vector, centroid) pair is rule 41's L2 score, bit for bit: one
 *      v_mfma_f32_32x32x2_f32 accumulator per pair that starts at +0.0, the steps ascending over D, zero padding, fl(h[l] -
 *      dot).  (The centroid rides in the A operand and the vector in B, the other way round than in mcq_coarse_probe; a product
 *      does not know which factor came first.)  assign[b] and score[b] are the least pair under rule 42's order, ties to the
 *      lower list; a vector whose every score is NaN gets (-1, +inf).  So assign is mcq_coarse_probe's out_list at P = 1 and
 *      score its out_score, for every input, whatever B, L and `parts`.  With prev_assign [B], changed[0] is the number of b
 *      with assign[b] != prev_assign[b]; the entry zeroes it itself and counts with an integer atomic, the only atomic.
 *      prev_assign may be NULL: changed is then not looked at.
 *  46. mcq_kmeans_update, domain and checks.  vectors is [B][D] in its ORIGINAL order; order is [B] int64 and list_offsets
 *      [L + 1] int64 as build_lists returns them: list l is order[list_offsets[l] .. list_offsets[l + 1]), ascending offsets
 *      within [0, B].  Nothing is permuted or copied: a row is read through a descriptor that covers that row alone, and an
 *      order entry outside [0, B) names no row: it is neither summed nor counted.  (Offsets of another making are cut to [0, B]
 *      and reach no memory outside the arguments; what they return is not stated.)  In this order: D > 16,384 is
 *      MCQ_EUNSUPPORTED; D < 1, B < 0 or L < 1 is MCQ_EINVAL; B or L >= 2^31 - 1, or ceil(B / 4096) + L >= 2^31 - 1, is
 *      MCQ_EUNSUPPORTED; a NULL list_offsets, centroids_in, centroids_out, counts, block_first or block_sums, and a NULL
 *      vectors or order where B > 0, is MCQ_EINVAL; then the alignments: the fp32 and int32 pointers to 4 bytes, the int64 and
 *      float64 ones to 8.  block_first is [L + 1] int64 and block_sums [mcq_kmeans_blocks(B, L, D)] float64, which is
 *      (ceil(B / 4096) + L) * D, and 0 outside the domain.  centroids_out must not overlap an input.
 *  47. mcq_kmeans_update, the result.  n_l is the number of members of list l that name a row; counts[l] = n_l.
 *      centroids_out[l] = (float)(S_l / n_l): the division in float64, rounded once to fp32; a list with n_l == 0 copies
 *      centroids_in[l].  S_l is the float64 sum, element by element, of the list's member rows (each element widened exactly;
 *      a member that names no row contributes +0.0) in ascending position over this FIXED tree: the list is cut into blocks
 *      of 4,096 consecutive members, the last one ragged; a block into 4 quarters of 1,024 consecutive members; a quarter is
 *      summed sequentially from +0.0 (a quarter without members is +0.0); a block's sum is ((q0 + q1) + q2) + q3; the blocks
 *      are added sequentially, ascending, from +0.0.  The row is a function of the list's member rows in their order, and of
 *      D, alone: not of L, B, the list's index, the grid, or where a block lands.  No floating-point atomics, no atomics at
 *      all.  The caller then runs mcq_coarse_terms on the new centroids.
 */
#ifndef MCQ_KMEANS_H
#define MCQ_KMEANS_H

#include "mcq_coarse.h"

#ifdef __cplusplus
extern "C" {
#endif

long mcq_kmeans_parts(long B, long L, int D);
int mcq_kmeans_assign(const float *vectors, long B, const float *centroids, long L, int D, const float *terms, long parts,
                      const int32_t *prev_assign /* may be NULL */, int32_t *assign, float *score,
                      int32_t *changed /* [1]; with prev_assign */, float *part_score, int32_t *part_list, void *stream);
long mcq_kmeans_blocks(long B, long L, int D);
int mcq_kmeans_update(const float *vectors, long B, int D, const int64_t *order, const int64_t *list_offsets, long L,
                      const float *centroids_in, float *centroids_out, int32_t *counts, int64_t *block_first,
                      double *block_sums, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MCQ_KMEANS_H */
