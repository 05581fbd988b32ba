/* mcq_bf16.h -- libmcq_hip.so: the Lloyd step of include/mcq_kmeans.h over a bf16 raw store -- the nearest centroid of every
 * bfloat16 training vector on the bf16 matrix cores, against fp32 centroids split into three bf16 planes, and the members' mean
 * per list gathered from the bf16 rows where they lie.  No fp32 copy of the store is made and nothing of size (B, L).
 *
 * A companion of include/mcq.h and its other companions (it includes include/mcq_kmeans.h): the same library, the same
 * conventions, the same ABI version.  Rules 56-59 continue the contract the other headers number 1-55.
 * quantization_amd/_lib.py binds the entries in BF16_SIGNATURES; quantization_amd/bf16.py is the step and the trainer.
 * As in mcq_kmeans.h: the checks come in the stated order before any pointer is looked at, nothing touches the device before
 * they have passed, nothing is ever read back to the host, inputs are never written, a refused call writes nothing, and scratch
 * buffers are typed arguments that are written before they are read.  Vectors are bfloat16 (the upper 16 bits of an IEEE
 * binary32) as uint16_t; centroids, terms, scores and the new centroids stay fp32.
 *
 *  56. mcq_kmeans_assign_bf16, domain and checks.  vectors is [B][D] bf16 and centroids [L][D] fp32, rows contiguous; terms is
 *      [L], what mcq_coarse_terms makes from the fp32 centroids under MCQ_SEARCH_L2.  L2 only.  The checks, their order, their
 *      return codes and the alignments are rule 48's: vectors to 2 bytes, planes to 16, every other pointer to 4; `planes`
 *      stands beside part_score and part_list among the pointers that must not be NULL.  B == 0 writes 0 to changed (where
 *      prev_assign is given) and nothing else.  `parts` is the caller's choice within [1, ceil(L / 128)] and the result does not
 *      depend on it; mcq_kmeans_bf16_parts(B, L, D) recommends one from this kernel's own plan, which is not rule 44's: its
 *      vector tile has 256 rows and 256 of them fill the chip, so with vt = ceil(B / 256) it is 1 where vt >= 256 or B == 0 or
 *      outside the domain, and min(ceil(256 / vt), ceil(L / 128)) otherwise.  planes is scratch of mcq_kmeans_bf16_planes(L, D)
 *      uint16 elements, which is 3 * L * 32 * ceil(D / 32), and 0 outside the domain: the entry writes all of it before it
 *      reads any of it.
 *  57. mcq_kmeans_assign_bf16, the score: a function of the two rows and D alone.  Each centroid element c is split once per
 *      call into three planes, each conversion rounding to nearest even: hi = bf16(c), mid = bf16(c - f32(hi)) and lo =
 *      bf16((c - f32(hi)) - f32(mid)).  Both subtractions are exact in fp32, and hi + mid + lo = c exactly wherever no piece
 *      falls into the bf16 subnormals; bf16 has fp32's exponent, so nothing is scaled.  A pair has ONE fp32 accumulator A that
 *      starts at +0.0.  Step t covers elements [16 t, 16 t + 16), t ascending, the rows padded with +0.0: three
 *      v_mfma_f32_32x32x16_bf16 of the vector fragment, with the lo, then the mid, then the hi fragment, into A.  There is no
 *      split over D and every pair sees the same instruction sequence.  score = fl(h[l] - A).  So the score does not depend on
 *      B, L, `parts`, the alignment of a pointer or where in a tile a pair lands.  A centroid element that rounds to an
 *      infinite hi gives NaN scores: rule 42 orders them as it orders any other; nothing detects it.  Pairs that hold
 *      subnormal bf16 elements, in a vector or in a plane, are outside the bit-exact promise: the matrix cores may take them
 *      for zero.
 *  58. mcq_kmeans_assign_bf16, the result.  assign[b] and score[b] are the least pair under rule 42's order, ties to the lower
 *      list; a vector whose every score is NaN gets (-1, +inf).  changed, prev_assign, part_score and part_list ([B][parts],
 *      exactly) are rule 45's.
 *  59. mcq_kmeans_update_bf16 is mcq_kmeans_update (rules 46 and 47) with vectors [B][D] bf16, checked to 2 bytes: the same
 *      checks in the same order, the same scratch (block_first [L + 1], block_sums [mcq_kmeans_blocks(B, L, D)]), the same
 *      tree.  Every bf16 element widens exactly to fp32, as its bits shifted left by 16, and to float64, so on rows v it
 *      gives, bit for bit, centroids_out and counts that mcq_kmeans_update gives on the rows widened to fp32.
 */
#ifndef MCQ_BF16_H
#define MCQ_BF16_H

#include "mcq_kmeans.h"

#ifdef __cplusplus
extern "C" {
#endif

long mcq_kmeans_bf16_parts(long B, long L, int D);
long mcq_kmeans_bf16_planes(long L, int D);
int mcq_kmeans_assign_bf16(const uint16_t *vectors, long B, const float *centroids, long L, int D, const float *terms, long parts,
                           const int32_t *prev_assign /* may be NULL */, int32_t *assign, float *score,
                           int32_t *changed /* [1]; with prev_assign */, float *part_score, int32_t *part_list,
                           uint16_t *planes, void *stream);
int mcq_kmeans_update_bf16(const uint16_t *vectors, long B, int D, const int64_t *order, const int64_t *list_offsets, long L,
                           const float *centroids_in, float *centroids_out, int32_t *counts, int64_t *block_first,
                           double *block_sums, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MCQ_BF16_H */
