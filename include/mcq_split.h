/* mcq_split.h -- libmcq_hip.so: the assignment of include/mcq_kmeans.h for fp32 rows on the bf16 matrix cores -- the nearest
 * centroid of every fp32 training vector from six products of bf16 planes, both rows split three ways, with an fp32-grade
 * score.  It stands beside mcq_kmeans_assign, whose bits it does not promise; no plane copy of the store is made and nothing
 * of size (B, L).  The rows are fp32, so the update of a step is mcq_kmeans_update as it stands.
 *
 * A companion of include/mcq.h and its other companions (it includes include/mcq_kmeans.h): the same library, the same
 * conventions, the same ABI version.  Rules 60-63 continue the contract the other headers number 1-59.
 * quantization_amd/_lib.py binds the entries in SPLIT_SIGNATURES; quantization_amd/split.py is the step and the trainer.
 * As in mcq_kmeans.h: the checks come in the stated order before any pointer is looked at, nothing touches the device before
 * they have passed, nothing is ever read back to the host, inputs are never written, a refused call writes nothing, and scratch
 * buffers are typed arguments that are written before they are read.  Vectors, centroids, terms and scores are fp32; planes
 * are bfloat16 (the upper 16 bits of an IEEE binary32) as uint16_t.
 *
 *  60. mcq_kmeans_assign_split, domain, checks and planes.  vectors is [B][D] fp32 and centroids [L][D] fp32, rows
 *      contiguous; terms is [L], what mcq_coarse_terms makes from the centroids under MCQ_SEARCH_L2.  L2 only.  The checks,
 *      their order and their return codes are rule 48's, with these alignments: planes to 16 bytes, vectors and every other
 *      pointer to 4; `planes` stands beside part_score and part_list among the pointers that must not be NULL.  B == 0 writes 0
 *      to changed (where prev_assign is given) and nothing else.  `parts` is the caller's choice within [1, ceil(L / 128)] and
 *      the result does not depend on it; mcq_kmeans_split_parts(B, L, D) recommends one in the form of rule 56 with this
 *      kernel's tile: 128 vectors, of which 256 fill the chip, so with vt = ceil(B / 128) it is 1 where vt >= 256 or B == 0 or
 *      outside the domain, and min(ceil(256 / vt), ceil(L / 128)) otherwise.  planes is scratch of
 *      mcq_kmeans_split_planes(L, D) uint16 elements, which is 3 * L * 32 * ceil(D / 32), and 0 outside the domain: the entry
 *      writes all of it before it reads any of it.  Both rows are split as rule 57 splits a centroid: every element v into
 *      hi = bf16(v), mid = bf16(v - f32(hi)) and lo = bf16((v - f32(hi)) - f32(mid)), each conversion rounding to nearest
 *      even.  Both subtractions are exact in fp32, and hi + mid + lo = v exactly wherever no piece falls into the bf16
 *      subnormals; bf16 has fp32's exponent, so nothing is scaled.  The centroids are split once per call into `planes`; the
 *      vectors are split in the kernel, while a chunk is staged, and their planes exist nowhere in memory.
 *  61. mcq_kmeans_assign_split, the products.  A pair has ONE fp32 accumulator A that starts at +0.0.  Step t covers elements
 *      [16 t, 16 t + 16), t ascending, the rows padded with +0.0: six v_mfma_f32_32x32x16_bf16 into A, in this fixed order
 *      (vector plane . centroid plane): lo.hi, mid.mid, hi.lo, mid.hi, hi.mid, hi.hi.  The three products that are not
 *      formed (mid.lo, lo.mid, lo.lo) are at most 2^-27, 2^-27 and 2^-36 of |x_e| |c_e|, below one fp32 rounding.  On a row
 *      whose elements are all bf16 numbers mid and lo are +0.0 and the sequence is 0, 0, hi.lo, 0, hi.mid, hi.hi, rule 57's lo,
 *      mid, hi: mcq_kmeans_assign_split on bf16 rows widened to fp32 gives the bits of mcq_kmeans_assign_bf16 on those rows.
 *  62. mcq_kmeans_assign_split, the score: score = fl(h[l] - A), h = terms.  There is no split over D and every pair sees the
 *      same instruction sequence, so the score is a function of the two rows and D alone: B, L, `parts`, the alignment of a
 *      pointer and where in a tile a pair lands do not enter.  An infinite element, or a finite one that rounds to an infinite
 *      hi, gives a NaN mid and hence NaN scores: rule 42 orders them as it orders any other; nothing detects it.  Pairs that
 *      hold subnormal bf16 pieces, in a plane of either row, are outside the bit-exact promise: the matrix cores may take
 *      them for zero.
 *  63. mcq_kmeans_assign_split, the result.  assign[b] and score[b] are the least pair under rule 42's order, ties to the lower
 *      list; a vector whose every score is NaN gets (-1, +inf).  changed, prev_assign, part_score and part_list ([B][parts],
 *      exactly) are rule 45's, as in rule 58.
 */
#ifndef MCQ_SPLIT_H
#define MCQ_SPLIT_H

#include "mcq_kmeans.h"

#ifdef __cplusplus
extern "C" {
#endif

long mcq_kmeans_split_parts(long B, long L, int D);
long mcq_kmeans_split_planes(long L, int D);
int mcq_kmeans_assign_split(const float *vectors, long B, const float *centroids, long L, int D, const float *terms, long parts,
                            const int32_t *prev_assign /* may be NULL */, int32_t *assign, float *score,
                            int32_t *changed /* [1]; with prev_assign */, float *part_score, int32_t *part_list,
                            uint16_t *planes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MCQ_SPLIT_H */
