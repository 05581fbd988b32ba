/* mcq_probe.h -- libmcq_hip.so: probes of single steps of the encode, for the tests.
 *
 * A companion of include/mcq.h (which it includes): the same library, the same conventions -- borrowed device pointers, calls
 * that enqueue on the given stream and return, 0 / MCQ_E* / hipError_t as the return value --, and the same ABI version.  The
 * entries here run one step of the encode through the launcher the encode itself uses, on inputs the caller supplies; no product
 * code needs them.  quantization_amd/_lib.py binds them in PROBE_SIGNATURES, beside the SIGNATURES of mcq.h.                  */
#ifndef MCQ_PROBE_H
#define MCQ_PROBE_H

#include "mcq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* E = |x_err|^2 and R[n] = |x_err - old_n|^2 of B slots, as a refinement pass forms them ahead of its stage 0 (the numeric contract:
 * oracle/mcq_oracle.c, "TABLE FORM", E, R).
 *   prepared     the blob of mcq_prepare* for (N, K, D): its Gram matrix is read
 *   xc, xx       float[rows][N*K] x.C products and float[rows] |x|^2 of the call's rows (mcq_test_xc and the limb kernel form them)
 *   idx          uint8[B][N], the current codes of the slots, every one < K; 16-byte aligned.  One-byte entries only:
 *                K > 256 is MCQ_EUNSUPPORTED
 *   nact         NULL, or a device int: only the slots below *nact are formed, the others of E_out / R_out are not written
 *   map          NULL (slot b is row b of xc / xx), or int32[B]: slot b is row map[b]
 *   form         0: the one launch that gathers the Gram entries itself (what the encode uses up to 8,192 vectors);
 *                1: the pair of launches of larger chunks (Gram terms XCD by XCD, then the sums); anything else: MCQ_EINVAL
 *   E_out, R_out float[B], float[B][N]
 *   workspace    mcq_test_er_workspace_bytes(B, N) bytes (the Gram terms of form 1), 256-byte aligned
 * Checks in this order: the domain of (N, K, D) and K <= 256; B < 0 or a form other than 0 / 1: MCQ_EINVAL; B == 0 returns 0 and
 * looks at nothing; NULL prepared / xc / xx / idx / E_out / R_out / workspace or a misaligned idx or workspace: MCQ_EINVAL; a
 * workspace that is too small: MCQ_EWORKSPACE.                                                                                 */
size_t mcq_test_er_workspace_bytes(long B, int N);
int mcq_test_er(const void *prepared, int N, int K, int D, const float *xc, const float *xx, const uint8_t *idx, long B,
                const int *nact /* may be NULL */, const int *map /* may be NULL */, int form, float *E_out, float *R_out,
                void *workspace, size_t workspace_bytes, void *stream);


/* mcq_test_xc of include/mcq.h (same arguments, checks and workspace: mcq_logits_workspace_bytes) that also leaves, in
 * xx_out[B], the |x - mean|^2 the limb kernel forms for the passes; xx_out == NULL with B > 0 is MCQ_EINVAL.                 */
int mcq_test_xc_xx(const float *x, long B, const void *prepared, int N, int K, int D, float *xc_out, float *xx_out,
                   void *workspace, size_t workspace_bytes, void *stream, unsigned flags);


/* Where the arrays of one chunk of B vectors lie in the encode's workspace (host only; reported by the function that lays the
 * workspace out for the encode, not by a copy of its arithmetic).  out[i], i < min(cap, 64), receive, in this fixed order:
 *   out[2 a], out[2 a + 1]   byte offset and byte size of array a; an array the shape does not have (a level without a list,
 *                            the group tables of fewer than 8 codebooks) reports 0, 0
 *      a = 0 idx   1 idxB   2 idxC   3 final_idx     codes, [B][N] of `code width` bytes (idx: the current codes, refined in place)
 *          4, 5 map[0..1]  int32[B]      6 cnt  int32[64]                      (fixed-point skipping)
 *          7 E  float[B]   8 R  float[B][N]   9 xx  float[B]   10 gterms  float[B][N][N]   11 XC  float[B][N*K]
 *          12 xf  limb planes of the centered frames   13 xe  their exponents, int32 per padded row
 *          14 ent            level-0 lists: [B][N][kc[0]] codebook entries of `code width` bytes
 *          15 .. 19 pos[1..5]   level v: uint8[B][N >> v][kc[v]][2], the positions in the two halves' lists
 *          20 .. 25 S[0..5]     level v: float[B][N >> v][kc[v]], the candidates' scores
 *          26, 27 tabs[0..1]    group tables (two consecutive levels)
 *   out[56 .. 61]  kc[0..5], the list length of every level (also of levels the shape has no list of)
 *   out[62]        the code width: 1 byte up to 256 entries per codebook, 2 above
 *   out[63]        the end of the last array rounded up to 256: what one chunk of B occupies
 * Every offset is a multiple of 256.  Returns 64 (MCQ_TEST_PASS_LAYOUT_VALUES).  Checks in this order: the domain of (N, K, D) as
 * the encode (MCQ_EUNSUPPORTED / MCQ_EINVAL); B < 1, out == NULL or cap < 0: MCQ_EINVAL.                                        */
#define MCQ_TEST_PASS_LAYOUT_VALUES 64
int mcq_test_pass_layout(long B, int N, int K, int D, size_t *out, int cap);

/* ONE refinement pass of B vectors as ONE chunk, from caller-supplied codes, through the launchers of the encode's own pass loop
 * (the chunk start with imported codes: frames to limb planes, k_import_indexes, the x.C product; then E / R, stage 0 and the
 * combines as separate launches -- never the LDS-resident pass of 8 x 16 and 16 x 16, which mcq_test_pass16 below runs; no
 * fixed-point skipping of its own, E / R of a next pass not formed).  What the pass leaves in `workspace` is read by mcq_test_pass_layout(B, ...).
 *   x            fp32 [B][D], the frames (row r)
 *   idx_in       int64 [B][N], the current codes of the SLOTS, every one in [0, K)
 *   idx_out      int64 [B][N]: the new codes of slot b go to row b, or to row map[b]; they are also left in the workspace's idx,
 *                slot by slot.  May alias idx_in where map is NULL
 *   nact         NULL, or a device int: only the slots below *nact are processed, nothing of the other slots is written
 *   map          NULL (slot b is row b of x), or int32[B]: slot b holds the vector of row map[b] (its x.C products, its |x|^2,
 *                its row of idx_out)
 *   flags        MCQ_TEST_PASS_CAPPED: the capped launchers (grid-stride instantiations of stage 0, the level-0 and level-1
 *                kernels and the last combine, as the encode takes them from the fourth pass of fixed-point skipping on)
 *   workspace    256-byte aligned, large enough for the encode to take B vectors as one chunk
 *                (mcq_encode_workspace_bytes(B, N, K, D) is, for every B up to the default chunk)
 * mcq_last_encode_launches() counts the launches of the call.  Checks in this order: the domain of (N, K, D); N == 1 (no lists):
 * MCQ_EUNSUPPORTED; B < 0 or an unknown flag: MCQ_EINVAL; B == 0 returns 0 and looks at nothing; NULL x / prepared / idx_in /
 * idx_out / workspace or a misaligned workspace: MCQ_EINVAL; a workspace that does not hold B as one chunk: MCQ_EWORKSPACE.   */
#define MCQ_TEST_PASS_CAPPED 1u
int mcq_test_pass(const float *x, long B, const void *prepared, int N, int K, int D, const int64_t *idx_in, int64_t *idx_out,
                  const int *nact /* may be NULL */, const int *map /* may be NULL */, unsigned flags, void *workspace,
                  size_t workspace_bytes, void *stream);


/* One record of the LDS-resident pass of 8 x 16 and 16 x 16 codebooks (k_tf_pass16<N>, which mcq_test_pass never takes; its probe
 * instantiation k_tf_pass16_probe<N> is the same body with the records added).  After the winner's walk of pass p of vector b, and
 * before the wave leaves a vector at its fixed point, the wave writes record b * iters + p.  A record is the list part of the
 * wave's LDS scratch as it lies, then what the pass held in registers (host only; the constants the kernel itself uses).  out[i],
 * i < min(cap, 25), receive
 *   out[2 a], out[2 a + 1]   byte offset in the record and byte size of array a; an array N codebooks do not have reports 0, 0
 *      a = 0 ent  uint8[N][8]            the level-0 lists: codebook entries
 *          1 pos1 uint8[N/2][8][2]   2 pos2 uint8[N/4][16][2]   3 pos3 uint8[2][16][2] (N = 16 only)   positions in the halves' lists
 *          4 S0 float[N][8]   5 S1 float[N/2][8]   6 S2 float[N/4][16]   7 S3 float[2][16] (N = 16 only)   the candidates' scores
 *          8 E  float         9 R  float[N]      E and R[n] of the pass
 *          10 idx uint8[N]    the codes the pass leaves
 *          11 mark uint32     0x36315021: the record was written
 *   out[24]                  the bytes of one record (the same for both N; a multiple of 4)
 * The bytes of a record outside these arrays hold whatever the scratch held (with N = 8, scratch the kernel never writes) or are
 * not written.  Returns 25 (MCQ_TEST_PASS16_LAYOUT_VALUES).  N other than 8 or 16: MCQ_EUNSUPPORTED; out == NULL or cap < 0:
 * MCQ_EINVAL.                                                                                                                   */
#define MCQ_TEST_PASS16_LAYOUT_VALUES 25
#define MCQ_TEST_PASS16_WRITTEN 0x36315021u
int mcq_test_pass16_layout(int N, size_t *out, int cap);

/* `iters` refinement passes of B vectors of N x 16 codebooks, N = 8 or 16, as ONE chunk, from caller-supplied codes, through the
 * LDS-resident pass: the encode's own chunk start with imported codes (as mcq_test_pass), then the launcher the encode calls
 * for these shapes -- one launch for all passes, a wave leaves a vector after the first pass that returns its input.
 *   x, idx_in    as mcq_test_pass
 *   idx_out      int64 [B][N]: the codes after the last pass a vector ran; they are also left in the workspace's idx
 *   dump         NULL: the instantiation the encode itself launches (k_tf_pass16<N>).  Else 4-byte aligned device memory of at
 *                least B * iters records: the probe instantiation, which writes record b * iters + p for every pass p vector
 *                b runs and nothing of the records of later passes
 *   max_workgroups  0: the launcher's own grid; positive: at most that many workgroups of eight waves (the kernel strides by
 *                its grid, so with 1 every wave carries B / 8 vectors one after the other through the same scratch)
 *   workspace    as mcq_test_pass
 * mcq_last_encode_launches() counts the launches of the call.  Checks in this order: the domain of (N, 16, D); N other than 8 or
 * 16: MCQ_EUNSUPPORTED; B < 0, iters outside 1 .. 60 or max_workgroups < 0: MCQ_EINVAL; B == 0 returns 0 and looks at nothing;
 * NULL x / prepared / idx_in / idx_out / workspace or a misaligned workspace or dump: MCQ_EINVAL; a workspace that does not hold
 * B as one chunk, then a dump of fewer than B * iters records: MCQ_EWORKSPACE.                                                  */
int mcq_test_pass16(const float *x, long B, const void *prepared, int N, int D, int iters, const int64_t *idx_in, int64_t *idx_out,
                    void *dump /* may be NULL */, size_t dump_bytes, int max_workgroups, void *workspace, size_t workspace_bytes,
                    void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MCQ_PROBE_H */
