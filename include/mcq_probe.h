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

#ifdef __cplusplus
}
#endif
#endif /* MCQ_PROBE_H */
