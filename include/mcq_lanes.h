/* mcq_lanes.h -- libmcq_hip.so: the chunk plan of an encode and the lanes it ran on, for the tests.
 *
 * A companion of include/mcq.h (which it includes): the same library and conventions.  An encode cuts its batch into chunks that
 * fit the workspace.  A batch below the lane threshold runs them one after the other on the caller's stream, each on the whole
 * workspace.  A larger batch runs them on two LANES: lane 0 is the caller's stream, lane 1 a side stream the library keeps per
 * device; each lane owns a share of the workspace that holds one chunk (everything the encode lays out per chunk: products,
 * lists, tables, E / R, Gram terms, counters, index arrays and maps), chunk i runs on lane i mod 2, and the chunk is half the
 * one-lane chunk, so the workspace does not grow with the lanes.  One event forks lane 1 behind the caller's stream at entry, one
 * joins it at exit; in between the lanes never wait for each other.
 *
 * Tuning hooks, read per call; neither changes a result:
 *   MCQ_ENCODE_LANES=1        one lane at the one-lane chunk size, whatever the batch; 2: a second lane from the threshold on
 *   MCQ_ENCODE_LANES_MIN=<n>  the threshold in vectors (0: any batch of two vectors or more)                                  */
#ifndef MCQ_LANES_H
#define MCQ_LANES_H

#include "mcq.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The plan of a batch of B >= 1 vectors in a workspace of workspace_bytes.  Host arithmetic only: no device is touched, so what
 * an encode decides at run time (a capturing stream or a missing side stream takes the one-lane plan) is not seen here.
 *   lanes   0: as the encode decides from B and the hooks; 1 / 2: that plan (2 falls back to 1 where no two-lane plan exists:
 *           B == 1, or shares of less than 128 vectors that do not hold half the batch)
 *   out[i], i < min(cap, 6):  lanes, vectors per chunk, number of chunks, byte offset of lane 0's share, of lane 1's share, the
 *           bytes a share is given
 *   out[6 + 3 c ..], while they fit cap: lane, first vector and number of vectors of chunk c
 * A chunk that is not the whole batch (one lane) or half of it rounded up (two lanes) is a multiple of 128 vectors.
 * Returns 6 (MCQ_TEST_CHUNK_PLAN_HEAD); the domain of (N, K, D) first (MCQ_EUNSUPPORTED / MCQ_EINVAL); B < 1, lanes outside
 * 0 .. 2, out == NULL or cap < 0: MCQ_EINVAL; a workspace that holds no plan: MCQ_EWORKSPACE.                                */
#define MCQ_TEST_CHUNK_PLAN_HEAD 6
int mcq_test_chunk_plan(long B, int N, int K, int D, size_t workspace_bytes, int lanes, long *out, int cap);

/* The number of streams the last encode on this thread enqueued on: 2 if it forked a second lane, else 1 (0: none yet).     */
int mcq_last_encode_lanes(void);

#ifdef __cplusplus
}
#endif
#endif /* MCQ_LANES_H */
