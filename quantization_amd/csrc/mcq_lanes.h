// mcq_lanes.h -- the chunk plan of an encode: how a batch is cut into chunks and how the chunks are dealt to lanes.  Host
// arithmetic only (no device code, nothing of HIP): mcq_api.hip runs the plan, mcq_test_chunk_plan of include/mcq_lanes.h
// reports it, tools/lanes_plan_check.cpp runs it under the host sanitizers.
//
// A LANE is a stream plus its own share of the caller's workspace: everything carve() lays out for a chunk (the x.C region,
// lists, tables, E / R, Gram terms, the 64 pass counters with the recheck counter among them, index arrays and maps).  Lane 0 is
// the caller's stream; lane 1 a side stream of the library.  Chunk i goes to lane i mod lanes, so consecutive chunks of a lane
// reuse its share in stream order and the lanes share nothing they write.
#pragma once
#include <cstddef>

namespace mcq {

constexpr int kMaxLanes = 2;

struct ChunkPlan {
    int lanes = 1;                      // lanes that receive chunks
    long chunk = 0;                     // vectors per chunk; the last chunk holds what is left
    long chunks = 0;                    // ceil(B / chunk)
    size_t lane_off[kMaxLanes] = {};    // byte offset of a lane's share in the workspace (multiples of 256)
    size_t lane_bytes = 0;              // bytes a lane's share is given (>= lane_slack + per * chunk)

    int lane_of(long i) const { return (int)(i % lanes); }
    long first_of(long i) const { return i * chunk; }
    long rows_of(long i, long B) const { return B - i * chunk < chunk ? B - i * chunk : chunk; }
};

// What the workspace holds besides `per` bytes per vector of the chunk(s): two lanes' alignment and padding (lane_slack each), one
// spare vector (an odd batch splits into ceil(B / 2) + floor(B / 2)) and the alignment of the second lane's share.
inline size_t plan_slack(size_t per, size_t lane_slack) { return 2 * lane_slack + per + 256; }

// The one-lane plan: the chunk is what the workspace holds, the whole batch if it can; a chunk that is not the whole batch is a
// multiple of 128 vectors and at least 128.  false: the workspace is too small.
inline bool plan_one_lane(long B, size_t ws_bytes, size_t per, size_t lane_slack, ChunkPlan *p) {
    const size_t slack = plan_slack(per, lane_slack);
    if (B < 1 || per == 0 || ws_bytes < slack + per) return false;
    const size_t holds = (ws_bytes - slack) / per;
    long chunk = holds > (size_t)B ? B : (long)holds;
    if (chunk < B && chunk < 128) return false;
    if (chunk < B) chunk &= ~127L;
    *p = ChunkPlan{};
    p->lanes = 1;
    p->chunk = chunk;
    p->chunks = (B + chunk - 1) / chunk;
    p->lane_bytes = ws_bytes;
    return true;
}

// The two-lane plan: each lane's share holds half of what one lane's would, so the chunk is half the batch (rounded up) if two
// such shares fit, else the largest multiple of 128 that does, by the one-lane rule applied to the share.  false: no two-lane
// plan (one vector, or shares below 128 vectors that do not hold half the batch): the caller takes the one-lane plan.
inline bool plan_two_lanes(long B, size_t ws_bytes, size_t per, size_t lane_slack, ChunkPlan *p) {
    if (B < 2 || per == 0 || ws_bytes < 2 * lane_slack + 256 + 2 * per) return false;
    const size_t holds = (ws_bytes - 2 * lane_slack - 256) / (2 * per);        // vectors per lane
    const long half = (B + 1) / 2;
    long chunk = holds >= (size_t)half ? half : (long)holds;
    if (chunk < half && chunk < 128) return false;
    if (chunk < half) chunk &= ~127L;
    *p = ChunkPlan{};
    p->lanes = 2;
    p->chunk = chunk;
    p->chunks = (B + chunk - 1) / chunk;
    p->lane_bytes = lane_slack + per * (size_t)chunk;
    p->lane_off[1] = (p->lane_bytes + 255) & ~(size_t)255;
    return p->lane_off[1] + p->lane_bytes <= ws_bytes;
}

}  // namespace mcq
