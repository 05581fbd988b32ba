// lanes_plan_check.cpp -- the chunk planner of quantization_amd/csrc/mcq_lanes.h over a grid of batches, workspaces and per-vector
// sizes, as a stand-alone host program (no device, no library): built with the host sanitizers it checks the arithmetic for
// overflow and the invariants the encode relies on.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/lanes_plan_check.cpp -o /tmp/lanes_plan_check
// Exit code 0 and "ok" on success; the first violated invariant is printed otherwise.
#include "../quantization_amd/csrc/mcq_lanes.h"

#include <cstdio>
#include <cstdlib>
#include <initializer_list>

using namespace mcq;

static long g_checked = 0;

#define REQUIRE(cond)                                                                                                        \
    do {                                                                                                                     \
        if (!(cond)) {                                                                                                       \
            std::printf("FAILED %s (line %d): B=%ld ws=%zu per=%zu lane_slack=%zu\n", #cond, __LINE__, B, ws, per, lane_slack); \
            std::exit(1);                                                                                                    \
        }                                                                                                                    \
    } while (0)

static void check_tiling(const ChunkPlan &p, long B, size_t ws, size_t per, size_t lane_slack) {
    long at = 0;
    REQUIRE(p.chunk >= 1 && p.chunks == (B + p.chunk - 1) / p.chunk);
    for (long i = 0; i < p.chunks; ++i) {
        REQUIRE(p.lane_of(i) == (int)(i % p.lanes) && p.first_of(i) == at);
        const long rows = p.rows_of(i, B);
        REQUIRE(rows >= 1 && rows <= p.chunk && (i + 1 == p.chunks || rows == p.chunk));
        at += rows;
    }
    REQUIRE(at == B);
}

static void check(long B, size_t ws, size_t per, size_t lane_slack) {
    ChunkPlan one, two;
    const bool ok1 = plan_one_lane(B, ws, per, lane_slack, &one);
    const bool ok2 = plan_two_lanes(B, ws, per, lane_slack, &two);
    ++g_checked;
    if (ok1) {
        REQUIRE(one.lanes == 1 && one.lane_off[0] == 0);
        REQUIRE(plan_slack(per, lane_slack) + per * (size_t)one.chunk <= ws);          // the chunk fits
        REQUIRE(one.chunk == B || (one.chunk % 128 == 0 && one.chunk >= 128));
        check_tiling(one, B, ws, per, lane_slack);
    }
    if (ok2) {
        const long half = (B + 1) / 2;
        REQUIRE(two.lanes == 2 && two.lane_off[0] == 0 && two.lane_off[1] % 256 == 0);
        REQUIRE(two.lane_bytes == lane_slack + per * (size_t)two.chunk);                // a share holds its chunk
        REQUIRE(two.lane_bytes <= two.lane_off[1] && two.lane_off[1] + two.lane_bytes <= ws);      // disjoint, inside
        REQUIRE(two.chunk == half || (two.chunk < half && two.chunk % 128 == 0 && two.chunk >= 128));
        REQUIRE(two.chunks >= 2);
        check_tiling(two, B, ws, per, lane_slack);
        REQUIRE(!ok1 || two.chunk <= one.chunk);      // one lane's chunk is at least as large
    }
    // the workspace the library asks for: one lane takes the batch whole, two lanes take the halves
    if (B >= 1 && ws == plan_slack(per, lane_slack) + per * (size_t)B) {
        REQUIRE(ok1 && one.chunk == B && one.chunks == 1);
        REQUIRE(B < 2 || (ok2 && two.chunk == (B + 1) / 2 && two.chunks == 2));
    }
}

int main() {
    const size_t pers[] = {1, 97, 2336, 9468, 70000, 1200000};
    const size_t slacks[] = {12288, 12288 + 128 * (4 * 64 + 4), 12288 + 128 * (4 * 16384 + 4)};
    const long batches[] = {0, 1, 2, 3, 127, 128, 129, 255, 256, 257, 300, 8191, 8192, 8320, 32767, 32768, 65535, 65536, 65537, 1 << 20, 123456789};
    for (size_t per : pers)
        for (size_t lane_slack : slacks)
            for (long B : batches) {
                const size_t S = plan_slack(per, lane_slack);
                for (long holds : {0L, 1L, 2L, 127L, 128L, 129L, 255L, 256L, 257L, 511L, 512L, 65536L, B / 2, B, B + 1})
                    for (long d : {-1L, 0L, 1L, 255L})
                        if (holds >= 0 && (long)(S + per * (size_t)holds) + d >= 0) check(B, S + per * (size_t)holds + (size_t)d, per, lane_slack);
                for (size_t ws : {(size_t)0, (size_t)1, lane_slack, 2 * lane_slack, S - 1, S, ~(size_t)0 / 4})
                    check(B, ws, per, lane_slack);
            }
    std::printf("ok: %ld plans checked\n", g_checked);
    return 0;
}
