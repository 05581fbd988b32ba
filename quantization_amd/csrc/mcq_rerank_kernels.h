// mcq_rerank_kernels.h -- gfx950 kernel of the exact re-ranking of a shortlist (include/mcq_rerank.h, rules 28-31): gather the
// raw rows a shortlist names, score each against the query in fp32, keep the k best.  The result list, its order and the
// merge of the parts are those of mcq_wide_kernels.h (WideList, pair_less, k_search_wide_merge) and nothing of that file or of
// mcq_search_kernels.h is changed; what is new is the scorer, a pure row gather.
//
// One workgroup per (query, part of the shortlist row).  The query sits in LDS as fp32, padded with zeros to a whole chunk.  A
// wave owns whole candidates: kRerankGroup of them a round, one per lane (the lane holds the candidate's position, its row and
// in the end its score), kRerankRows rows in flight at a time.  A row is read in chunks of kRerankTrips trips of 256
// elements; all the loads of a chunk, of all rows in flight, are issued before the first add, so a row of up to 512
// elements is wholly in flight before anything waits for it.  Lane l reads elements [256 t + 4 l, 256 t + 4 l + 4) of trip t:
// one vector load per trip (16 bytes of fp32, 8 of fp16) where the base pointer is aligned to that and D % 4 == 0 (every row
// is then aligned too), element by element otherwise -- the same values into the same registers, so the same bits.  A
// register without an element holds +0.0 as the padded query does, and its term is +0.0 under every metric: an accumulator
// starts at +0.0 and a sum is -0.0 only if both operands are, so it never is -0.0 and (acc + +0.0) has the bits of acc.
// That is rule 29's "a lane adds its terms in ascending e" with the absent terms left out.
// The bounds: a position is checked against [0, Bs) and a row index against [0, B) before either is used, and a row is read
// through a descriptor that covers that row alone (rerank_row): a candidate that names no row makes no memory access.
#pragma once
#include <hip/hip_fp16.h>

#include "mcq_wide_kernels.h"

namespace mcq {

// ---- launch arithmetic (tests/rerank_grid.py reads these constants from this file and mirrors rerank_plan of mcq_api.hip)
constexpr int kRerankWaves = 4;            // waves per workgroup (256 threads): the WideList's round is one group per wave
constexpr int kRerankGroup = 16;           // candidates of a wave per round, one per lane 0 .. 15
constexpr int kRerankRows = 4;             // rows a wave has in flight
constexpr int kRerankTrips = 2;            // trips of 256 elements whose loads are issued together
constexpr int kRerankMaxD = 16384;         // the longest row: the query takes 64 KiB of LDS as fp32
constexpr int kRerankTargetBlocks = 1024;  // workgroups that fill the chip once (4 per CU, 16 waves per CU)
static_assert(kRerankGroup % kRerankRows == 0 && kRerankGroup <= 64, "a group is whole batches of rows, one candidate per lane");
static_assert(kRerankWaves == kWideWaves, "k_search_wide_merge and the WideList are built for that many waves");

// LDS: [the query, fp32, D rounded up to a chunk][the wide list]
__host__ __device__ constexpr int rerank_query_floats(int D) {
    return (D + 256 * kRerankTrips - 1) / (256 * kRerankTrips) * (256 * kRerankTrips);
}
__host__ __device__ constexpr int rerank_lds_bytes(int D, int k) { return rerank_query_floats(D) * 4 + wide_list_bytes(k); }

template <bool HALF>
__device__ __forceinline__ float rerank_widen(const void *p, long at) {
    if constexpr (HALF) return __half2float(static_cast<const __half *>(p)[at]);
    else return static_cast<const float *>(p)[at];
}

// A row is read through a buffer descriptor of its own: base = the row's first byte, records = its length in bytes, or 0
// for a candidate that names no row.  The hardware's range check then does both bounds of rule 28 without a branch: a lane
// past the end of the row, and every lane of a row-less candidate, makes no memory access and receives zero bits, +0.0 in
// either format.  (Loads under per-lane or per-row branches were tried first: the compiler merged each loaded register with
// its zero through a copy behind s_waitcnt vmcnt(0), so four of a batch's eight loads ran one after the other: 0.43 ms for
// fp32 rows and 0.41 ms for fp16 rows where this form takes 0.39 and 0.25 ms, 1,024 queries x 1,000 candidates of dim 512.)
// The descriptor is built from wave-uniform values only: the kernel argument and a row index that v_readlane put into an
// SGPR.
typedef int rerank_v4i __attribute__((ext_vector_type(4)));
typedef int rerank_v2i __attribute__((ext_vector_type(2)));

template <bool HALF>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rerank_row(const void *vectors, int row, int D) {
    constexpr int EL = HALF ? 2 : 4;
    const char *base = static_cast<const char *>(vectors) + (long)(row >= 0 ? row : 0) * D * EL;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(base), 0, row >= 0 ? D * EL : 0, 0x00020000);
}

// the four elements of one lane and trip, from element e of the row on.  VEC: one load (D % 4 == 0: a group lies wholly
// inside the row or wholly outside); else element by element
template <bool HALF, bool VEC>
__device__ __forceinline__ void rerank_load(float (&x)[4], __amdgpu_buffer_rsrc_t rs, int e) {
    if constexpr (VEC && HALF) {
        const rerank_v2i raw = __builtin_amdgcn_raw_buffer_load_b64(rs, e * 2, 0, 0);
        const unsigned lo = (unsigned)raw[0], hi = (unsigned)raw[1];             // elements e, e + 1 | e + 2, e + 3
        x[0] = __half2float(__ushort_as_half((unsigned short)(lo & 0xffffu)));
        x[1] = __half2float(__ushort_as_half((unsigned short)(lo >> 16)));
        x[2] = __half2float(__ushort_as_half((unsigned short)(hi & 0xffffu)));
        x[3] = __half2float(__ushort_as_half((unsigned short)(hi >> 16)));
    } else if constexpr (VEC) {
        const rerank_v4i raw = __builtin_amdgcn_raw_buffer_load_b128(rs, e * 4, 0, 0);
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = __int_as_float(raw[j]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (HALF) x[j] = __half2float(__ushort_as_half(__builtin_amdgcn_raw_buffer_load_b16(rs, (e + j) * 2, 0, 0)));
            else x[j] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (e + j) * 4, 0, 0));
        }
    }
}

// rule 29's butterfly: the same bits in every lane
__device__ __forceinline__ float rerank_butterfly(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

// a shortlist entry -> (position, row), or (kNoIndex, -1) where it names no candidate (rule 28)
__device__ __forceinline__ void rerank_entry(const int64_t *__restrict__ srow, int S, long long step, long long hi, int lane,
                                             const int64_t *__restrict__ row_of, long Bs, long B, int &pos, int &row) {
    pos = kNoIndex;
    row = -1;
    const long long c = step * kRerankGroup + lane;
    if (step < hi && lane < kRerankGroup && c < S) {
        const int64_t p = srow[c];
        if (p >= 0 && p < Bs) {
            const int64_t r = row_of ? row_of[p] : p;
            if (r >= 0 && r < B) {
                pos = (int)p;                                   // (Bs < 2^31 - 1: never kNoIndex)
                row = (int)r;
            }
        }
    }
}

// The scores of one group: lane j < kRerankGroup holds the row of candidate j (-1: none) and receives its score; the other
// lanes receive 0.  Rows go kRerankRows at a time, a batch without any row is passed over, and the loops over batches and
// chunks stay loops.
template <bool XHALF, int METRIC, bool VEC>
__device__ __forceinline__ float rerank_group(const float *qs, const void *__restrict__ vectors, int D, int chunks, int row,
                                              int lane) {
    constexpr int R = kRerankRows, TR = kRerankTrips;
    float sc = 0.f;
#pragma unroll 1
    for (int j0 = 0; j0 < kRerankGroup; j0 += R) {
        __amdgpu_buffer_rsrc_t rs[R];                        // (wave-uniform)
        int any = -1;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int at = __builtin_amdgcn_readlane(row, j0 + r);
            any = any > at ? any : at;
            rs[r] = rerank_row<XHALF>(vectors, at, D);
        }
        if (any < 0) continue;
        float acc[R], accx[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = accx[r] = 0.f;
#pragma unroll 1
        for (int c = 0; c < chunks; ++c) {
            float x[R][TR][4];
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int t = 0; t < TR; ++t) rerank_load<XHALF, VEC>(x[r][t], rs[r], (c * TR + t) * 256 + lane * 4);
#pragma unroll
            for (int t = 0; t < TR; ++t) {
                const float4 qv = *reinterpret_cast<const float4 *>(qs + (c * TR + t) * 256 + lane * 4);
                const float qe[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float xe = x[r][t][j];
                        if constexpr (METRIC == kMetricL2) {
                            const float d = qe[j] - xe;
                            acc[r] = acc[r] + d * d;
                        } else {
                            acc[r] = acc[r] + qe[j] * xe;
                            if constexpr (METRIC == kMetricCos) accx[r] = accx[r] + xe * xe;
                        }
                    }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float v = rerank_butterfly(acc[r]);
            if constexpr (METRIC == kMetricIP) v = -v;
            if constexpr (METRIC == kMetricCos) v = -(v * rnorm_of(rerank_butterfly(accx[r])));
            if (lane == j0 + r) sc = v;
        }
    }
    return sc;
}

// vec: the vector loads of the header comment may be used (the host decides: base pointer and D)
template <bool QHALF, bool XHALF, int METRIC>
__global__ void __launch_bounds__(64 * kRerankWaves)
k_rerank(const void *__restrict__ queries, const void *__restrict__ vectors, long B, int D,
         const int64_t *__restrict__ shortlist, int S, const int64_t *__restrict__ row_of, long Bs, int k, int parts, int vec,
         float *__restrict__ ws_s, int *__restrict__ ws_i) {
    extern __shared__ __attribute__((aligned(16))) char rerank_smem[];
    constexpr int THREADS = 64 * kRerankWaves, TR = kRerankTrips;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x / parts, part = blockIdx.x % parts;
    const long long T = ((long long)S + kRerankGroup - 1) / kRerankGroup;   // steps: groups of the row
    const long long lo = T * part / parts, hi = T * (part + 1) / parts;
    const long out = ((long)q * parts + part) * k;
    if (lo >= hi) {                                          // no step: the empty list, and nothing is staged
        for (int e = tid; e < k; e += THREADS) {
            ws_s[out + e] = __builtin_inff();
            ws_i[out + e] = kNoIndex;
        }
        return;
    }
    float *qs = reinterpret_cast<float *>(rerank_smem);
    const int Dq = rerank_query_floats(D);
    for (int e = tid; e < Dq; e += THREADS) qs[e] = e < D ? rerank_widen<QHALF>(queries, (long)q * D + e) : 0.f;
    WideList<THREADS> list;
    list.init(rerank_smem + Dq * 4, k, tid);                 // (ends on a barrier: the query is staged)

    const int64_t *srow = shortlist + (long)q * S;
    const int chunks = Dq / (256 * TR);
    long long step = lo + wave;
    int pos, row, pos_next, row_next;
    rerank_entry(srow, S, step, hi, lane, row_of, Bs, B, pos, row);
    int parity = 0;
    for (long long first = lo; first < hi; first += kRerankWaves) {
        if (first > lo) list.begin_round(parity ^ 1, tid);
        if (step < hi) {
            const long long nstep = step + kRerankWaves;
            rerank_entry(srow, S, nstep, hi, lane, row_of, Bs, B, pos_next, row_next);      // one group ahead
            const float sc = vec ? rerank_group<XHALF, METRIC, true>(qs, vectors, D, chunks, row, lane)
                                 : rerank_group<XHALF, METRIC, false>(qs, vectors, D, chunks, row, lane);
            list.offer(sc, pos, pos != kNoIndex, lane);
            pos = pos_next;
            row = row_next;
            step = nstep;
        }
        list.end_round(parity, wave, lane);
        parity ^= 1;
    }
    __syncthreads();
    list.flush(tid);
    for (int e = tid; e < k; e += THREADS) {
        ws_s[out + e] = list.s[e];
        ws_i[out + e] = list.i[e];
    }
}

}  // namespace mcq
