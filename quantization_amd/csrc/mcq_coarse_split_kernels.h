// mcq_coarse_split_kernels.h -- gfx950 kernel of the coarse probes for fp32 queries on the bf16 matrix cores
// (include/mcq_coarse_split.h, rules 64-67): score every fp32 query against every coarse centroid from six products of bf16
// planes and keep the P best per query, exactly.  The product is rule 61's (the three planes of k_bf16_split on BOTH sides,
// v_mfma_f32_32x32x16_bf16, one fp32 accumulator a pair, the order of k_kmeans_assign_split); the plane row loads
// (half_load<true>, half_keep) are those of mcq_half_kernels.h; the order (pair_less), the merge of the parts and the winners'
// bias (k_coarse_finish) are those of mcq_coarse_kernels.h.  Nothing of those files is changed.
//
// k_coarse_probe_split<METRIC, CLASS>: one workgroup of W waves per (tile of 32 W queries, part of the centroid tiles of 128),
// one workgroup per compute unit.  BOTH operands arrive as 16-bit plane rows: the host splits the queries once per call with
// k_bf16_split as it splits the centroids, so the kernel moves 16-byte groups from memory to LDS without looking into them.
// A query is owned by ONE wave: wave w holds queries 32 w .. 32 w + 31 of the tile against all 128 centroids, as 4 blocks of
// 32 x 32 with one accumulator each: 64 registers.  The CENTROIDS are the A operand, as in k_coarse_probe_half: lane l supplies
// 8 elements of row l % 32 at k = 8 (l / 32) and receives, in register r of block ci, the dot of query l % 32 with centroid
// 32 ci + 8 (r / 4) + 4 (l / 32) + r % 4.  So a lane holds ONE query and 16 centroids of each block, the two lanes of a query
// sit in the same wave, and the query's bound is a register pair that every score meets before anything touches LDS.
// D goes through LDS in chunks of 16 elements -- ONE step -- double-buffered, one barrier a chunk: a staged row is 32 bytes at
// a pitch of 48 (12 banks: the 16 lanes of a quarter-wave read 16 distinct groups of 4 banks).  A step reads 15 fragments of 16
// bytes (3 query planes, 3 x 4 centroid planes) and issues 24 MFMAs: per block, in rule 61's order (query plane . centroid
// plane) lo.hi, mid.mid, hi.lo, mid.hi, hi.mid, hi.hi; the four blocks alternate inside each product, so no MFMA waits for the
// one before it.  Thread t stages elements [8 (t % 2), 8 (t % 2) + 8) of row t / 2 of each query plane and of rows t / 2 +
// 32 W j of each centroid plane: 6 groups of 16 bytes with 4 waves, 9 with 2.  The terms of a tile's 128 centroids sit in LDS
// by tile parity, as in k_kmeans_assign_split.
//
// Selection: a bounded binary MAX-heap per query under pair_less, in LDS, written by ONE lane.  Entry e of the heap of the
// wave's query j lies at [e][j] of the wave's region: the 32 lanes that work 32 heaps at the same depth touch 32 consecutive
// entries.  The root is the worst entry kept, so once the heap holds P entries the root IS the bound; before that the bound is
// (+inf, kNoIndex), which every score but a NaN passes.  After a block of 32 centroids the 16 scores of a lane meet the register
// bound one by one; where any lane of the wave has a survivor the upper lane of a query hands its score to the lower lane by
// one cross-lane move and the lower lane -- the only writer -- appends and sifts up (heap not full), or replaces the root, sifts
// down and reloads the bound (full), its own survivor first, then the partner's, which meets the new bound again.  The 32
// heaps of a wave are worked by 32 lanes with divergent trip counts.  The fill count lives in a register of the writer: no
// counter in LDS, no atomic, no sort, and no workgroup barrier in the epilogue (coarse_wave_sync alone, once, before the part
// leaves).  pair_less is a strict total order over what a heap holds (a NaN never passes a bound; a centroid is offered once),
// so the SET a heap ends with does not depend on the order of arrival; it leaves in heap order, P entries a part, the tail as
// (+inf, -1), and k_coarse_finish, which offers the part entries to a WideList in any order, sorts.
// The classes of P (the host picks; heap capacity C, queries of a tile, all LDS):
//     P <= 32:  C = 32,  128 queries, 4 waves: 2 x 768 x 48 + 1,024 + 128 x 32 x 8 = 107,520 B
//     P <= 64:  C = 64,  128 queries, 4 waves: 73,728 + 1,024 + 65,536 = 140,288 B
//     P <= 128: C = 128,  64 queries, 2 waves: 2 x 576 x 48 + 1,024 + 64 x 128 x 8 = 121,856 B
// all within the 160 KiB (163,840 B) of a compute unit and without scratch (profiles/coarse_split_isa.txt).
#pragma once
#include "mcq_split_kernels.h"

namespace mcq {

// ---- launch arithmetic (mcq_coarse_split_parts of mcq_api.hip is the plan, and the caller may choose another)
constexpr int kCsBlocks = 4;               // blocks of 32 centroids a wave holds
constexpr int kCsCT = 32 * kCsBlocks;      // centroid rows of a tile
constexpr int kCsDC = 16;                  // elements of a D chunk: one step
constexpr int kCsPitch = kCsDC + 8;        // 16-bit elements of a staged row: 48 bytes
constexpr int kCsFullBlocks = 256;         // query tiles that fill the chip alone: one workgroup per CU
__host__ __device__ constexpr int coarse_split_class(int P) { return P <= 32 ? 0 : (P <= 64 ? 1 : 2); }
__host__ __device__ constexpr int coarse_split_waves(int cls) { return cls == 2 ? 2 : 4; }
__host__ __device__ constexpr int coarse_split_queries(int cls) { return 32 * coarse_split_waves(cls); }
__host__ __device__ constexpr int coarse_split_heap(int cls) { return 32 << cls; }
// one buffer: the queries' hi, mid, lo rows, then the centroids'
__host__ __device__ constexpr int coarse_split_stage(int cls) { return (3 * coarse_split_queries(cls) + 3 * kCsCT) * kCsPitch; }
// LDS: [2 staging buffers][terms 2 x 128][heap entries (score, list): C x 32 per wave]
__host__ __device__ constexpr int coarse_split_lds(int cls) {
    return 2 * coarse_split_stage(cls) * 2 + 2 * kCsCT * 4 + coarse_split_queries(cls) * coarse_split_heap(cls) * 8;
}
static_assert(kCsPitch * 2 % 16 == 0 && half_padded_dim(1) % kCsDC == 0, "a fragment is one aligned 16-byte read; a padded row is whole chunks");
static_assert(coarse_split_heap(coarse_split_class(32)) >= 32 && coarse_split_heap(coarse_split_class(64)) >= 64 &&
              coarse_split_heap(coarse_split_class(kCoarseMaxP)) >= kCoarseMaxP, "a heap holds the P of its class");
static_assert(coarse_split_lds(0) <= 160 * 1024 && coarse_split_lds(1) <= 160 * 1024 && coarse_split_lds(2) <= 160 * 1024 &&
              (2 * coarse_split_stage(1) * 2) % 16 == 0, "the LDS budget");

// query_planes, planes: what k_bf16_split wrote for the queries and for the centroids.  terms: as k_coarse_scores takes them
// (NULL under the inner product).  Part s of query q leaves as P entries in heap order at part_score / part_list
// [(q * parts + s) * P]; the tail is (+inf, -1)
template <int METRIC, int CLASS>
__global__ void __launch_bounds__(64 * coarse_split_waves(CLASS), 1)
k_coarse_probe_split(const unsigned short *__restrict__ query_planes, int Q, const unsigned short *__restrict__ planes, int L, int D,
                     const float *__restrict__ terms, int P, int parts, float *__restrict__ part_score,
                     int *__restrict__ part_list) {
    constexpr int WAVES = coarse_split_waves(CLASS), QT = 32 * WAVES, CAP = coarse_split_heap(CLASS);
    constexpr int STAGE = coarse_split_stage(CLASS), CPASS = kCsCT / QT;     // a thread stages CPASS rows of each centroid plane
    extern __shared__ __attribute__((aligned(16))) char coarse_split_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qt = blockIdx.x / parts, part = blockIdx.x % parts;
    const long q0 = (long)qt * QT;
    const long T = ((long)L + kCsCT - 1) / kCsCT;
    const long lo = T * part / parts, hi = T * (part + 1) / parts;
    const int Dp = half_padded_dim(D), chunks = Dp / kCsDC;
    const long qplane = (long)Q * Dp, cplane = (long)L * Dp;

    unsigned short *stage = reinterpret_cast<unsigned short *>(coarse_split_smem);
    float *tt = reinterpret_cast<float *>(coarse_split_smem + 2 * STAGE * 2);
    const int srow = tid >> 1, scol = (tid & 1) * 8;         // staging: this thread's first row and first element of a chunk
    const int frow = lane & 31, half = lane >> 5;            // fragments: this lane's row and k group of a step
    const int qi = 32 * wave + frow;                         // this lane's query of the tile: its wave owns it
    const bool qthere = q0 + qi < Q;
    // the heap of this lane's query: entry e at hp[32 e].  Wave-private, and written by the lower lane of the query alone
    float2 *hp = reinterpret_cast<float2 *>(tt + 2 * kCsCT) + 32 * wave * CAP + frow;
    int n = 0;                                               // (lower lane)  entries in the heap
    float bs = __builtin_inff();                             // the bound of query qi: the root once the heap is full
    int bi = kNoIndex;

    const unsigned short *qtile = query_planes + q0 * Dp;
    const int qleft = (int)(Q - q0);
    uint4 rq[3], rc[3][CPASS];
    bool okq, okc[CPASS];
    auto load = [&](long tile, int c) {
        const int e = c * kCsDC + scol;                      // (e < Dp: a padded row is wholly there)
        const unsigned short *ctile = planes + tile * kCsCT * Dp;
        const int cleft = (int)(L - tile * kCsCT);
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            rq[p] = half_load<true>(qtile + p * qplane, srow, qleft, Dp, e, okq);
#pragma unroll
            for (int j = 0; j < CPASS; ++j) rc[p][j] = half_load<true>(ctile + p * cplane, srow + QT * j, cleft, Dp, e, okc[j]);
        }
    };
    auto store = [&](int buf) {
        unsigned short *b = stage + buf * STAGE + srow * kCsPitch + scol;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            *reinterpret_cast<uint4 *>(b + QT * p * kCsPitch) = half_keep(okq, rq[p]);
#pragma unroll
            for (int j = 0; j < CPASS; ++j)
                *reinterpret_cast<uint4 *>(b + (3 * QT + kCsCT * p + QT * j) * kCsPitch) = half_keep(okc[j], rc[p][j]);
        }
    };
    // (lower lane)  an entry below the bound goes into the heap; the bound is the root from the moment the heap is full
    auto push = [&](float s, int c) {
        const float2 entry = make_float2(s, __int_as_float(c));
        int i;
        if (n < P) {                                         // append and sift up: a parent below the entry comes down
            i = n++;
            while (i > 0) {
                const int up = (i - 1) >> 1;
                const float2 pe = hp[32 * up];
                if (!pair_less(pe.x, __float_as_int(pe.y), s, c)) break;
                hp[32 * i] = pe;
                i = up;
            }
            hp[32 * i] = entry;
            if (n < P) return;
        } else {                                             // replace the root and sift down: the larger child comes up
            i = 0;
            for (;;) {
                int down = 2 * i + 1;
                if (down >= P) break;
                float2 ce = hp[32 * down];
                if (down + 1 < P) {
                    const float2 other = hp[32 * (down + 1)];
                    if (pair_less(ce.x, __float_as_int(ce.y), other.x, __float_as_int(other.y))) {
                        ce = other;
                        ++down;
                    }
                }
                if (!pair_less(s, c, ce.x, __float_as_int(ce.y))) break;
                hp[32 * i] = ce;
                i = down;
            }
            hp[32 * i] = entry;
        }
        const float2 root = hp[0];
        bs = root.x;
        bi = __float_as_int(root.y);
    };

    for (long tile = lo; tile < hi; ++tile) {
        // the tile's terms.  Buffer tile % 2: a wave that is still in the epilogue of the tile before reads the other one, and
        // the readers of this one passed a barrier since
        float *tw = tt + (tile & 1) * kCsCT;
        if constexpr (METRIC != kMetricIP) {
            if (tid < kCsCT) {
                const long cl = tile * kCsCT + tid;
                tw[tid] = terms[cl < L ? cl : L - 1];
            }
        }
        load(tile, 0);
        store(0);
        __syncthreads();
        coarse_f32x16 acc[kCsBlocks];
#pragma unroll
        for (int ci = 0; ci < kCsBlocks; ++ci)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ci][r] = 0.f;
        for (int c = 0; c < chunks; ++c) {
            if (c + 1 < chunks) load(tile, c + 1);
            const unsigned short *b = stage + (c & 1) * STAGE + 8 * half;
            const unsigned short *qa = b + qi * kCsPitch;
            const unsigned short *pa = b + (3 * QT + frow) * kCsPitch;
            bf16_v8 x[3], y[3][kCsBlocks];                   // [plane: hi, mid, lo](, block)
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                x[p] = *reinterpret_cast<const bf16_v8 *>(qa + QT * p * kCsPitch);
#pragma unroll
                for (int ci = 0; ci < kCsBlocks; ++ci)
                    y[p][ci] = *reinterpret_cast<const bf16_v8 *>(pa + (kCsCT * p + 32 * ci) * kCsPitch);
            }
            // step c of the four blocks, rule 61's order: lo.hi, mid.mid, hi.lo, mid.hi, hi.mid, hi.hi
            constexpr int vp[6] = {2, 1, 0, 1, 0, 0}, cp[6] = {0, 1, 2, 0, 1, 0};
#pragma unroll
            for (int k = 0; k < 6; ++k)
#pragma unroll
                for (int ci = 0; ci < kCsBlocks; ++ci)
                    acc[ci] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(y[cp[k]][ci], x[vp[k]], acc[ci], 0, 0, 0);
            if (c + 1 < chunks) store((c + 1) & 1);
            __syncthreads();
        }
        // the offers of this lane's query, a block of 32 centroids at a time
        const int first = (int)(tile * kCsCT), left = L - first;
#pragma unroll
        for (int ci = 0; ci < kCsBlocks; ++ci) {
            float sc[16];
            unsigned open = 0;                               // bit r: score r is below the register bound
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c0 = 32 * ci + 8 * (r / 4) + 4 * half + (r % 4);
                if constexpr (METRIC == kMetricL2) sc[r] = tw[c0] - acc[ci][r];
                else if constexpr (METRIC == kMetricIP) sc[r] = -acc[ci][r];
                else sc[r] = -(acc[ci][r] * tw[c0]);
                if (qthere && c0 < left && pair_less(sc[r], first + c0, bs, bi)) open |= 1u << r;
            }
            // a round takes one survivor of every lane that has one, each lane its own next (the condition is wave-uniform:
            // every lane is in the round or none)
            while (__ballot(open != 0) != 0) {
                const int r = open ? __builtin_ctz(open) : 0;
                float s = sc[0];
#pragma unroll
                for (int k = 1; k < 16; ++k) s = r == k ? sc[k] : s;
                const int c = open ? first + 32 * ci + 8 * (r >> 2) + 4 * half + (r & 3) : -1;
                open &= open - 1;
                const float os = __shfl_xor(s, 32, 64);      // the partner lane's offer: the lower lane of a query takes both
                const int oc = __shfl_xor(c, 32, 64);
                if (half == 0) {
#pragma unroll 1
                    for (int h = 0; h < 2; ++h) {            // its own first; each meets the bound as it is by then
                        const float cs = h ? os : s;
                        const int cc = h ? oc : c;
                        if (cc >= 0 && pair_less(cs, cc, bs, bi)) push(cs, cc);
                    }
                }
                bs = __shfl(bs, frow, 64);                   // the writer's bound, for both lanes of the query
                bi = __shfl(bi, frow, 64);
            }
        }
    }
    // the part leaves in heap order; what the heap never held is the tail
    if (half == 0)
        for (int e = n; e < P; ++e) hp[32 * e] = make_float2(__builtin_inff(), __int_as_float(kNoIndex));
    coarse_wave_sync();
    const float2 *hw = hp - frow;                            // the wave's region: entry e of its query j at [32 e + j]
    for (int e = lane; e < 32 * P; e += 64) {
        const int j = e / P, p = e % P;
        if (q0 + 32 * wave + j < Q) {
            const long out = ((q0 + 32 * wave + j) * parts + part) * P + p;
            const float2 entry = hw[32 * p + j];
            const int l = __float_as_int(entry.y);
            part_score[out] = entry.x;
            part_list[out] = l == kNoIndex ? -1 : l;
        }
    }
}

}  // namespace mcq
