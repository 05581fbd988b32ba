// mcq_api.hip -- C ABI (include/mcq.h) over the gfx950 kernels of the mcq_*_kernels.h headers below: prepare, encode, decode, the
// trainer's loss and update kernels, search and range search over stored codes.  Host side only: argument checks, launch
// arithmetic, kernel selection; every entry point enqueues on the caller's stream and returns (mcq.h has the contract).
#include "../../include/mcq.h"
#include "../../include/mcq_residual.h"
#include "../../include/mcq_probe.h"
#include "../../include/mcq_wide.h"
#include "../../include/mcq_rerank.h"
#include "../../include/mcq_code16.h"
#include "../../include/mcq_shortlist.h"
#include "../../include/mcq_lanes.h"
#include "mcq_kernels.h"
#include "mcq_fix_kernels.h"
#include "mcq_loss_kernels.h"
#include "mcq_tf_kernels.h"
#include "mcq_pass16_kernels.h"
#include "mcq_train_kernels.h"
#include "mcq_search_kernels.h"
#include "mcq_range_kernels.h"
#include "mcq_wide_kernels.h"
#include "mcq_rerank_kernels.h"
#include "mcq_shortlist_kernels.h"
#include "mcq_lanes.h"

#include <cstdlib>
#include <iterator>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

using namespace mcq;

namespace {

inline int round_up16(int d) { return (d + 15) & ~15; }
inline size_t align256(size_t v) { return (v + 255) & ~size_t(255); }
inline bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// K_cutoff rule of _refine_indexes (quantization/quantization.py:453-463)
int k_cutoff(int K, int L) {
    int kc = (K <= 16) ? 8 : 16;
    while (L >= 4) { L /= 4; kc *= 2; }
    return kc < 128 ? kc : 128;
}

struct Prepared {
    const float *C, *Q, *bias, *scales, *G, *mean, *wmu, *cmean;
    const int8_t *Cf, *Wf;      // limb planes of the scaled centers / of to_logits.weight (mcq_fix_kernels.h)
    const int *Ce, *We;         // their row exponents
};

struct PreparedLayout {
    size_t offC, offQ, offCf, offCe, offWf, offWe, offWmu, offBias, offScales, offMean, offCMean, offG, total;
};

PreparedLayout prepared_layout(int N, int K, int D) {
    const size_t nk = (size_t)N * K, Dp = round_up16(D);
    const size_t planes = fix_plane_bytes((long)nk, D), exps = (size_t)fix_round_rows((long)nk) * 4;
    PreparedLayout l;
    l.offC = 0;
    l.offQ = align256(l.offC + nk * Dp * 4);
    l.offCf = align256(l.offQ + nk * 4);
    l.offCe = align256(l.offCf + planes);
    l.offWf = align256(l.offCe + exps);
    l.offWe = align256(l.offWf + planes);
    l.offWmu = align256(l.offWe + exps);          // fixdot(data mean, W[r]), float[nk] (the logits product reads centered frames)
    l.offBias = align256(l.offWmu + nk * 4);
    l.offScales = align256(l.offBias + nk * 4);   // float[2] {cscale_exp, lscale_exp} (mcq_prepare_dev)
    l.offMean = align256(l.offScales + 8);        // get_data_mean() of the scaled centers, float[Dp]
    l.offCMean = align256(l.offMean + Dp * 4);    // the codebooks' own means mu_n, float[N][Dp] (mean = mu_0 + mu_1 + ...)
    l.offG = align256(l.offCMean + (size_t)N * Dp * 4);   // Gram matrix G[nk][nk] of the CENTERED rows C[n][k] - mu_n
    l.total = align256(l.offG + nk * nk * 4);
    // k_fgemm's epilogue DMA-copies 128 bias floats per row tile without a bound check: rows past N*K of the last tile read what
    // FOLLOWS the bias (scale factors, means, the Gram matrix: finite floats inside this blob; such rows belong to no codebook and
    // their values are never stored).  The layout guarantees those bytes exist:
    static_assert(kFixTile == 128, "");
    if (l.total < l.offBias + (nk + kFixTile) * 4) l.total = align256(l.offBias + (nk + kFixTile) * 4);
    return l;
}

Prepared prepared_view(const void *p, int N, int K, int D) {
    const PreparedLayout l = prepared_layout(N, K, D);
    const char *b = static_cast<const char *>(p);
    auto f = [b](size_t off) { return reinterpret_cast<const float *>(b + off); };
    return Prepared{f(l.offC), f(l.offQ), f(l.offBias), f(l.offScales), f(l.offG), f(l.offMean), f(l.offWmu), f(l.offCMean),
                    reinterpret_cast<const int8_t *>(b + l.offCf), reinterpret_cast<const int8_t *>(b + l.offWf),
                    reinterpret_cast<const int *>(b + l.offCe), reinterpret_cast<const int *>(b + l.offWe)};
}

template <typename T>
T *writable(const T *p) { return const_cast<T *>(p); }      // mcq_prepare* fill the blob through the view its readers use

// CT: how a codebook entry is held (mcq_tf_kernels.h: one byte up to 256 entries per codebook, two above)
template <typename CT>
struct WorkspaceT {
    CT *idx, *idxB, *idxC, *final_idx;        // B, C: fixed-point skipping only; final_idx: spare (the workspace size is ABI)
    int *map[2], *cnt;
    float *E, *R, *xx, *XC;                   // per vector: |x_err|^2, |x_err - old_n|^2, |x|^2, x.C products
    float *gterms;                            // per vector: the N*N Gram entries G[o_m][o_m2] of the current indexes
    int8_t *xf;                               // limb planes of the CENTERED frames of a chunk (x - mean: both products read them)
    int *xe;                                  // and their row exponents
    float *tabs[2];                           // group tables of two consecutive levels (ping-pong)
    TfLists tf;                               // candidate lists of every level
};

int tf_levels(int N) { int v = 0; while ((1 << v) < N) ++v; return v; }   // lists exist at levels 0 .. tf_levels(N) - 1

// floats of the largest set of group tables any combine needs at one level (per vector)
size_t tf_tab_floats(int N, int K) {
    const int nlev = tf_levels(N);
    size_t best = 0;
    for (int v = 2; v < nlev; ++v) {
        const size_t groups = (size_t)N >> (v + 1);
        for (int u = 1; u < v; ++u) {
            const size_t per = (size_t)1 << (v - u), kc = k_cutoff(K, 1 << u);
            const size_t f = groups * per * per * kc * kc;
            best = f > best ? f : best;
        }
    }
    return best;
}

inline size_t code_bytes_of(int K) { return K > 256 ? 2 : 1; }

size_t workspace_per_vector(int N, int K, int D) {
    // idx x4, maps, E, xx, R, XC, lists (entries / positions / scores: <= 16 cb + 2*16 + 4*16 bytes per codebook and level), tabs x2,
    // the frame as limb planes + its exponent, the N*N Gram terms of E / R
    const size_t cb = code_bytes_of(K);
    return 4 * cb * (size_t)N + 8 + 8 + 4 * (size_t)N + 4 * (size_t)N * K + (size_t)tf_levels(N) * N * (16 * cb + 2 * 16 + 4 * 16) + 64 +
           2 * 4 * tf_tab_floats(N, K) + 4 * (size_t)fix_round_cols(D) + 4 + 4 * (size_t)N * N;
}
// what one lane's share holds besides its vectors: alignment of the carved arrays + the rows the limb planes are padded by (to a
// multiple of 128); and what the whole workspace does (mcq_lanes.h: two such shares, a spare vector, the second share's alignment)
size_t lane_slack(int D) { return 48 * 256 + (size_t)kFixTile * (4 * (size_t)fix_round_cols(D) + 4); }
size_t workspace_slack(int N, int K, int D) { return plan_slack(workspace_per_vector(N, K, D), lane_slack(D)); }

// default chunk: 65,536 vectors, fewer when a vector's share of the workspace is large (N >= 32), so that the workspace
// mcq_encode_workspace_bytes asks for stays near 2 GB
long default_chunk(int N, int K, int D) {
    long c = (long)(((size_t)2 << 30) / workspace_per_vector(N, K, D));
    c = c > 65536 ? 65536 : c;
    c = c < 1024 ? 1024 : c;
    return c & ~127L;
}

// The arrays carve() lays out, by number (mcq_test_pass_layout of include/mcq_probe.h reports them under these numbers; in
// memory a level's positions and scores lie together).  A level has its slots whether it holds a list or not
enum { CV_IDX = 0, CV_IDXB, CV_IDXC, CV_FINAL_IDX, CV_MAP0, CV_MAP1, CV_CNT, CV_E, CV_R, CV_XX, CV_GTERMS, CV_XC, CV_XF, CV_XE,
       CV_ENT, CV_POS1, CV_S0 = CV_POS1 + kTfLevels - 1, CV_TABS0 = CV_S0 + kTfLevels, CV_TABS1, CV_COUNT };
struct CarveExtents {
    size_t off[CV_COUNT] = {}, bytes[CV_COUNT] = {};      // (an array carve did not lay out: 0, 0)
    size_t total = 0;
};

// ext: where every array lies, for the probe (carve is the only place that knows)
template <typename CT>
WorkspaceT<CT> carve(void *ws, long Bc, int N, int K, int D, CarveExtents *ext = nullptr) {
    char *p = static_cast<char *>(ws);
    size_t off = 0;
    auto take = [&](int what, size_t bytes) {
        if (ext) { ext->off[what] = off; ext->bytes[what] = bytes; }
        char *q = p + off;
        off = align256(off + bytes);
        return q;
    };
    WorkspaceT<CT> w;
    w.idx = reinterpret_cast<CT *>(take(CV_IDX, (size_t)Bc * N * sizeof(CT)));
    w.idxB = reinterpret_cast<CT *>(take(CV_IDXB, (size_t)Bc * N * sizeof(CT)));
    w.idxC = reinterpret_cast<CT *>(take(CV_IDXC, (size_t)Bc * N * sizeof(CT)));
    w.final_idx = reinterpret_cast<CT *>(take(CV_FINAL_IDX, (size_t)Bc * N * sizeof(CT)));
    for (int i = 0; i < 2; ++i) w.map[i] = reinterpret_cast<int *>(take(CV_MAP0 + i, (size_t)Bc * 4));
    w.cnt = reinterpret_cast<int *>(take(CV_CNT, 64 * 4));
    w.E = reinterpret_cast<float *>(take(CV_E, (size_t)Bc * 4));
    w.R = reinterpret_cast<float *>(take(CV_R, (size_t)Bc * N * 4));
    w.xx = reinterpret_cast<float *>(take(CV_XX, (size_t)Bc * 4));
    w.gterms = reinterpret_cast<float *>(take(CV_GTERMS, (size_t)Bc * N * N * 4));
    w.XC = reinterpret_cast<float *>(take(CV_XC, (size_t)Bc * N * K * 4));
    w.xf = reinterpret_cast<int8_t *>(take(CV_XF, fix_plane_bytes(Bc, D)));
    w.xe = reinterpret_cast<int *>(take(CV_XE, (size_t)fix_round_rows(Bc) * 4));
    const int nlev = tf_levels(N);
    w.tf.ent = nullptr;
    w.tf.out_i64 = nullptr;
    w.tf.out_u8 = nullptr;
    w.tf.out_pack = 1;
    w.tf.map = nullptr;
    w.tf.erG = w.tf.erXC = w.tf.erxx = nullptr;
    w.tf.erE = w.tf.erR = nullptr;
    w.tf.erK = 0;
    for (int v = 0; v < kTfLevels; ++v) {
        w.tf.kc[v] = k_cutoff(K, 1 << v);
        w.tf.pos[v] = nullptr;
        w.tf.S[v] = nullptr;
        if (v >= nlev) continue;                       // no list of that level
        const int kc = w.tf.kc[v];
        if (v == 0) w.tf.ent = reinterpret_cast<uint8_t *>(take(CV_ENT, (size_t)Bc * N * kc * sizeof(CT)));
        else w.tf.pos[v] = reinterpret_cast<uint8_t *>(take(CV_POS1 + v - 1, (size_t)Bc * (N >> v) * kc * 2));
        w.tf.S[v] = reinterpret_cast<float *>(take(CV_S0 + v, (size_t)Bc * (N >> v) * kc * 4));
    }
    const size_t tf = tf_tab_floats(N, K);
    for (int i = 0; i < 2; ++i) w.tabs[i] = tf ? reinterpret_cast<float *>(take(CV_TABS0 + i, (size_t)Bc * tf * 4)) : nullptr;
    if (ext) ext->total = off;
    return w;
}

// up to 64 codebooks (QuantizerTrainer produces at most 64 x 16 and 32 x 256: bytes_per_frame <= 32); codebooks of 512 and 1,024
// entries (Quantizer(codebook_size = ...) used with as_bytes = False) as long as the Gram matrix stays within 16,384 rows (1 GB)
constexpr int kMaxRows = 16384;
bool domain_ok(int N, int K, int D) {
    return is_pow2(K) && K >= 16 && K <= 1024 && is_pow2(N) && N <= 64 && (long)N * K <= kMaxRows && D >= 1 && D <= 16384;
}
int domain_err(int N, int K, int D = 1) {
    return (K < 16 || K > 1024 || N > 64 || (long)N * K > kMaxRows || D > 16384) ? MCQ_EUNSUPPORTED : MCQ_EINVAL;
}

// optional per-launch timing (mcq_profile_encode)
struct Prof {
    hipStream_t stream;
    int only = -1;                            // the one category this encode times (-1: all)
    std::vector<hipEvent_t> ev;
    std::vector<int> cat, first, last;        // interval i: events first[i] .. last[i]
    int open = -1;
    // An event pair round EVERY launch keeps the launches from overlapping their predecessor's tail (the profiled encode took
    // 9-11 % longer than the timed one), so mcq_profile_encode runs one encode per category and times only that category's
    // launches in it; two timed launches that follow each other share the event between them.
    void begin(int category) {
        if (only >= 0 && category != only) { open = -1; return; }      // (a launch that is not timed separates two that are)
        if (ev.empty() || open != (int)ev.size() - 1) {
            hipEvent_t e;
            (void)hipEventCreate(&e);
            (void)hipEventRecord(e, stream);
            ev.push_back(e);
        }
        open = (int)ev.size() - 1;
    }
    void untimed() { open = -1; }             // something was enqueued outside every category: the next interval takes a fresh event
    void end(int category) {
        if (only >= 0 && category != only) { open = -1; return; }
        hipEvent_t e;
        (void)hipEventCreate(&e);
        (void)hipEventRecord(e, stream);
        ev.push_back(e);
        first.push_back(open);
        last.push_back((int)ev.size() - 1);
        cat.push_back(category);
        open = (int)ev.size() - 1;
    }
};

thread_local int g_last_launches = 0;
thread_local int g_last_lanes = 0;       // streams the last encode of this thread enqueued on (mcq_last_encode_lanes)

#define MCQ_LAUNCH_CHECK()                               \
    do {                                                 \
        hipError_t e_ = hipGetLastError();               \
        if (e_ != hipSuccess) return (int)e_;            \
        ++g_last_launches;                               \
    } while (0)

// what a launch left behind, as the entry points return it: uncounted, and counted as MCQ_LAUNCH_CHECK counts
inline int launch_rc() {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
inline int counted_launch_rc() { MCQ_LAUNCH_CHECK(); return 0; }

// A kernel that spends `threads_per_row` threads on a row is launched over B rows in pieces of at most kPieceRows * 64 /
// threads_per_row rows, 2^31 threads each: launch(first row, rows) -> rc.  A grid of 2^32 threads or more is not refused by
// the runtime here; it returns hipSuccess and runs the thread count modulo 2^32, so the rows past it keep what the output held
// ("Stores past 2^26 rows").  B within one piece is exactly one launch with the geometry it always had.
template <typename F>
int launch_in_pieces(long B, int threads_per_row, F &&launch) {
    const long piece = (long)kPieceRows * 64 / (threads_per_row > 64 ? threads_per_row : 64);
    for (long at = 0; at < B; at += piece)
        if (const int rc = launch(at, B - at < piece ? B - at : piece)) return rc;
    return 0;
}

// Kernel selection: a runtime value becomes a template argument ("Kernel selection").  pick<Vs...>(v, f) calls
// f(std::integral_constant<int, V>{}) for the V that equals v and returns what f returns; no V equals v: MCQ_EUNSUPPORTED.  The
// list IS the set of instantiations: f is stamped for every V, so a case belongs in it only if the host can reach it.
template <int... Vs, typename F>
int pick(int v, F &&f) {
    int rc = MCQ_EUNSUPPORTED;
    (void)((v == Vs && ((rc = f(std::integral_constant<int, Vs>{})), true)) || ...);
    return rc;
}
template <typename F>
int pick_bool(bool b, F &&f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

// The same over the rows of a constexpr table of pairs (a list of pairs, not the product of two lists): f(A, B) for the row
// {A, B} that equals {a, b}.  A predicate that asks "is there a kernel for (a, b)" reads the same table (in_pairs).
struct Pair { int a, b; };
template <const auto &Table, typename F, size_t... I>
int pick_pair(int a, int b, F &&f, std::index_sequence<I...>) {
    int rc = MCQ_EUNSUPPORTED;
    (void)((a == Table[I].a && b == Table[I].b &&
            ((rc = f(std::integral_constant<int, Table[I].a>{}, std::integral_constant<int, Table[I].b>{})), true)) || ...);
    return rc;
}
template <const auto &Table, typename F>
int pick_pair(int a, int b, F &&f) { return pick_pair<Table>(a, b, f, std::make_index_sequence<std::size(Table)>{}); }
template <size_t R>
bool in_pairs(const Pair (&table)[R], int a, int b) {
    for (const Pair &p : table) if (p.a == a && p.b == b) return true;
    return false;
}

// Allow `kernel` up to `bytes` of dynamic LDS, once per device (a process may drive several).  `allowed` is the calling
// launcher's static flag array: one per kernel instantiation.
int allow_dynamic_lds(bool (&allowed)[64], const void *kernel, int bytes) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 63;
    if (!allowed[dev] || dev == 63) {
        const hipError_t attr = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (attr != hipSuccess) return (int)attr;
        allowed[dev] = true;
    }
    return 0;
}

// What the encode keeps per device, made once under the record's mutex: the side stream and the fork / join events of the
// second lane (run_encode_t), and the LDS opt-ins of the LDS-resident pass (launch_pass16).  A device the runtime does not name
// (or one past the table) has no record: no second lane there, and the opt-ins are repeated on every call.
struct DeviceRec {
    std::mutex mu;                  // guards the lane fields; held over the two-lane section of an encode (fork .. join)
    bool lanes_tried = false, lanes_ok = false;
    hipStream_t side = nullptr;     // lane 1
    hipEvent_t fork = nullptr, join = nullptr;
    std::mutex lds_mu;              // guards the opt-in flags (taken inside the two-lane section: a mutex of its own)
    bool pass16_ok = false, pass16_probe_ok = false;
};
DeviceRec g_device[64];
DeviceRec *device_rec() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return (dev >= 0 && dev < 64) ? &g_device[dev] : nullptr;
}

// r.mu held.  The side stream does not synchronise with the null stream (the events order it) and the events carry no
// timestamps.  A failure is remembered (not retried on every call) and leaves no error behind: the encode runs on one lane
bool lanes_ready(DeviceRec &r) {
    if (r.lanes_tried) return r.lanes_ok;
    r.lanes_tried = true;
    if (hipStreamCreateWithFlags(&r.side, hipStreamNonBlocking) == hipSuccess &&
        hipEventCreateWithFlags(&r.fork, hipEventDisableTiming) == hipSuccess &&
        hipEventCreateWithFlags(&r.join, hipEventDisableTiming) == hipSuccess) {
        r.lanes_ok = true;
        return true;
    }
    (void)hipGetLastError();
    if (r.join) (void)hipEventDestroy(r.join);
    if (r.fork) (void)hipEventDestroy(r.fork);
    if (r.side) (void)hipStreamDestroy(r.side);
    r.side = nullptr; r.fork = r.join = nullptr;
    (void)hipGetLastError();
    return false;
}

// The launches of its scope as one interval of category `cat` of the profiler, if there is one: `{ Timed t(prof, CAT); launch }`
struct Timed {
    Prof *const prof;
    const int cat;
    Timed(Prof *p, int c) : prof(p), cat(c) { if (prof) prof->begin(cat); }
    ~Timed() { if (prof) prof->end(cat); }
    Timed(const Timed &) = delete;
};

// rows -> limb planes + exponents (+ |row|^2): the operands of every product of the path
FixRowsArgs fix_rows_args(const float *src, int xh, long R, int D, long ld, int8_t *planes, int *exps, float *xx,
                          const float *bias_src = nullptr, float *bias_dst = nullptr, const float *sub = nullptr,
                          long sub_per = 0, long sub_ld = 0, const float *dot_vec = nullptr, float *dot_out = nullptr) {
    return FixRowsArgs{src, xh, R, fix_round_rows(R), D, ld, fix_round_cols(D), planes, exps, xx, bias_src, bias_dst,
                       sub, sub_per, sub_ld, dot_vec, dot_out, nullptr};
}

// sub != nullptr: the rows are centered by sub[0 .. D) (the frames of the search and of the logits: x - mean)
int launch_fix_rows(const float *src, int xh, long R, int D, long ld, int8_t *planes, int *exps, float *xx, hipStream_t st,
                    const float *sub = nullptr, unsigned *clear = nullptr) {
    FixRowsArgs a = fix_rows_args(src, xh, R, D, ld, planes, exps, xx, nullptr, nullptr, sub, 0, 0);
    a.clear = clear;
    // four rows per workgroup, one per wave (16 rows per workgroup and 256-byte runs into the planes measured slower:
    // 0.086 vs 0.071 ms at 65,536 x 512)
    hipLaunchKernelGGL(k_fix_rows<4>, dim3((unsigned)(a.Rp / 4)), dim3(256), 0, st, a);
    return counted_launch_rc();
}

int launch_fix_rows2(const FixRowsArgs &a, const FixRowsArgs &b, hipStream_t st) {
    const unsigned na = (unsigned)(a.Rp / 4), nb = (unsigned)(b.Rp / 4);
    hipLaunchKernelGGL(k_fix_rows2<4>, dim3(na + nb), dim3(256), 0, st, a, b, na);
    return counted_launch_rc();
}

// the fixed-point GEMM: persistent workgroups of eight waves, one per CU
template <int MODE>
int launch_fgemm(FixGemm g, hipStream_t st) {
    static bool allowed[64] = {};                      // (the kernel's 132 KB of dynamic LDS)
    constexpr int lds = MODE == FG_SCREEN ? kFixLdsScreen : kFixLds;
    if (const int rc = allow_dynamic_lds(allowed, reinterpret_cast<const void *>(&k_fgemm<MODE>), lds)) return rc;
    const long MT = g.RA / kFixTile, NT = g.RB / kFixTile;
    const int H = (MODE != FG_STORE && g.K > kFixTile) ? g.K / kFixTile : 1;
    const long big = g.walk_rows ? NT : MT, small_units = (g.walk_rows ? MT : NT) / H;
    long units = (big + 7) / 8 * small_units;          // per XCD
    if (units > 32) units = 32;                        // 32 CUs per XCD, one workgroup each
    hipLaunchKernelGGL((k_fgemm<MODE>), dim3((unsigned)(8 * units)), dim3(512), lds, st, g);
    return counted_launch_rc();
}

// XC[b][r] = fixdot(x_b, C_r) (or the Gram matrix with the centers as "frames"): frames stream, the centers are the table.
// (The other arrangement -- centers as the tile rows, four consecutive centers of a frame as one 16-byte store, as the
// logits are laid out -- measured 0.600 against 0.581 ms with eight waves; with four it was the faster one, 0.712 / 0.746.)
int launch_xc(const int8_t *xf, const int *xe, long B, const int8_t *Cf, const int *Ce, long nk, int D, float *out,
              hipStream_t st) {
    FixGemm g{};
    g.A = xf; g.ea = xe; g.RA = fix_round_rows(B); g.M = B;
    g.B = Cf; g.eb = Ce; g.RB = fix_round_rows(nk); g.N = nk;
    g.Dq = fix_round_cols(D);
    g.walk_rows = 0;
    g.out = out; g.ldo = nk;
    return launch_fgemm<FG_STORE>(g, st);
}

// MCQ_EXACT_LOGITS=1: the initial codes from the full ten-product kernel (same-box A/B of the screened path; identical results)
inline bool exact_logits_forced() {
    static const bool on = getenv("MCQ_EXACT_LOGITS") && atoi(getenv("MCQ_EXACT_LOGITS")) != 0;
    return on;
}

// logits[b][r] = fixdot(x_b, W_r) * lscale + bias[r] (stored when logits != nullptr) and the arg max per codebook.
// und_cnt != nullptr (arg max only): six limb products decide the winner where they can (k_fgemm<FG_SCREEN>), the pairs they
// cannot decide are listed in und_list (room for B * N entries of two words; *und_cnt is zero on entry) and redone exactly by k_fscreen_recheck
int launch_logits(const int8_t *xf, const int *xe, long B, const Prepared &P, int N, int K, int D, float lscale,
                  const float *lscale_ptr, float *logits, void *idx, hipStream_t st, unsigned *und_cnt = nullptr,
                  unsigned *und_list = nullptr) {
    const long nk = (long)N * K;
    FixGemm g{};
    g.A = P.Wf; g.ea = P.We; g.RA = fix_round_rows(nk); g.M = nk;
    g.B = xf; g.eb = xe; g.RB = fix_round_rows(B); g.N = B;
    g.Dq = fix_round_cols(D);
    g.walk_rows = 1;
    g.bias = P.bias; g.wmu = P.wmu; g.lscale = lscale; g.lscale_ptr = lscale_ptr;
    g.logits = logits; g.ldo = nk; g.idx = idx; g.idx_wide = K > 256 ? 1 : 0; g.K = K; g.ncb = N;
    if (und_cnt == nullptr) return launch_fgemm<FG_LOGITS>(g, st);
    if (logits != nullptr) return MCQ_EINVAL;
    g.und_cnt = und_cnt; g.und_list = und_list; g.und_cap = (unsigned)(B * N);
    const int rc = launch_fgemm<FG_SCREEN>(g, st);
    if (rc) return rc;
    FixRecheck r{};
    r.W = P.Wf; r.X = xf; r.ew = P.We; r.ex = xe; r.RW = g.RA; r.RX = g.RB; r.Dq = g.Dq;
    r.bias = P.bias; r.wmu = P.wmu; r.lscale_ptr = lscale_ptr; r.lscale = lscale;
    r.idx = idx; r.idx_wide = g.idx_wide; r.K = K; r.ncb = N; r.cnt = und_cnt; r.list = und_list; r.cap = g.und_cap;
    const long waves = B * N;          // a wave per pair at most, 4,096 waves (16 per CU) striding over the list at the most
    hipLaunchKernelGGL(k_fscreen_recheck, dim3((unsigned)(waves < 4096 ? (waves + 3) / 4 : 1024)), dim3(256), 0, st, r);
    return counted_launch_rc();
}

// ---------------------------------------------------------------- the refinement pass
// Grid of a pass kernel: the full grid, or at most `cap` workgroups (a multiple of 8) that stride over the virtual workgroups of
// the active vectors (capped: later passes of fixed-point skipping, where most workgroups of the full grid would find no vector
// and still cost their dispatch, about 0.2 ns each)
constexpr unsigned kCapStage0 = 32768, kCapWave = 65536;     // workgroups of four waves / of one wave
// MCQ_PASS_CAP_STAGE0=<n> / MCQ_PASS_CAP_WAVE=<n> move the caps (read per call, rounded down to a multiple of 8, at least 8): the
// tests make a workgroup loop many times over a few dozen vectors with them, the A/B runs try other caps
inline unsigned pass_cap(const char *name, unsigned dflt) {
    const char *v = getenv(name);
    if (!v) return dflt;
    const long n = atol(v);
    return n < 8 ? 8u : n > 0x7ffffff8L ? 0x7ffffff8u : (unsigned)n & ~7u;
}
inline unsigned cap_stage0() { return pass_cap("MCQ_PASS_CAP_STAGE0", kCapStage0); }
inline unsigned cap_wave() { return pass_cap("MCQ_PASS_CAP_WAVE", kCapWave); }
// The looping (STRIDED) form of a kernel only where the grid IS capped: a capped pass whose full grid fits under the cap takes the
// dense form, whose workgroups past the active vectors return at once (full == cap used to run the loop for one iteration each)
inline bool pass_strided(unsigned full, bool capped, unsigned cap) { return capped && full > cap; }
inline unsigned pass_grid(unsigned full, bool capped, unsigned cap) { return pass_strided(full, capped, cap) ? cap : full; }

// Stage 0 of a pass.  Four or more 16-entry codebooks: four codebooks per wave, rank-in-row selection (k_tf_stage0_k16: its lists
// of kc[0] == 8 fit a row, so k_tf_stage0<16, N> exists for N <= 2 only).  No shape past kMaxRows rows is stamped either.
template <typename CT>
int launch_tf_stage0(int K, int N, const float *G, const float *XC, const CT *idx, const float *R, const float *Q, long B, int keep,
                     CT *ent, float *S, CT *fin, const int *nact, const int *map, hipStream_t st, bool capped) {
    const unsigned vgrid = (unsigned)(((B + 3) / 4) * N);
    const unsigned cap = cap_stage0();
    const dim3 grid(pass_grid(vgrid, capped, cap)), block(256);
    auto with_k = [&](auto kk) {
        constexpr int KK = kk;
        return pick<1, 2, 4, 8, 16, 32, 64>(N, [&](auto nn) {
            constexpr int NN = nn;
            if constexpr ((KK == 16 && NN >= 4) || KK * NN > kMaxRows) return MCQ_EUNSUPPORTED;
            else return pick_bool(pass_strided(vgrid, capped, cap), [&](auto strided) {
                constexpr bool STRIDED = strided;
                hipLaunchKernelGGL((k_tf_stage0<KK, NN, STRIDED>), grid, block, 0, st, G, XC, idx, R, Q, B, keep, ent, S, fin, nact, map, vgrid);
                return counted_launch_rc();
            });
        });
    };
    if constexpr (sizeof(CT) == 1) {
        if (K == 16 && N >= 4) {
            const dim3 grid16((unsigned)((B * (N / 4) + 3) / 4));
            return pick<4, 8, 16, 32, 64>(N, [&](auto nn) {
                constexpr int NN = nn;
                hipLaunchKernelGGL((k_tf_stage0_k16<NN>), grid16, block, 0, st, G, XC, idx, R, Q, B, keep, ent, S, nact, map);
                return counted_launch_rc();
            });
        }
        return pick<16, 32, 64, 128, 256>(K, with_k);
    } else {
        return pick<512, 1024>(K, with_k);
    }
}

// E / R of a pass's vectors; a codebook entry of two bytes means K >= 512, so no more than kMaxRows / 512 codebooks.
// Up to 8,192 vectors: one launch that gathers the Gram entries itself.  Above: two launches, the Gram terms XCD by XCD and
// then the sums; 4, 8 and 16 codebooks of one-byte entries take the dense form of the pair (mcq_tf_kernels.h: a lane per
// vector / per (vector, column), the unordered pairs only), the other shapes a wave per request.  `stride`: the vectors the
// Gram-terms buffer was carved for
template <typename CT>
int launch_tf_er(int N, const float *G, const float *XC, const CT *idx, const float *xx, long B, int K, float *E, float *R,
                 float *gterms, long stride, const int *nact, const int *map, hipStream_t st, int form = -1) {
    const dim3 grid((unsigned)((B + 3) / 4)), block(256);
    // one launch instead of two (E / R of a trainer batch: 4.9 + 4.7 -> about 5 us); form 0 / 1: mcq_test_er asks for one of them
    const bool direct = form < 0 ? B <= 8192 : form == 0;
    return pick<1, 2, 4, 8, 16, 32, 64>(N, [&](auto nn) {
        constexpr int NN = nn, VG = 4 * (64 / NN);      // vectors per workgroup of k_tf_gram_terms, and of the dense k_tf_er
        if constexpr (sizeof(CT) == 2 && NN * 512 > kMaxRows) return MCQ_EUNSUPPORTED;
        else {
            constexpr bool DENSE = sizeof(CT) == 1 && (NN == 4 || NN == 8 || NN == 16);
            if (!direct) {
                const long per = DENSE ? 256 : VG;          // vectors per workgroup of k_tf_gram_terms (dense: a lane each)
                hipLaunchKernelGGL((k_tf_gram_terms<NN, CT, DENSE>), dim3((unsigned)(((B + per - 1) / per) * NN)), block, 0, st, G, idx, B, K,
                                   gterms, nact, stride);
                if (const int rc = counted_launch_rc()) return rc;
                if constexpr (DENSE) {
                    hipLaunchKernelGGL((k_tf_er<NN, CT, true>), dim3((unsigned)((B + VG - 1) / VG)), block, 0, st, gterms, XC, idx, xx, B, K,
                                       E, R, nact, map, static_cast<const float *>(nullptr), stride);
                    return counted_launch_rc();
                }
            }
            hipLaunchKernelGGL((k_tf_er<NN, CT>), grid, block, 0, st, gterms, XC, idx, xx, B, K, E, R, nact, map,
                               direct ? G : static_cast<const float *>(nullptr), stride);
            return counted_launch_rc();
        }
    });
}

// The (kh, kc) list lengths of two consecutive levels >= 1: K >= 32 holds lists of 16, 16, 32, 32, 64, 64 candidates, K == 16
// lists of 8, 8, 16, 16, 32, 32 (one-byte entries only)
constexpr Pair kTfUpLists[] = {{16, 32}, {32, 32}, {32, 64}, {8, 16}, {16, 16}};
constexpr Pair kTfCombLists[] = {{16, 32}, {32, 32}, {32, 64}, {64, 64}, {8, 16}, {16, 16}};

// Which combines run_tf_combines asks for (DESIGN.md section 4 has the table).  Level v combines lists of (kc[v - 1], kc[v]) and
// is the last one of 2^(v + 1) codebooks, but level 3 of 16 codebooks is k_tf_comb3's: lists of equal lengths (level 3, and
// level 5 of 64 x 16 with (32, 32)) are never the last combine otherwise.  (32, 64) is level 4 (32 codebooks: last; 64: not),
// (64, 64) level 5 (64 codebooks: last).  Two-byte entries (K >= 512) stop at 32 codebooks, lists of 8 are one-byte entries'.
// k_tf_comb<64, 64, false, uint8_t> is never asked for either, and stays: without it the compiler emits other code for its
// two LAST siblings
template <typename CT>
constexpr bool tf_comb_reached(int kh, int kc, bool last) {
    const bool wide = sizeof(CT) == 2;
    if (kh == 8 || kc == 16) return !wide && !(kh == kc && last);
    if (kh == 64) return !wide;
    if (kh == kc) return !(last && wide);
    return !(kc == 64 && wide && !last);
}

// group tables of level u >= 2 from those of level u - 1 (list lengths kh -> kc)
int launch_tf_up(int kh, int kc, const TfLists &L, long B, int N, int u, int ntab, int per, const float *in, float *out,
                 const int *nact, hipStream_t st) {
    return pick_pair<kTfUpLists>(kh, kc, [&](auto a, auto c) {
        constexpr int KH = a, KC = c;
        hipLaunchKernelGGL((k_tf_up<KH, KC>), dim3((unsigned)(B * ntab)), dim3(64), 0, st, L, B, N, u, ntab, per, in, out, nact);
        return counted_launch_rc();
    });
}

// combine of the siblings of level v >= 2 (list lengths kh at level v - 1, kc at level v); fin: the last combine
template <typename CT>
int launch_tf_comb(int kh, int kc, const float *E, const TfLists &L, long B, int N, int v, int keep, const float *tabs,
                   CT *fin, const int *nact, hipStream_t st, bool capped) {
    // (capped: the last combine only; the others of more than 8 codebooks keep their full grid)
    if (fin == nullptr) capped = false;
    const unsigned full = (unsigned)(B * (N >> (v + 1))), cap = cap_wave();
    const dim3 grid(pass_grid(full, capped, cap)), block(64);
    return pick_pair<kTfCombLists>(kh, kc, [&](auto a, auto c) {
        return pick_bool(fin != nullptr, [&](auto last) {
            constexpr int KH = decltype(a)::value, KC = decltype(c)::value;
            constexpr bool LAST = last;
            if constexpr (!tf_comb_reached<CT>(KH, KC, LAST)) return MCQ_EUNSUPPORTED;
            else return pick_bool(pass_strided(full, capped, cap), [&](auto strided) {
                constexpr bool STRIDED = strided;
                if constexpr (STRIDED && !LAST) return MCQ_EUNSUPPORTED;      // (not reached: capped only with fin)
                else {
                    hipLaunchKernelGGL((k_tf_comb<KH, KC, LAST, CT, STRIDED>), grid, block, 0, st, E, L, B, N, v, keep, tabs, fin, nact);
                    return counted_launch_rc();
                }
            });
        });
    });
}

// profiling categories (mcq_profile_encode): one per KIND OF LAUNCH of the shipped sequence -- the profiler records events round
// the launches an encode makes and changes none of them
enum { CAT_LOGITS = 0, CAT_XX = 1, CAT_STAGE0 = 2, CAT_XC = 3, CAT_LEVEL0 = 4, CAT_LEVEL1 = 5, CAT_TABLES = 6, CAT_COMBINE = 7,
       CAT_TABLES_UP = 8, CAT_COMBINE_UP = 9, CAT_ER = 10, CAT_LEVEL1_FUSED = 11, CAT_TAIL = 12, CAT_COUNT = 13 };
const char *const kCatNames[CAT_COUNT] = {
    "logits_product_argmax",      // k_fgemm<FG_LOGITS>, or k_fgemm<FG_SCREEN> + k_fscreen_recheck
    "frames_to_limbs",            // k_fix_rows
    "stage0_tables",              // k_tf_stage0 / k_tf_stage0_k16
    "xc_product",                 // k_fgemm<FG_STORE>
    "combine_level0",             // k_tf_pair0
    "combine_level1",             // k_tf_pair1 (4 codebooks: the last combine; 8 and 16 codebooks in chunks of lazy_tables_min() and more)
    "tables_level1",              // k_tf_table1 after k_tf_pair1: the masked cousin tables of level 2 (8 codebooks; 16: tables_upper_levels)
    "combine_level2",             // k_tf_comb at level 2 (8 codebooks: the last combine, which also forms E / R of the next pass)
    "tables_upper_levels",        // k_tf_table1 / k_tf_up above level 2
    "combine_upper_levels",       // k_tf_comb / k_tf_comb3 above level 2
    "residual_energies",          // k_tf_gram_terms + k_tf_er (first pass; later passes: inside the last combine, or the dense pair again)
    "level1_combines_and_tables", // k_tf_level1: the level-1 combines and the cousin tables of level 2 in one launch
    "encode_tail",                // k_finalize / k_import_indexes / k_compact
};

// The list length of levels 0 and 1 as a template argument: 8 for 16-entry codebooks, else 16.  The kernels over lists of 8
// exist for one-byte entries only
template <typename CT, typename F>
int pick_leaf_lists(int K, F &&f) {
    if constexpr (sizeof(CT) == 1) return pick<8, 16>(K == 16 ? 8 : 16, f);
    else return pick<16>(16, f);
}
// MCQ_PASS16=0: the separate kernels for 16 x 16 codebooks as well (same-box A/B of the LDS-resident pass; identical results)
inline bool pass16_enabled() {
    static const bool on = !(getenv("MCQ_PASS16") && atoi(getenv("MCQ_PASS16")) == 0);
    return on;
}
// fixed-point skipping applies to chunks of at least this many vectors; MCQ_SKIP_MIN_BATCH=<n> moves the threshold (read per
// call: tools/exp_skip_trained.py measures the crossover, the tests run the skipping path on small batches)
inline long skip_min_batch() {
    const char *v = getenv("MCQ_SKIP_MIN_BATCH");
    return v ? atol(v) : 8192;      // (4,096 vectors: 0.472 ms with compaction, 0.477 without; 8,192: 0.773 / 0.800)
}
// chunks of at least this many vectors of 4, 8 or 16 codebooks form E / R of EVERY pass with the dense pair of launch_tf_er
// instead of in the emitting wave of the pass before; MCQ_ER_DENSE_MIN=<n> moves the threshold (read per call; 0: any chunk --
// up to 8,192 vectors the pair is the one direct launch --, a huge value: none)
// (unprofiled bench pairs, 8 x 256, dim 512: 16,384 vectors 1.311 against 1.332 ms, 32,768 2.361 against 2.415, ranges apart;
// at 8,192 the pair is the one direct launch, 10.5 us a pass against the 6 us the emit costs there: profiles/r24_ab_er_dense.txt)
constexpr long kErDenseMin = 16384;
inline long er_dense_min() {
    const char *v = getenv("MCQ_ER_DENSE_MIN");
    return v ? atol(v) : kErDenseMin;
}
// chunks of at least this many vectors of 8 or 16 codebooks of 32 entries or more (one-byte entries) build their cousin tables
// AFTER the level-1 combines and only where the level-2 lists look (tf_table1, USED2): k_tf_pair1, then the masked k_tf_table1,
// instead of the one k_tf_level1 launch.  MCQ_LAZY_TABLES_MIN=<n> moves the threshold (read per call; 0: any chunk, a huge value:
// none).  Above 4,096, so that the launches tests/test_gpu_launch_census.py pins at 256 vectors stay what they are
// (unprofiled bench pairs, 8 x 256, dim 512, three each, this sequence against the one launch: 4,096 vectors 0.463-0.465 against
// 0.449-0.454 ms -- the extra boundary loses --, 8,192 0.766-0.767 against 0.764-0.769, overlap, 16,384 1.314-1.324 against
// 1.335-1.341 and 32,768 2.399-2.406 against 2.464-2.469, ranges apart: profiles/r26_ab_lazy_tables.txt)
constexpr long kLazyTablesMin = 16384;
inline long lazy_tables_min() {
    const char *v = getenv("MCQ_LAZY_TABLES_MIN");
    return v ? atol(v) : kLazyTablesMin;
}
// Batches of at least encode_lanes_min() vectors are encoded as chunks on TWO lanes (mcq_lanes.h), when encode_lanes() allows a
// second one.  MCQ_ENCODE_LANES=1: one lane at the one-lane chunk size whatever the batch (same-library A/B), 2: a second lane;
// MCQ_ENCODE_LANES_MIN=<n> moves the threshold (0: any batch).  Both read per call
// (unprofiled bench pairs, 8 x 256, dim 512, three each, one lane against two: 8,192 vectors 0.763-0.766 against 0.783-0.788 ms --
// the fork and join lose --, 16,384 1.306-1.315 against 1.300-1.310, overlap, 32,768 2.372-2.380 against 2.300-2.319, 65,536
// 4.531-4.558 against 4.346-4.467 and 131,072 9.042-9.120 against 8.761-8.803, ranges apart: profiles/r27_ab_two_lanes.txt.  The
// halves of 32,768 are chunks of 16,384: still at kErDenseMin and kLazyTablesMin)
constexpr int kEncodeLanes = 2;
constexpr long kEncodeLanesMin = 32768;
inline int encode_lanes() {
    const char *v = getenv("MCQ_ENCODE_LANES");
    const int n = v ? atoi(v) : kEncodeLanes;
    return n >= 2 ? 2 : 1;
}
inline long encode_lanes_min() {
    const char *v = getenv("MCQ_ENCODE_LANES_MIN");
    return v ? atol(v) : kEncodeLanesMin;
}

// the combines of one refinement pass
template <typename CT>
int run_tf_combines(const float *G, const CT *idx_cur, CT *idx_new, const WorkspaceT<CT> &w, const TfLists &L, long B, int N,
                    int K, const int *nact, hipStream_t st, Prof *prof, bool capped) {
    const bool small = (K == 16);
    const int nlev = tf_levels(N);
    const dim3 wave(64);
    const unsigned cap = cap_wave();
    {   // level 0: single codebooks
        const int keep = (N == 2) ? 1 : L.kc[1];
        CT *fin = (N == 2) ? idx_new : nullptr;
        const dim3 grid((unsigned)(B * (N / 2)));
        Timed t(prof, CAT_LEVEL0);
        const int rc = pick_leaf_lists<CT>(K, [&](auto kc0) {
            constexpr int KC = kc0;
            if constexpr (sizeof(CT) == 1 && KC == 16) {
                // lists of 16 one-byte entries: the slot-major kernel (a 16-lane group of a gather = one table row: a fifth faster than
                // the lane-major one, profiles/r06_ab_pair0_slot_major.txt)
                return pick_bool(pass_strided(grid.x, capped, cap), [&](auto strided) {
                    constexpr bool STRIDED = strided;
                    hipLaunchKernelGGL(k_tf_pair0s<STRIDED>, dim3(pass_grid(grid.x, capped, cap)), wave, 0, st, G, idx_cur, w.E, L, B, N,
                                       K, keep, fin, nact);
                    return counted_launch_rc();
                });
            } else {
                hipLaunchKernelGGL((k_tf_pair0<KC, CT>), grid, wave, 0, st, G, idx_cur, w.E, L, B, N, K, keep, fin, nact);
                return counted_launch_rc();
            }
        });
        if (rc) return rc;
    }
    // the level-1 combines and the cousin tables of level 2 share a launch (k_tf_level1): same workgroup-to-XCD mapping as the two
    // launches, one boundary and one tail less (5.95 -> 5.86 ms per encode of 65,536 vectors, 0.55 -> 0.51 ms at 4,096)
    // -- except in chunks of lazy_tables_min() vectors or more (8 / 16 codebooks of 32 entries or more, one-byte entries): the level-1
    // combines as k_tf_pair1, then ONE k_tf_table1 launch that builds the cousin tables of level 2 -- with 16 codebooks those of
    // level 3 as well, into tabs[1] -- on the candidates the level-2 lists name.  A launch more with 8 codebooks, none with 16
    const bool lazy = sizeof(CT) == 1 && !small && (N == 8 || N == 16) && B >= lazy_tables_min();
    const bool fuse_l1 = (N >= 8) && !lazy;
    // 16 codebooks: the 16 cousin tables of level 3 ride along (into tabs[1]).  With 256-entry codebooks at 65,536 vectors
    // that launch is 0.93 ms long and the merge bought nothing (23.99 / 23.92 against 23.90 / 24.0 ms per encode); a trainer
    // step of the first phase (16 x 16 codebooks, 4,096 vectors) saves a 29 us launch per pass
    const bool fuse_l3 = fuse_l1 && N == 16 && small;
    if (lazy) {
        if constexpr (sizeof(CT) == 1) {
            const int ntab1 = (N >> 3) * 4, ntab3 = (N == 16) ? 16 : 1, per3 = (N == 16) ? 4 : 1;
            const unsigned pair_blocks = (unsigned)(B * (N / 4)), tab_blocks = (unsigned)(B * ntab1);
            const unsigned vgrid = tab_blocks + (N == 16 ? (unsigned)(B * ntab3) : 0u);
            // (each launch takes the looping form by its own grid: at 32,768 vectors of 8 codebooks the level-1 combines fit the cap
            // and the tables do not)
            int rc = pick_bool(pass_strided(pair_blocks, capped, cap), [&](auto strided) {
                constexpr bool STRIDED = strided;
                Timed t(prof, CAT_LEVEL1);
                hipLaunchKernelGGL((k_tf_pair1<16, 16, CT, STRIDED>), dim3(pass_grid(pair_blocks, capped, cap)), wave, 0, st, G, idx_cur,
                                   w.E, L, B, N, K, L.kc[2], static_cast<CT *>(nullptr), nact);
                return counted_launch_rc();
            });
            if (rc) return rc;
            rc = pick_bool(pass_strided(vgrid, capped, cap), [&](auto strided) {
                constexpr bool STRIDED = strided;
                Timed t(prof, N == 16 ? CAT_TABLES_UP : CAT_TABLES);      // (16 codebooks: the category of their level-3 launch)
                hipLaunchKernelGGL((k_tf_table1<16, 16, CT, true, STRIDED>), dim3(pass_grid(vgrid, capped, cap)), wave, 0, st, G, idx_cur,
                                   L, B, N, K, ntab1, 2, w.tabs[0], nact, tab_blocks, ntab3, per3, w.tabs[1], vgrid);
                return counted_launch_rc();
            });
            if (rc) return rc;
        }
    } else if (fuse_l1) {
        const int keep = L.kc[2];
        const int groups2 = N >> 3, per1 = 2, ntab1 = groups2 * per1 * per1;
        const unsigned pair_blocks = (unsigned)(B * (N / 4)), tab_blocks = (unsigned)(B * ntab1);
        const int ntab3 = fuse_l3 ? 16 : 1, per3 = fuse_l3 ? 4 : 1;
        const unsigned vgrid = pair_blocks + tab_blocks + (fuse_l3 ? (unsigned)(B * ntab3) : 0u);
        const dim3 grid(pass_grid(vgrid, capped, cap));
        Timed t(prof, CAT_LEVEL1_FUSED);
        const int rc = pick_leaf_lists<CT>(K, [&](auto kc0) {
            return pick_bool(pass_strided(vgrid, capped, cap), [&](auto strided) {
                constexpr int KC = decltype(kc0)::value;
                constexpr bool STRIDED = strided;
                hipLaunchKernelGGL((k_tf_level1<KC, KC, CT, STRIDED>), grid, wave, 0, st, G, idx_cur, w.E, L, B, N, K, keep, ntab1, per1,
                                   w.tabs[0], nact, pair_blocks, tab_blocks, ntab3, per3, w.tabs[1], vgrid);
                return counted_launch_rc();
            });
        });
        if (rc) return rc;
    } else if (N >= 4) {   // level 1: pairs of codebooks -- four codebooks (eight and more: above), so this is the last combine
        Timed t(prof, CAT_LEVEL1);
        const int rc = pick_leaf_lists<CT>(K, [&](auto kc0) {
            constexpr int KC = kc0;
            hipLaunchKernelGGL((k_tf_pair1<KC, KC, CT>), dim3((unsigned)B), wave, 0, st, G, idx_cur, w.E, L, B, N, K, 1, idx_new, nact);
            return counted_launch_rc();
        });
        if (rc) return rc;
    }
    for (int v = 2; v < nlev; ++v) {   // level v: level-1 tables of the cousins below, raised level by level, then the combine
        const int groups = N >> (v + 1);
        const bool last = (v == nlev - 1);
        const int keep = last ? 1 : L.kc[v + 1];
        CT *fin = last ? idx_new : nullptr;
        const int per1 = 1 << (v - 1), ntab1 = groups * per1 * per1;
        const int cat_tab = (v == 2) ? CAT_TABLES : CAT_TABLES_UP, cat_comb = (v == 2) ? CAT_COMBINE : CAT_COMBINE_UP;
        if (!(fuse_l1 && v == 2) && !(fuse_l3 && v == 3) && !lazy) {     // (these tables came with the level-1 combines, or right after them)
            Timed t(prof, cat_tab);
            const int rc = pick_leaf_lists<CT>(K, [&](auto kc0) {
                constexpr int KC = kc0;
                // (every launch here is of level 3 or above and follows the level-1 combines: lists of 16 one-byte entries take the
                // mask of the level-2 lists at no boundary -- 16 codebooks below lazy_tables_min(), 32 and 64 codebooks: 16 x 256,
                // dim 1024, 256 / 1,024 / 4,096 vectors 0.449 / 0.652 / 1.577 against 0.453 / 0.665 / 1.637 ms, 32 x 256 at 4,096 /
                // 32,768 vectors 10.12 / 79.2 against 11.24 / 88.3 ms, ranges apart everywhere: profiles/r26_ab_lazy_tables.txt)
                constexpr bool USED2 = sizeof(CT) == 1 && KC == 16;
                hipLaunchKernelGGL((k_tf_table1<KC, KC, CT, USED2>), dim3((unsigned)(B * ntab1)), wave, 0, st, G, idx_cur, L, B, N, K, ntab1, per1,
                                   w.tabs[0], nact, (unsigned)(B * ntab1), 1, 1, static_cast<float *>(nullptr), (unsigned)(B * ntab1));
                return counted_launch_rc();
            });
            if (rc) return rc;
        }
        if (N == 16 && v == 3) {       // two groups of eight: levels 2 and 3 in one kernel, tables in LDS
            Timed t(prof, cat_comb);
            const float *t3 = (fuse_l3 || lazy) ? w.tabs[1] : w.tabs[0];
            const int rc = pick_leaf_lists<CT>(K, [&](auto kc0) {
                constexpr int KC = kc0;
                hipLaunchKernelGGL((k_tf_comb3<KC, 2 * KC, 2 * KC, CT>), dim3((unsigned)B), dim3(256), 0, st, idx_cur, w.E, L, B, N, t3, idx_new, nact);
                return counted_launch_rc();
            });
            if (rc) return rc;
            continue;
        }
        int cur = 0;
        for (int u = 2; u < v; ++u) {
            const int per = 1 << (v - u), ntab = groups * per * per;
            Timed t(prof, cat_tab);
            if (const int rc = launch_tf_up(L.kc[u - 1], L.kc[u], L, B, N, u, ntab, per, w.tabs[cur], w.tabs[cur ^ 1], nact, st)) return rc;
            cur ^= 1;
        }
        Timed t(prof, cat_comb);
        if (const int rc = launch_tf_comb<CT>(L.kc[v - 1], L.kc[v], w.E, L, B, N, v, keep, w.tabs[cur], fin, nact, st, capped)) return rc;
    }
    return 0;
}

// ---------------------------------------------------------------- the encode: checks, then per chunk start / pass16 or passes / tail
struct EncodeCall {     // what every chunk of one call shares
    Prepared P;
    float lscale;
    int N, K, D, iters;
    unsigned flags;
    hipStream_t st;
    Prof *prof;
};

// Where a chunk's codes go: the caller's arrays at the chunk's first vector (null where the caller gave none)
struct ChunkOut {
    uint8_t *u8;            // out_u8: `pack` codes per byte
    int64_t *i64;
    uint8_t *also;          // codes_also: with i64, the same indexes as unpacked bytes [B][N]
    int pack;
    uint8_t *bytes() const { return u8 ? u8 : also; }        // the byte array of a kernel that writes one: out_u8, else codes_also
    int bytes_pack() const { return u8 ? pack : 1; }         // (codes_also is never packed)
};

// The start of a chunk: its frames as limb planes, centered (x - mean: both products of the call read them; |x - mean|^2 rides
// along), the initial codes -- imported, or the arg max of the logits -- and the x.C products the passes read
template <typename CT>
int launch_chunk_start(const EncodeCall &c, const WorkspaceT<CT> &w, const float *xc, long Bc, const int64_t *init_idx,
                       float *logits_out) {
    const int N = c.N, K = c.K, D = c.D;
    // codes only: the initial arg max from six of the ten limb products, the pairs they leave open redone exactly (same
    // codes).  The list lies in the x.C products, which the launch after the recheck writes; its counter is the last
    // of the 64 pass counters (passes use the first 60), cleared by the frames' limb kernel
    const bool screen = init_idx == nullptr && logits_out == nullptr && (c.flags & MCQ_ENCODE_EXACT_LOGITS) == 0 &&
                        !exact_logits_forced() && (size_t)Bc * N < ((size_t)1 << 31);
    unsigned *const und_cnt = reinterpret_cast<unsigned *>(w.cnt + 63), *const und_list = reinterpret_cast<unsigned *>(w.XC);
    if (init_idx == nullptr || c.iters > 0) {
        Timed t(c.prof, CAT_XX);
        const int xh = (c.flags & MCQ_ENCODE_X_FP16) ? 1 : 0;   // rows of 2-byte elements
        if (const int rc = launch_fix_rows(xc, xh, Bc, D, D, w.xf, w.xe, w.xx, c.st, c.P.mean, screen ? und_cnt : nullptr)) return rc;
    }
    if (init_idx != nullptr) {
        hipLaunchKernelGGL(k_import_indexes<CT>, dim3((unsigned)((Bc * N + 255) / 256)), dim3(256), 0, c.st, init_idx, Bc * N, K, w.idx);
        MCQ_LAUNCH_CHECK();
        if (c.prof) c.prof->untimed();
    } else {
        Timed t(c.prof, CAT_LOGITS);
        if (const int rc = launch_logits(w.xf, w.xe, Bc, c.P, N, K, D, c.lscale,
                                         (c.flags & MCQ_ENCODE_LSCALE_FROM_PREPARED) ? c.P.scales + 1 : nullptr, logits_out, w.idx, c.st,
                                         screen ? und_cnt : nullptr, und_list))
            return rc;
    }
    if (c.iters > 0) {   // what the passes read per vector: the x.C products, once per call
        Timed t(c.prof, CAT_XC);
        if (const int rc = launch_xc(w.xf, w.xe, Bc, c.P.Cf, c.P.Ce, (long)N * K, D, w.XC, c.st)) return rc;
    }
    return 0;
}

// 16 or 8 codebooks of 16 entries (the trainer's first phase at 8 / 4 bytes per frame): ALL passes of the call in one launch of
// persistent workgroups that hold the Gram matrix in LDS (mcq_pass16_kernels.h); a wave leaves a vector at its fixed point
// by itself, without compaction.  Not under the profiler, whose categories are the separate launches.  The kernel writes the
// caller's arrays itself where codes are not packed (out.pack == 1); packed nibbles leave through k_finalize, from w.idx
// (mcq_test_pass16 of include/mcq_probe.h only: dump -- the probe instantiation, which also leaves a record per vector and pass
// there; max_wgs > 0 -- fewer workgroups than the launcher's own cap, the kernel strides by its grid)
int launch_pass16(const EncodeCall &c, const WorkspaceT<uint8_t> &w, long Bc, const ChunkOut &out, uint8_t *dump = nullptr,
                  int max_wgs = 0) {
    // the first pass16 call on a device opts BOTH shapes in: the other shape's first call may come inside a captured stream
    // (flags of the device's record, set under its mutex: two host threads, or the two lanes' first chunks, find them consistent)
    auto opt_in = [](const void *k16, const void *k8) {
        const hipError_t e16 = hipFuncSetAttribute(k16, hipFuncAttributeMaxDynamicSharedMemorySize, p16_lds_bytes<16>());
        if (e16 != hipSuccess) return (int)e16;
        return (int)hipFuncSetAttribute(k8, hipFuncAttributeMaxDynamicSharedMemorySize, p16_lds_bytes<8>());
    };
    {
        DeviceRec *const r = device_rec();
        std::unique_lock<std::mutex> lock;
        if (r) lock = std::unique_lock<std::mutex>(r->lds_mu);
        if (!r || !r->pass16_ok) {
            if (const int rc = opt_in(reinterpret_cast<const void *>(&k_tf_pass16<16>), reinterpret_cast<const void *>(&k_tf_pass16<8>)))
                return rc;
            if (r) r->pass16_ok = true;
        }
        if (dump && (!r || !r->pass16_probe_ok)) {
            if (const int rc = opt_in(reinterpret_cast<const void *>(&k_tf_pass16_probe<16>),
                                      reinterpret_cast<const void *>(&k_tf_pass16_probe<8>)))
                return rc;
            if (r) r->pass16_probe_ok = true;
        }
    }
    Pass16Args a;
    a.G = c.P.G; a.XC = w.XC; a.xx = w.xx; a.Q = c.P.Q; a.idx = w.idx; a.B = Bc; a.iters = c.iters;
    a.out_i64 = out.pack == 1 ? out.i64 : nullptr;
    a.out_u8 = out.pack == 1 ? out.bytes() : nullptr;
    const long wgs = (Bc + kP16Waves - 1) / kP16Waves;
    return pick<16, 8>(c.N, [&](auto nn) {   // one workgroup per CU (157,696 B of LDS), two with eight codebooks (62,464 B)
        constexpr int NN = nn, cap = NN == 16 ? 256 : 512;
        const long lim = (max_wgs > 0 && max_wgs < cap) ? max_wgs : cap;
        const dim3 grid((unsigned)(wgs < lim ? wgs : lim)), block(64 * kP16Waves);
        if (dump) hipLaunchKernelGGL(k_tf_pass16_probe<NN>, grid, block, p16_lds_bytes<NN>(), c.st, a, dump);
        else hipLaunchKernelGGL(k_tf_pass16<NN>, grid, block, p16_lds_bytes<NN>(), c.st, a);
        return counted_launch_rc();
    });
}

// What moves from pass to pass.  Without skipping the indexes are refined in place in w.idx and nothing rotates.  Under skipping
// k_compact packs the vectors still active after a pass to the front: slot s is the caller's row map[s], *nact slots are in use
template <typename CT>
struct PassState {
    CT *idx_cur, *idx_new, *idx_pk;           // the indexes a pass reads / writes, and where k_compact packs the active ones
    int *map_cur = nullptr, *map_nxt, *map_spare, *cnt;
    const int *nact = nullptr;
    // E / R of the active slots; under skipping with E / R formed in the emit they move with the indexes into the packed
    // slots, between w.E / w.R and a second pair in the Gram-terms buffer (which only the first pass's k_tf_gram_terms uses).
    // With E / R formed ahead of every pass (er_dense_min()) nothing moves: w.E / w.R throughout, the buffer is k_tf_gram_terms' own
    float *E_cur, *R_cur, *E_alt, *R_alt;

    PassState(const WorkspaceT<CT> &w, long Bc, bool skip)
        : idx_cur(w.idx), idx_new(skip ? w.idxB : w.idx), idx_pk(w.idxC), map_nxt(w.map[0]), map_spare(w.map[1]), cnt(w.cnt),
          E_cur(w.E), R_cur(w.R), E_alt(w.gterms), R_alt(w.gterms + ((Bc + 3) & ~3L)) {}

    // after k_compact of pass `it`: the packed list becomes the current one, its map the current map (the first pass has none
    // to hand back: the spare takes its place), its count the active count; E / R follow the indexes when the emit formed them
    void rotate(int it, bool er_ready) {
        std::swap(idx_cur, idx_pk);
        std::swap(map_cur, map_nxt);
        if (map_nxt == nullptr) map_nxt = map_spare;
        nact = cnt + it;
        if (er_ready) { std::swap(E_cur, E_alt); std::swap(R_cur, R_alt); }
    }
};

// One refinement pass of a chunk: E / R of the slots (unless the pass before formed them in its emitting wave), stage 0, the
// combines.  run_passes below calls it pass by pass; mcq_test_pass of include/mcq_probe.h calls it once.  emit_er: the emitting
// wave of this pass forms E / R of the next one (er_ready then leaves as true); last_pass: the winners also go to `out`
template <typename CT>
int run_one_pass(const EncodeCall &c, const WorkspaceT<CT> &w, long Bc, const PassState<CT> &s, bool last_pass, bool emit_er,
                 bool capped, bool &er_ready, const ChunkOut &out) {
    const int N = c.N, K = c.K;
    const Prepared &P = c.P;
    if (!er_ready) {
        Timed t(c.prof, CAT_ER);
        if (const int rc = launch_tf_er<CT>(N, P.G, w.XC, s.idx_cur, w.xx, Bc, K, s.E_cur, s.R_cur, w.gterms, Bc, s.nact, s.map_cur, c.st))
            return rc;
    }
    er_ready = false;
    {
        Timed t(c.prof, CAT_STAGE0);
        if (const int rc = launch_tf_stage0(K, N, P.G, w.XC, s.idx_cur, s.R_cur, P.Q, Bc, (N == 1) ? 1 : w.tf.kc[0],
                                            reinterpret_cast<CT *>(w.tf.ent), w.tf.S[0], (N == 1) ? s.idx_new : static_cast<CT *>(nullptr),
                                            s.nact, s.map_cur, c.st, capped))
            return rc;
    }
    if (N >= 2) {
        TfLists L = w.tf;
        L.map = s.map_cur;
        if (emit_er && !last_pass) {
            L.erG = P.G; L.erXC = w.XC; L.erxx = w.xx; L.erE = s.E_cur; L.erR = s.R_cur; L.erK = K;
            er_ready = true;
        }
        if (last_pass) { L.out_i64 = out.i64; L.out_u8 = out.bytes(); L.out_pack = out.bytes_pack(); }
        WorkspaceT<CT> wc = w;
        wc.E = s.E_cur; wc.R = s.R_cur;
        if (const int rc = run_tf_combines<CT>(P.G, s.idx_cur, s.idx_new, wc, L, Bc, N, K, s.nact, c.st, c.prof, capped)) return rc;
    }
    return 0;
}

// The refinement passes of a chunk as separate launches.  With two codebooks or more the last pass's winners go straight to
// the caller's arrays (tf_emit; under skipping to row map[slot]); a single codebook's stay in w.idx for k_finalize.  skip: after
// every pass but an emitting one k_compact retires the vectors the pass left unchanged (to the caller's arrays) and packs the rest
template <typename CT>
int run_passes(const EncodeCall &c, const WorkspaceT<CT> &w, long Bc, bool skip, const ChunkOut &out) {
    const int N = c.N;
    PassState<CT> s(w, Bc, skip);
    if (skip) {     // (a kernel, not hipMemsetAsync: replays of a captured encode have to clear them too, LAB_NOTEBOOK.md)
        hipLaunchKernelGGL(k_zero_counts, dim3(1), dim3(64), 0, c.st, w.cnt, 64);
        MCQ_LAUNCH_CHECK();
        if (c.prof) c.prof->untimed();
    }
    // E / R of pass it + 1 can be formed by the wave that emits the indexes of pass it (tf_emit), which saves that pass
    // its two E / R launches (4, 8 or 16 codebooks); under skipping k_compact moves them into the packed slots
    // -- except in chunks of er_dense_min() vectors or more, where the two dense launches ahead of every pass cost less than the
    // dependent memory phase at the end of every emitting wave's life: k_compact then moves no E / R, the Gram-terms buffer is
    // never borrowed, and a retired vector has none formed
    const bool er_in_emit = (N == 4 || N == 8 || N == 16) && !(sizeof(CT) == 1 && Bc >= er_dense_min());
    bool er_ready = false;
    for (int it = 0; it < c.iters; ++it) {
        const bool last_pass = (it + 1 == c.iters);
        // capped grids over the active vectors from the fourth pass on (passes 1-3 hold nearly every vector of an
        // untrained batch, and the strided kernels cost the dense passes a few per cent: DESIGN.md section 4)
        const bool capped = skip && it >= 3;
        if (const int rc = run_one_pass<CT>(c, w, Bc, s, last_pass, er_in_emit, capped, er_ready, out)) return rc;
        const bool emits = N >= 2 && last_pass;
        if (skip && !emits) {
            {
                Timed t(c.prof, CAT_TAIL);
                hipLaunchKernelGGL(k_compact<CT>, dim3((unsigned)((Bc + 255) / 256)), dim3(256), 0, c.st, s.idx_cur, s.idx_new, s.map_cur,
                                   s.nact, Bc, N, last_pass ? 1 : 0, s.idx_pk, s.map_nxt, w.cnt + it, er_ready ? s.E_cur : nullptr,
                                   er_ready ? s.R_cur : nullptr, s.E_alt, s.R_alt, out.pack, out.u8, out.i64, out.also);
                MCQ_LAUNCH_CHECK();
            }
            s.rotate(it, er_ready);
        }
    }
    return 0;
}

template <typename CT>
int run_encode_t(const float *x, long B, const void *prepared, float lscale, int N, int K, int D, int iters,
                 uint8_t *out_u8, int64_t *out_i64, void *workspace, size_t workspace_bytes, hipStream_t st,
                 Prof *prof, const int64_t *init_idx, unsigned flags, float *logits_out,
                 uint8_t *codes_also /* with out_i64: the same indexes as unpacked bytes [B][N] */) {
    g_last_launches = 0;
    if (!domain_ok(N, K, D)) return domain_err(N, K, D);
    if (B < 0 || iters < 0 || iters > 60 || (out_u8 == nullptr) == (out_i64 == nullptr)) return MCQ_EINVAL;
    // entries of more than 256-entry codebooks do not fit the byte outputs (encode(as_bytes=True) asserts the same, :271)
    if (sizeof(CT) > 1 && (out_u8 != nullptr || codes_also != nullptr)) return MCQ_EINVAL;
    if (B == 0) return 0;
    if (!x || !prepared || !workspace) return MCQ_EINVAL;
    const size_t per = workspace_per_vector(N, K, D);
    // The plan: one lane, or two for a batch of encode_lanes_min() vectors or more -- unless the caller's stream is capturing (a
    // fork inside a captured graph makes parallel branches), which takes the one-lane sequence as it always was
    ChunkPlan plan;
    bool two = encode_lanes() == 2 && B >= encode_lanes_min();
    if (two && prof == nullptr) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cap) != hipSuccess) { (void)hipGetLastError(); two = false; }
        else if (cap != hipStreamCaptureStatusNone) two = false;
    }
    if (two) two = plan_two_lanes(B, workspace_bytes, per, lane_slack(D), &plan);
    if (!two && !plan_one_lane(B, workspace_bytes, per, lane_slack(D), &plan)) return MCQ_EWORKSPACE;
    // Fork: lane 1 starts behind everything the caller's stream holds now -- the frames, `prepared`, earlier users of the
    // workspace.  The profiler keeps its one stream: the same chunks on the same shares, one after the other (include/mcq.h)
    DeviceRec *rec = nullptr;
    std::unique_lock<std::mutex> lanes_lock;
    if (two && prof == nullptr && plan.chunks >= 2 && (rec = device_rec()) != nullptr) {
        lanes_lock = std::unique_lock<std::mutex>(rec->mu);
        if (!lanes_ready(*rec) || hipEventRecord(rec->fork, st) != hipSuccess || hipStreamWaitEvent(rec->side, rec->fork, 0) != hipSuccess) {
            (void)hipGetLastError();
            lanes_lock.unlock();
            rec = nullptr;
        }
    }
    if (two && prof == nullptr && rec == nullptr && plan.chunks >= 2 &&
        !plan_one_lane(B, workspace_bytes, per, lane_slack(D), &plan))      // no second stream: today's sequence
        return MCQ_EWORKSPACE;
    const hipStream_t lane_st[kMaxLanes] = {st, rec ? rec->side : st};
    g_last_lanes = rec ? 2 : 1;
    const EncodeCall c{prepared_view(prepared, N, K, D), lscale, N, K, D, iters, flags, st, prof};
    const int pack = (out_u8 != nullptr && K == 16 && N >= 2) ? 2 : 1;
    // fixed-point skipping (the default; MCQ_ENCODE_ALL_PASSES turns it off): vectors whose indexes a pass leaves unchanged
    // drop out of the later passes (k_compact) and their codes go straight to the caller's arrays; results are identical, the
    // cost becomes data dependent.  Below skip_min_batch() vectors per chunk the passes are bound by the launch chain, and the
    // compactions would only add launches to it
    const bool want_skip = (flags & MCQ_ENCODE_ALL_PASSES) == 0 && iters >= 3;     // (with two passes the second one holds ~every vector)
    const bool use_p16 = sizeof(CT) == 1 && K == 16 && (N == 16 || N == 8) && iters > 0 && prof == nullptr && pass16_enabled();

    // one chunk on its lane: `cl` is the call with the lane's stream, `ws` the lane's share
    auto encode_chunk = [&](const EncodeCall &cl, void *ws, long lo, long Bc) -> int {
        const WorkspaceT<CT> w = carve<CT>(ws, Bc, N, K, D);
        const ChunkOut out{out_u8 ? out_u8 + lo * (N / pack) : nullptr, out_i64 ? out_i64 + lo * N : nullptr,
                           codes_also ? codes_also + lo * N : nullptr, pack};
        const float *xc = (flags & MCQ_ENCODE_X_FP16) ? reinterpret_cast<const float *>(reinterpret_cast<const uint16_t *>(x) + lo * D)
                                                      : x + lo * D;
        if (const int rc = launch_chunk_start<CT>(cl, w, xc, Bc, init_idx ? init_idx + lo * N : nullptr,
                                                  logits_out ? logits_out + lo * N * K : nullptr))
            return rc;
        bool left = false;      // the codes are in the caller's arrays already; otherwise in w.idx, for k_finalize
        if constexpr (sizeof(CT) == 1) {
            if (use_p16) {
                if (const int rc = launch_pass16(cl, w, Bc, out)) return rc;
                left = out.pack == 1;
            }
        }
        if (!use_p16) {
            const bool skip = want_skip && Bc >= skip_min_batch();
            if (const int rc = run_passes<CT>(cl, w, Bc, skip, out)) return rc;
            left = skip || (iters > 0 && N >= 2);      // every vector left through k_compact or the last emit / the last emit
        }
        if (left) return 0;
        const long outn = out.i64 ? Bc * N : Bc * (N / pack);
        Timed t(prof, CAT_TAIL);
        hipLaunchKernelGGL(k_finalize<CT>, dim3((unsigned)((outn + 255) / 256)), dim3(256), 0, cl.st, w.idx, Bc, N, pack, out.u8, out.i64,
                           out.also);
        MCQ_LAUNCH_CHECK();
        return 0;
    };
    // chunk i on lane i mod lanes; between fork and join the lanes never wait for each other
    int rc = 0;
    for (long i = 0; i < plan.chunks && rc == 0; ++i) {
        const int lane = plan.lane_of(i);
        EncodeCall cl = c;
        cl.st = lane_st[lane];
        rc = encode_chunk(cl, static_cast<char *>(workspace) + plan.lane_off[lane], plan.first_of(i), plan.rows_of(i, B));
    }
    // Join, also after a failed launch: from here the caller's stream alone orders the codes and the workspace.  A join that cannot
    // be enqueued is made on the host
    if (rec != nullptr && (hipEventRecord(rec->join, rec->side) != hipSuccess || hipStreamWaitEvent(st, rec->join, 0) != hipSuccess)) {
        const hipError_t e = hipGetLastError();
        (void)hipStreamSynchronize(rec->side);
        if (rc == 0) rc = e != hipSuccess ? (int)e : MCQ_EINVAL;
    }
    return rc;
}

int run_encode(const float *x, long B, const void *prepared, float lscale, int N, int K, int D, int iters,
               uint8_t *out_u8, int64_t *out_i64, void *workspace, size_t workspace_bytes, hipStream_t st,
               Prof *prof, const int64_t *init_idx = nullptr, unsigned flags = 0, float *logits_out = nullptr,
               uint8_t *codes_also = nullptr) {
    if (K > 256)
        return run_encode_t<uint16_t>(x, B, prepared, lscale, N, K, D, iters, out_u8, out_i64, workspace, workspace_bytes, st, prof,
                                      init_idx, flags, logits_out, codes_also);
    return run_encode_t<uint8_t>(x, B, prepared, lscale, N, K, D, iters, out_u8, out_i64, workspace, workspace_bytes, st, prof,
                                 init_idx, flags, logits_out, codes_also);
}

// mcq_test_pass of include/mcq_probe.h: one pass of B vectors as ONE chunk from imported codes -- the chunk start, then
// run_one_pass as the last pass of a call without skipping, on the slots / rows the caller names
template <typename CT>
int test_pass(const EncodeCall &c, const float *x, long B, const int64_t *idx_in, int64_t *idx_out, const int *nact, const int *map,
              bool capped, void *workspace) {
    const WorkspaceT<CT> w = carve<CT>(workspace, B, c.N, c.K, c.D);
    if (const int rc = launch_chunk_start<CT>(c, w, x, B, idx_in, nullptr)) return rc;
    PassState<CT> s(w, B, false);
    s.nact = nact;
    s.map_cur = const_cast<int *>(map);       // (read only: nothing rotates without k_compact)
    bool er_ready = false;
    return run_one_pass<CT>(c, w, B, s, true, false, capped, er_ready, ChunkOut{nullptr, idx_out, nullptr, 1});
}

// floats per lane of k_decode_backward when every row involved is 16-byte aligned.  Codebooks of 64 entries and more: 4 (a
// row has few matching vectors, the kernel is bound by scanning the index column, so as few waves per row as possible:
// 22.5 us with 4, 28.3 with 2, 41.4 with 1 at 8 x 256, dim 512, 4,096 vectors).  Smaller codebooks: the widest of 4, 2, 1
// that leaves four feature chunks (a row gathers many vectors; more, narrower waves and an L2 that holds a quarter of the
// gradient matrix: 35.5 us with 4, 28.7 with 2, 30.2 with 1 at 16 x 16).  1 for unaligned rows.
int db_cw_of(int D, int K) {
    if ((D & 3) != 0) return 1;
    if (K >= 64) return 4;
    return D >= 1024 ? 4 : (D >= 512 ? 2 : 1);
}
int db_cw(const void *g, const void *out, int D, int K, long gsb, long gsn, const void *dotw = nullptr) {
    const bool al = ((D & 3) == 0) && ((gsb & 3) == 0) && ((gsn & 3) == 0) && ((reinterpret_cast<uintptr_t>(g) & 15) == 0) &&
                    ((reinterpret_cast<uintptr_t>(out) & 15) == 0) && ((reinterpret_cast<uintptr_t>(dotw) & 15) == 0);
    return al ? db_cw_of(D, K) : 1;
}
int db_chunks(int D, int cw) { return (D + 64 * cw - 1) / (64 * cw); }

template <typename IdxT>
int launch_decode_backward(const float *g, const IdxT *idx, long B, int N, int K, int D, float *out, long gsb, long gsn,
                           int idx_stride, hipStream_t st, const float *sa = nullptr, const float *sb = nullptr, float sc = 1.0f,
                           const float *dotw = nullptr, float *dot_part = nullptr) {
    const int cw = db_cw(g, out, D, K, gsb, gsn, dotw), chunks = db_chunks(D, cw);
    const long rowgroups = ((long)N * K + 3) / 4;
    long blocks;
    if (chunks <= 8 && (8 % chunks) == 0) blocks = ((rowgroups + (8 / chunks) - 1) / (8 / chunks)) * 8;
    else blocks = ((long)N * K * chunks + 3) / 4;
    const dim3 grid((unsigned)blocks), block(256);
    return pick<4, 2, 1>(cw, [&](auto w) {
        constexpr int CW = w;
        hipLaunchKernelGGL((k_decode_backward<IdxT, CW>), grid, block, 0, st, g, idx, B, N, K, D, chunks, out, gsb, gsn, idx_stride, sa, sb, sc,
                           dotw, dot_part);
        return launch_rc();
    });
}
}  // namespace

// ---- search over stored codes (mcq_search_kernels.h) -------------------------------------------------------------------
namespace {

// one-byte codes, lists of at most one entry per lane, positions that fit an int
int search_domain(int N, int K, int D) {
    if (!domain_ok(N, K, D)) return domain_err(N, K, D);
    return K > 256 ? MCQ_EUNSUPPORTED : 0;
}

// two-byte codes (include/mcq_code16.h rule 33): every codebook size of the library; N * K <= kMaxRows is the 64 KiB of table
// the list kernels carry beside the probe ranges
int code16_domain(int N, int K, int D) { return domain_ok(N, K, D) ? 0 : domain_err(N, K, D); }
static_assert(wide_lds_bytes(kMaxRows, kListMaxProbes, kWideMaxK) <= 160 * 1024, "the table of a two-byte call fits the CU");

// the probe set of a call that goes list by list (rules 13-20); a call over the whole store has none and passes NULL
struct ListsIn {
    const int64_t *list_offsets;
    long L;
    const int32_t *probes;
    int P;
    const float *bias = nullptr;              // rule 21: float[Q][P], one value per (query, probe slot); NULL: none
};
// the whole store as one list: probes == NULL to k_search_wide and k_range_lists
constexpr ListsIn kWholeStore{nullptr, 0, nullptr, 1};

// the table rows a list kernel over codes of type T is allowed LDS for: 64 codebooks of 256 entries under one-byte codes, the
// library's cap under two-byte ones (N = 64 is reachable at K <= 256 only, rule 33)
template <typename T>
constexpr int kTableRowsOf = sizeof(T) == 2 ? kMaxRows : 64 * 256;

// checks that several entry points make, each where its own order has it (the test_*_host.py files pin the orders)
bool metric_ok(int metric) { return metric == MCQ_SEARCH_L2 || metric == MCQ_SEARCH_IP || metric == MCQ_SEARCH_COS; }
bool w_ok(const float *w, int metric) { return w || metric == MCQ_SEARCH_IP; }          // (the inner product never reads w)
bool codes_aligned(const void *codes, int N, int code_bytes) {           // a candidate's codes are loaded as one vector
    return reinterpret_cast<uintptr_t>(codes) % (N * code_bytes >= 16 ? 16 : N * code_bytes) == 0;
}
// what the mcq_*_workspace_bytes entries of the scans, sweeps and lists size; outside it they answer 256.  n: B up to
// 2^31 - 1, or P up to kListMaxProbes; an entry without k passes 1 of 1
bool sized(long Q, long n, long n_max, int N, int K, int k, int k_max, int code_bytes = 1) {
    return Q >= 1 && Q <= 0x7fffffffL && n >= 1 && n <= n_max && k >= 1 && k <= k_max &&
           (code_bytes == 2 ? code16_domain(N, K, 1) : search_domain(N, K, 1)) == 0;
}

// What every scan, sweep and list-by-list entry point rejects, in this order (tests/test_search_host.py, test_search_metric_host.py,
// test_search_mask_host.py, test_search_range_host.py, test_search_lists_host.py and test_search_range_lists_host.py pin it);
// nothing touches the device.  k: 1 where the entry has none.  outs_ok: the outputs this call writes are there (the caller
// knows which of them an empty call still writes).  *empty: the call has no candidate anywhere (Q or B is 0; with lists, L or
// P) -- it reads no input, so none is looked at.  mask: NULL where the call has none (rule 12); one that is there is read as
// 8-byte words.  li: the limits of rule 16 come between B's and the outputs, its pointers and alignments with the others
// (a bias, rule 23, is optional: only its alignment is looked at, last).  code_bytes: 1, or 2 for the entries of
// include/mcq_code16.h, which differ in the domain and in the alignment of the codes (rules 33 and 34) and in nothing else.
int search_check(const float *tables, long Q, const void *codes, const float *w, long B, int N, int K, int k, int metric,
                 const uint64_t *mask, const ListsIn *li, bool outs_ok, const void *workspace, bool *empty, int code_bytes = 1) {
    *empty = false;
    if (const int rc = code_bytes == 2 ? code16_domain(N, K, 1) : search_domain(N, K, 1)) return rc;
    if (k > 64) return MCQ_EUNSUPPORTED;
    if (k < 1 || Q < 0 || B < 0 || Q > 0x7fffffffL) return MCQ_EINVAL;
    if (!metric_ok(metric)) return MCQ_EINVAL;
    if (B > 0x7fffffffL) return MCQ_EUNSUPPORTED;
    if (li && (li->P < 0 || li->L < 0)) return MCQ_EINVAL;
    if (li && li->P > kListMaxProbes) return MCQ_EUNSUPPORTED;
    if (!outs_ok) return MCQ_EINVAL;
    if (Q == 0 || B == 0 || (li && (li->L == 0 || li->P == 0))) {
        *empty = true;
        return 0;
    }
    if (!tables || !codes || !workspace || (li && (!li->list_offsets || !li->probes))) return MCQ_EINVAL;
    if (!w_ok(w, metric) || !codes_aligned(codes, N, code_bytes)) return MCQ_EINVAL;
    if (reinterpret_cast<uintptr_t>(mask) % 8 != 0) return MCQ_EINVAL;
    if (li && (reinterpret_cast<uintptr_t>(li->list_offsets) % 8 != 0 || reinterpret_cast<uintptr_t>(li->probes) % 4 != 0)) return MCQ_EINVAL;
    if (li && reinterpret_cast<uintptr_t>(li->bias) % 4 != 0) return MCQ_EINVAL;
    return 0;
}

// mcq_code_norms (t[b]) and mcq_code_rnorms (RNORM: r[b]); BASED: mcq_code_norms_based and mcq_code_rnorms_based, rule 22, the
// norms of base[assign[b]] + decode(codes[b]) -- its checks of L, base and assign run only then.  T = uint16_t: mcq_code_norms_u16
template <bool RNORM, bool BASED = false, typename T = uint8_t>
int code_norms(const T *codes, long B, const void *prepared, int N, int K, int D, float *out, void *stream,
               const float *base = nullptr, long L = 0, const int32_t *assign = nullptr) {
    if (const int rc = sizeof(T) == 2 ? code16_domain(N, K, D) : search_domain(N, K, D)) return rc;
    if (B < 0) return MCQ_EINVAL;
    if (B > 0x7fffffffL) return MCQ_EUNSUPPORTED;
    if (BASED && L < 0) return MCQ_EINVAL;
    if (B == 0) return 0;
    if (!codes || !prepared || !out) return MCQ_EINVAL;
    if (BASED && (!base || !assign)) return MCQ_EINVAL;
    if (BASED && (reinterpret_cast<uintptr_t>(base) % 4 != 0 || reinterpret_cast<uintptr_t>(assign) % 4 != 0)) return MCQ_EINVAL;
    if (reinterpret_cast<uintptr_t>(codes) % sizeof(T) != 0) return MCQ_EINVAL;
    const Prepared P = prepared_view(prepared, N, K, D);
    return launch_in_pieces(B, 64, [&](long at, long rows) {     // one wave per stored vector
        hipLaunchKernelGGL((k_code_norms<RNORM, BASED, T>), dim3((unsigned)((rows + kNormWaves - 1) / kNormWaves)), dim3(64 * kNormWaves), 0,
                           static_cast<hipStream_t>(stream), codes + at * N, rows, P.C, N, K, round_up16(D), out + at, base, L, D,
                           BASED ? assign + at : assign);
        return launch_rc();
    });
}

// the launch arithmetic of the scan and of the sweeps (mirrored by tile_plan of tests/search_grid.py): a tile of qt queries per
// workgroup -- as many as fit kScanTableLds, no more than the call has -- and as many slices of the store as fill the chip
// once, none shorter than one step of 64 candidates for each of the workgroup's `waves` waves
struct TilePlan {
    int qt, qtiles, slices;
    long per_slice;
};

TilePlan tile_plan(long Q, long B, int N, int K, int waves) {
    TilePlan p;
    int cap = kScanQTMax;
    while (cap > 1 && (size_t)cap * N * K * 4 > (size_t)kScanTableLds) cap /= 2;
    int qt = 1;
    while (qt < cap && qt < Q) qt *= 2;
    p.qt = qt;
    p.qtiles = (int)((Q + qt - 1) / qt);
    long cap_slices = kScanTargetBlocks / (p.qtiles > 0 ? p.qtiles : 1);
    cap_slices = cap_slices < 1 ? 1 : (cap_slices > kScanMaxSlices ? kScanMaxSlices : cap_slices);
    const long steps = (B + 63) / 64;                                    // steps of 64 candidates; at least one per wave
    long want = (steps + waves - 1) / waves;
    want = want < 1 ? 1 : (want > cap_slices ? cap_slices : want);
    p.per_slice = (((B + want - 1) / want) + 63) / 64 * 64;
    if (p.per_slice < 64) p.per_slice = 64;
    p.slices = (int)((B + p.per_slice - 1) / p.per_slice);
    return p;
}

// the workspace of a top-k call: k scores per (query, list), then as many positions, each array 256-aligned
size_t topk_ws_bytes(long Q, int lists, int k) { return 2 * align256((size_t)Q * lists * k * 4); }

// the scan: LDS holds the tables, then the waves' lists; a list per (query, slice)
struct ScanPlan : TilePlan {
    size_t lds, ws_bytes;
};

ScanPlan scan_plan(long Q, long B, int N, int K, int k) {
    ScanPlan p{tile_plan(Q, B, N, K, kScanWaves), 0, 0};
    const size_t tab = (size_t)p.qt * N * K * 4, lists = (size_t)p.qt * kScanWaves * 64 * 8;
    p.lds = tab > lists ? tab : lists;
    p.ws_bytes = topk_ws_bytes(Q, p.slices, k);
    return p;
}

// The metric and the mask are template parameters of the scan (and the mask of the sweeps) as the tile and the codebook count
// are: the L2 instantiations without a mask are the code they were before the other metrics and the masks existed (DESIGN.md
// section 4)
static_assert(kMetricL2 == MCQ_SEARCH_L2 && kMetricIP == MCQ_SEARCH_IP && kMetricCos == MCQ_SEARCH_COS, "include/mcq.h");
int launch_scan(const ScanPlan &p, hipStream_t st, const float *tables, int Q, const uint8_t *codes, const float *w, long B, int N,
                int K, int k, int metric, float *ws_s, int *ws_i, const uint64_t *mask) {
    return pick<kMetricL2, kMetricIP, kMetricCos>(metric, [&](auto m) {
        return pick<1, 2, 4, 8, 16>(p.qt, [&](auto qt) {
            return pick<1, 2, 4, 8, 16, 32, 64>(N, [&](auto nn) {
                return pick_bool(mask != nullptr, [&](auto masked) {
                    constexpr int M = decltype(m)::value, QT = decltype(qt)::value, NN = decltype(nn)::value;
                    constexpr bool MASKED = masked;
                    static bool allowed[64] = {};
                    if (const int rc = allow_dynamic_lds(allowed, reinterpret_cast<const void *>(&k_search_scan<QT, NN, M, MASKED>), kScanTableLds))
                        return rc;
                    hipLaunchKernelGGL((k_search_scan<QT, NN, M, MASKED>), dim3((unsigned)p.qtiles * (unsigned)p.slices), dim3(64 * kScanWaves),
                                       p.lds, st, tables, Q, codes, M == kMetricIP ? nullptr : w, B, K, k, p.slices, p.per_slice, ws_s, ws_i,
                                       reinterpret_cast<const u64 *>(mask));
                    return launch_rc();
                });
            });
        });
    });
}

// The plan of every kernel that gives a workgroup one query and one of `parts` parts of that query's candidates: the search
// list by list, past 64 neighbours and over a shortlist, the re-ranking, the range search list by list.  A function of the
// call's shape alone: what a list or a shortlist row holds is known to the device only (nothing is read back).
// parts == 0 (PartPlan{}): the call has no candidate anywhere.
struct PartPlan {
    int parts;
    size_t lds, ws_bytes;
};

// as many parts as fill the chip once at small Q (`target` workgroups), no more than `cap`, no more than the `steps` a
// query's candidates make where that is known on the host, at least one
int part_count(long Q, long target, long cap, long steps = 0x7fffffffL) {
    long parts = target / (Q > 0 ? Q : 1);
    parts = parts > cap ? cap : parts;
    parts = parts > steps ? steps : parts;
    return (int)(parts < 1 ? 1 : parts);
}
// the cap that keeps the merge of a query to kWideMergeEntries streamed entries per entry of its sorted half: 128 parts up to
// k = 512 and 64 beyond
long wide_merge_cap(int k) { return kWideMergeEntries / wide_half(k); }

// the search list by list (rules 13-16; mirrored by lists_plan of tests/search_lists_grid.py): capped as the slice count is
PartPlan lists_plan(long Q, int P, int N, int K, int k) {
    const int parts = part_count(Q, kListTargetBlocks, kScanMaxSlices);
    return {parts, (size_t)lists_lds_bytes(N * K, P), topk_ws_bytes(Q, parts, k)};
}

// a bias (li.bias != NULL; rules 21 and 23) is one more flag of the same kernel: a call moves between the two by its bias alone
int launch_lists(const PartPlan &p, hipStream_t st, const float *tables, int Q, const uint8_t *codes, const float *w, long B,
                 int N, int K, int k, int metric, const uint64_t *mask, const ListsIn &li, float *ws_s, int *ws_i) {
    return pick<kMetricL2, kMetricIP, kMetricCos>(metric, [&](auto m) {
        return pick<1, 2, 4, 8, 16, 32, 64>(N, [&](auto nn) {
            return pick_bool(mask != nullptr, [&](auto masked) {
                return pick_bool(li.bias != nullptr, [&](auto biased) {
                    constexpr int M = decltype(m)::value, NN = decltype(nn)::value;
                    constexpr bool MASKED = masked, BIAS = biased;
                    static bool allowed[64] = {};
                    if (const int rc = allow_dynamic_lds(allowed, reinterpret_cast<const void *>(&k_search_lists<NN, M, MASKED, BIAS>),
                                                         lists_lds_bytes(64 * 256, kListMaxProbes)))
                        return rc;
                    hipLaunchKernelGGL((k_search_lists<NN, M, MASKED, BIAS>), dim3((unsigned)Q * (unsigned)p.parts), dim3(64 * kListWaves),
                                       p.lds, st, tables, Q, codes, M == kMetricIP ? nullptr : w, B, K, k, p.parts, li.list_offsets, li.L,
                                       li.probes, li.P, ws_s, ws_i, reinterpret_cast<const u64 *>(mask), li.bias);
                    return launch_rc();
                });
            });
        });
    });
}

// The tail of every top-k call, once its arguments have passed: the size of the workspace against the plan's, its split
// into scores, then positions, launch(ws_s, ws_i) -- a list of k entries per (query, part) --, and the merge of a query's
// lists into its result (wide: k_search_wide_merge of mcq_wide_kernels.h).  A plan without parts (no candidate anywhere)
// launches the merge alone, on no list: the fill of rule 4.
template <typename Launch>
int topk_tail(const PartPlan &p, void *workspace, size_t workspace_bytes, hipStream_t st, long Q, int k, float *out_score,
              int64_t *out_index, bool wide, Launch &&launch) {
    float *ws_s = nullptr;
    int *ws_i = nullptr;
    if (p.parts > 0) {
        if (workspace_bytes < p.ws_bytes) return MCQ_EWORKSPACE;
        ws_s = static_cast<float *>(workspace);
        ws_i = reinterpret_cast<int *>(static_cast<char *>(workspace) + p.ws_bytes / 2);
        if (const int rc = launch(ws_s, ws_i)) return rc;
    }
    if (wide)
        hipLaunchKernelGGL(k_search_wide_merge, dim3((unsigned)Q), dim3(64 * kWideWaves), 0, st, ws_s, ws_i, p.parts, k, out_score,
                           out_index);
    else
        hipLaunchKernelGGL(k_search_merge, dim3((unsigned)Q), dim3(64), 0, st, ws_s, ws_i, p.parts, k, out_score, out_index);
    return launch_rc();
}

// every top-k entry point: the scan over the whole store (rules 1-6 and 10-12), or list by list (li; rules 13-16)
int search_topk(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K, int k, int metric,
                const uint64_t *mask, const ListsIn *li, float *out_score, int64_t *out_index, void *workspace,
                size_t workspace_bytes, void *stream) {
    bool empty;
    if (const int rc = search_check(tables, Q, codes, w, B, N, K, k, metric, mask, li, Q == 0 || (out_score && out_index), workspace, &empty))
        return rc;
    if (Q == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ScanPlan sp = (empty || li) ? ScanPlan{} : scan_plan(Q, B, N, K, k);
    const PartPlan p = empty ? PartPlan{} : li ? lists_plan(Q, li->P, N, K, k) : PartPlan{sp.slices, sp.lds, sp.ws_bytes};
    return topk_tail(p, workspace, workspace_bytes, st, Q, k, out_score, out_index, false, [&](float *ws_s, int *ws_i) {
        return li ? launch_lists(p, st, tables, (int)Q, codes, w, B, N, K, k, metric, mask, *li, ws_s, ws_i)
                  : launch_scan(sp, st, tables, (int)Q, codes, w, B, N, K, k, metric, ws_s, ws_i, mask);
    });
}

// ---- the search past 64 neighbours (mcq_wide_kernels.h; rules 24-27 of include/mcq_wide.h; mirrored by wide_plan of
// tests/search_wide_grid.py): the parts of lists_plan, capped so that the merge of a query streams at most kWideMergeEntries
// entries per entry of its sorted half -- 128 parts up to k = 512 and 64 beyond (wide_merge_cap), where lists_plan alone
// would hand the merge of a single query 256 lists.  P is 1 for a call over the whole store.
PartPlan wide_plan(long Q, int P, int N, int K, int k) {
    const long cap = wide_merge_cap(k) < kScanMaxSlices ? wide_merge_cap(k) : kScanMaxSlices;
    const int parts = part_count(Q, kListTargetBlocks, cap);
    return {parts, (size_t)wide_lds_bytes(N * K, P, k), topk_ws_bytes(Q, parts, k)};
}

// search_check with the cap of this feature: k in 65 .. 1,024 passes where search_check tests k > 64, a larger one fails there
int wide_check(const float *tables, long Q, const void *codes, const float *w, long B, int N, int K, int k, int metric,
               const uint64_t *mask, const ListsIn *li, bool outs_ok, const void *workspace, bool *empty, int code_bytes = 1) {
    const int as = k > kWideMaxK ? 65 : (k > 64 ? 64 : k);
    return search_check(tables, Q, codes, w, B, N, K, as, metric, mask, li, outs_ok, workspace, empty, code_bytes);
}

// li.probes == NULL: the whole store as one list; a bias is a null test inside the kernel, not a flag.  T = uint16_t
// (mcq_search_topk_u16): the same plan, the two-byte instantiations
template <typename T>
int launch_wide(const PartPlan &p, hipStream_t st, const float *tables, int Q, const T *codes, const float *w, long B, int N,
                int K, int k, int metric, const uint64_t *mask, const ListsIn &li, float *ws_s, int *ws_i) {
    return pick<kMetricL2, kMetricIP, kMetricCos>(metric, [&](auto m) {
        return pick<1, 2, 4, 8, 16, 32, 64>(N, [&](auto nn) {
            return pick_bool(mask != nullptr, [&](auto masked) {
                constexpr int M = decltype(m)::value, NN = decltype(nn)::value;
                constexpr bool MASKED = masked;
                static bool allowed[64] = {};
                if (const int rc = allow_dynamic_lds(allowed, reinterpret_cast<const void *>(&k_search_wide<NN, M, MASKED, T>),
                                                     wide_lds_bytes(kTableRowsOf<T>, kListMaxProbes, kWideMaxK)))
                    return rc;
                hipLaunchKernelGGL((k_search_wide<NN, M, MASKED, T>), dim3((unsigned)Q * (unsigned)p.parts), dim3(64 * kWideWaves),
                                   p.lds, st, tables, Q, codes, M == kMetricIP ? nullptr : w, B, K, k, p.parts, li.list_offsets, li.L,
                                   li.probes, li.P, ws_s, ws_i, reinterpret_cast<const u64 *>(mask), li.bias);
                return launch_rc();
            });
        });
    });
}

// both wide entry points: over the whole store (li == NULL), or list by list.  T = uint16_t: mcq_search_topk_u16
template <typename T>
int search_wide(const float *tables, long Q, const T *codes, const float *w, long B, int N, int K, int k, int metric,
                const uint64_t *mask, const ListsIn *li, float *out_score, int64_t *out_index, void *workspace,
                size_t workspace_bytes, void *stream) {
    bool empty;
    if (const int rc = wide_check(tables, Q, codes, w, B, N, K, k, metric, mask, li, Q == 0 || (out_score && out_index), workspace, &empty,
                                  sizeof(T)))
        return rc;
    if (Q == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ListsIn &in = li ? *li : kWholeStore;
    const PartPlan p = empty ? PartPlan{} : wide_plan(Q, in.P, N, K, k);
    return topk_tail(p, workspace, workspace_bytes, st, Q, k, out_score, out_index, true, [&](float *ws_s, int *ws_i) {
        return launch_wide<T>(p, st, tables, (int)Q, codes, w, B, N, K, k, metric, mask, in, ws_s, ws_i);
    });
}

// ---- the exact re-ranking of a shortlist (mcq_rerank_kernels.h; rules 28-31 of include/mcq_rerank.h; mirrored by rerank_plan
// of tests/rerank_grid.py): one query per workgroup and `parts` parts of its shortlist row, cut by count of its steps of
// kRerankGroup entries -- as many as fill the chip once at small Q, no more than the row has steps, capped as wide_plan caps
// them for the merge.
PartPlan rerank_plan(long Q, long S, int D, int k) {
    const int parts = part_count(Q, kRerankTargetBlocks, wide_merge_cap(k), (S + kRerankGroup - 1) / kRerankGroup);
    return {parts, (size_t)rerank_lds_bytes(D, k), topk_ws_bytes(Q, parts, k)};
}

// the limits the calls over a shortlist share (rules 28 and 36), in their order, behind what the call says of its rows (D,
// or N and K); 0 inside the domain
int shortlist_limits(long Q, long S, long B, long Bs, int k, int metric) {
    constexpr long kLimit = 0x7fffffffL;                                   // sizes stay below 2^31 - 1
    if (k > kWideMaxK) return MCQ_EUNSUPPORTED;
    if (k < 1 || Q < 0 || S < 0 || B < 0 || Bs < 0) return MCQ_EINVAL;
    if (!metric_ok(metric)) return MCQ_EINVAL;
    if (Q >= kLimit || S >= kLimit || B >= kLimit || Bs >= kLimit) return MCQ_EUNSUPPORTED;
    return 0;
}

// rule 28's limits, in its order; 0 inside the domain.  A k past the cap is reported before a D below 1
int rerank_domain(long Q, long S, long B, long Bs, int D, int k, int metric) {
    if (D > kRerankMaxD) return MCQ_EUNSUPPORTED;
    if (D < 1 && k <= kWideMaxK) return MCQ_EINVAL;
    return shortlist_limits(Q, S, B, Bs, k, metric);
}

int launch_rerank(const PartPlan &p, hipStream_t st, const void *queries, bool qhalf, int Q, const void *vectors, bool xhalf,
                  long B, int D, const int64_t *shortlist, int S, const int64_t *row_of, long Bs, int k, int metric, int vec,
                  float *ws_s, int *ws_i) {
    return pick<kMetricL2, kMetricIP, kMetricCos>(metric, [&](auto m) {
        return pick_bool(qhalf, [&](auto qh) {
            return pick_bool(xhalf, [&](auto xh) {
                constexpr int M = decltype(m)::value;
                constexpr bool QH = qh, XH = xh;
                static bool allowed[64] = {};
                if (const int rc = allow_dynamic_lds(allowed, reinterpret_cast<const void *>(&k_rerank<QH, XH, M>),
                                                     rerank_lds_bytes(kRerankMaxD, kWideMaxK)))
                    return rc;
                hipLaunchKernelGGL((k_rerank<QH, XH, M>), dim3((unsigned)Q * (unsigned)p.parts), dim3(64 * kRerankWaves), p.lds, st,
                                   queries, vectors, B, D, shortlist, S, row_of, Bs, k, p.parts, vec, ws_s, ws_i);
                return launch_rc();
            });
        });
    });
}

int rerank(const void *queries, bool qhalf, long Q, const void *vectors, bool xhalf, long B, int D, const int64_t *shortlist,
           long S, const int64_t *row_of, long Bs, int k, int metric, float *out_score, int64_t *out_index, void *workspace,
           size_t workspace_bytes, void *stream) {
    if (!row_of) Bs = B;                                                   // (positions are rows)
    if (const int rc = rerank_domain(Q, S, B, Bs, D, k, metric)) return rc;
    if (Q > 0 && (!out_score || !out_index)) return MCQ_EINVAL;
    if (Q == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t qel = qhalf ? 2 : 4, xel = xhalf ? 2 : 4;
    PartPlan p{};                                                         // (no row can hold a candidate: the fill)
    if (S > 0 && B > 0 && Bs > 0) {
        if (!queries || !vectors || !shortlist || !workspace) return MCQ_EINVAL;
        if (reinterpret_cast<uintptr_t>(queries) % qel != 0 || reinterpret_cast<uintptr_t>(vectors) % xel != 0) return MCQ_EINVAL;
        if (reinterpret_cast<uintptr_t>(shortlist) % 8 != 0 || reinterpret_cast<uintptr_t>(row_of) % 8 != 0) return MCQ_EINVAL;
        p = rerank_plan(Q, S, D, k);
    }
    // one vector load per lane and trip where every row starts on its boundary: 16 bytes of fp32, 8 of fp16
    const int vec = D % 4 == 0 && reinterpret_cast<uintptr_t>(vectors) % (4 * xel) == 0;
    return topk_tail(p, workspace, workspace_bytes, st, Q, k, out_score, out_index, true, [&](float *ws_s, int *ws_i) {
        return launch_rerank(p, st, queries, qhalf, (int)Q, vectors, xhalf, B, D, shortlist, (int)S, row_of, Bs, k, metric, vec,
                             ws_s, ws_i);
    });
}

// ---- the search over a shortlist (mcq_shortlist_kernels.h; rules 36-39 of include/mcq_shortlist.h; mirrored by short_plan of
// tests/search_shortlist_grid.py): one query per workgroup and `parts` parts of its shortlist row, cut by count of its steps
// of kShortStep entries -- as many as fill the chip once at small Q, no more than the row has steps, capped as wide_plan caps
// them for the merge.
PartPlan short_plan(long Q, long S, int N, int K, int k) {
    const int parts = part_count(Q, kShortTargetBlocks, wide_merge_cap(k), (S + kShortStep - 1) / kShortStep);
    return {parts, (size_t)short_lds_bytes(N * K, k), topk_ws_bytes(Q, parts, k)};
}

// rule 36's limits, in its order; 0 inside the domain.  code_bytes: 1, or 2 for mcq_search_shortlist_u16
int short_domain(long Q, long S, long B, long Bs, int N, int K, int k, int metric, int code_bytes) {
    if (const int rc = code_bytes == 2 ? code16_domain(N, K, 1) : search_domain(N, K, 1)) return rc;
    return shortlist_limits(Q, S, B, Bs, k, metric);
}

template <typename T>
int launch_short(const PartPlan &p, hipStream_t st, const float *tables, int Q, const T *codes, const float *w, long B, int N,
                 int K, int k, int metric, const int64_t *shortlist, int S, const int64_t *row_of, long Bs, const float *bias,
                 float *ws_s, int *ws_i) {
    return pick<kMetricL2, kMetricIP, kMetricCos>(metric, [&](auto m) {
        return pick<1, 2, 4, 8, 16, 32, 64>(N, [&](auto nn) {
            constexpr int M = decltype(m)::value, NN = decltype(nn)::value;
            static bool allowed[64] = {};
            if (const int rc = allow_dynamic_lds(allowed, reinterpret_cast<const void *>(&k_search_short<NN, M, T>),
                                                 short_lds_bytes(kMaxRows, kWideMaxK)))
                return rc;
            hipLaunchKernelGGL((k_search_short<NN, M, T>), dim3((unsigned)Q * (unsigned)p.parts), dim3(64 * kWideWaves), p.lds, st,
                               tables, Q, codes, M == kMetricIP ? nullptr : w, B, K, k, p.parts, shortlist, S, row_of, Bs, bias,
                               ws_s, ws_i);
            return launch_rc();
        });
    });
}

// both entries of include/mcq_shortlist.h.  T = uint16_t: mcq_search_shortlist_u16
template <typename T>
int search_shortlist(const float *tables, long Q, const T *codes, const float *w, long B, int N, int K, int k, int metric,
                     const int64_t *shortlist, long S, const int64_t *row_of, long Bs, const float *bias, float *out_score,
                     int64_t *out_index, void *workspace, size_t workspace_bytes, void *stream) {
    if (!row_of) Bs = B;                                                   // (positions are rows)
    if (const int rc = short_domain(Q, S, B, Bs, N, K, k, metric, sizeof(T))) return rc;
    if (Q > 0 && (!out_score || !out_index)) return MCQ_EINVAL;
    if (Q == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    PartPlan p{};                                                         // (no row can hold a candidate: the fill)
    if (S > 0 && B > 0 && Bs > 0) {
        if (!tables || !codes || !shortlist || !workspace) return MCQ_EINVAL;
        if (!w_ok(w, metric) || !codes_aligned(codes, N, sizeof(T))) return MCQ_EINVAL;
        if (reinterpret_cast<uintptr_t>(shortlist) % 8 != 0 || reinterpret_cast<uintptr_t>(row_of) % 8 != 0) return MCQ_EINVAL;
        if (reinterpret_cast<uintptr_t>(bias) % 4 != 0) return MCQ_EINVAL;
        p = short_plan(Q, S, N, K, k);
    }
    return topk_tail(p, workspace, workspace_bytes, st, Q, k, out_score, out_index, true, [&](float *ws_s, int *ws_i) {
        return launch_short<T>(p, st, tables, (int)Q, codes, w, B, N, K, k, metric, shortlist, (int)S, row_of, Bs, bias, ws_s, ws_i);
    });
}

}  // namespace


// ---- range search over stored codes (mcq_range_kernels.h) ---------------------------------------------------------------
namespace {

// the two sweeps: one slot base per (wave, query) behind the tables in LDS, one int64 per (query, slice, wave) of workspace
struct RangePlan : TilePlan {
    size_t lds, ws_bytes;
};

RangePlan range_plan(long Q, long B, int N, int K) {
    RangePlan p{tile_plan(Q, B, N, K, kRangeWaves), 0, 0};
    p.lds = (size_t)p.qt * N * K * 4 + (size_t)kRangeWaves * p.qt * 8;
    p.ws_bytes = align256((size_t)Q * p.slices * kRangeWaves * 8);
    return p;
}

template <typename T>
struct RangeArgsT {
    const float *tables;
    int Q;
    const T *codes;
    const float *w;
    long B;
    int N, K, metric;
    const float *thr;
    int64_t *ws;
    const int64_t *lims;
    float *out_s;
    int64_t *out_i;
    long capacity;
    const uint64_t *mask;                                                 // NULL: none (rule 12)
};
using RangeArgs = RangeArgsT<uint8_t>;                                    // (uint16_t: the entries of include/mcq_code16.h)

// a sweep: FILL == false counts, FILL == true stores; a candidate's digits arrive in chunks of CH = min(N, 8)
template <bool FILL>
int launch_range(const RangePlan &p, hipStream_t st, const RangeArgs &a) {
    return pick<1, 2, 4, 8, 16>(p.qt, [&](auto qt) {
        return pick<1, 2, 4, 8>(a.N < 8 ? a.N : 8, [&](auto ch) {
            return pick_bool(a.mask != nullptr, [&](auto masked) {
                constexpr int QT = decltype(qt)::value, CH = decltype(ch)::value;
                constexpr bool MASKED = masked;
                static bool allowed[64] = {};
                if (const int rc = allow_dynamic_lds(allowed, reinterpret_cast<const void *>(&k_range_sweep<QT, CH, FILL, MASKED>),
                                                     kScanTableLds + kRangeWaves * kScanQTMax * 8))
                    return rc;
                hipLaunchKernelGGL((k_range_sweep<QT, CH, FILL, MASKED>), dim3((unsigned)p.qtiles * (unsigned)p.slices),
                                   dim3(64 * kRangeWaves), p.lds, st, a.tables, a.Q, a.codes, a.w, a.B, a.N, a.K, a.metric, p.slices,
                                   p.per_slice, a.thr, a.ws, a.lims, a.out_s, a.out_i, a.capacity, reinterpret_cast<const u64 *>(a.mask));
                return launch_rc();
            });
        });
    });
}

// the range search list by list (rules 17-20; mirrored by range_lists_plan of tests/search_range_lists_grid.py): the parts of
// lists_plan, the LDS of k_search_lists, one int64 per (query, part, wave) of workspace
PartPlan range_lists_plan(long Q, int P, int N, int K) {
    const int parts = part_count(Q, kListTargetBlocks, kScanMaxSlices);
    return {parts, (size_t)lists_lds_bytes(N * K, P), align256((size_t)Q * parts * kRangeListWaves * 8)};
}

// (a bias, li.bias != NULL, is a flag here as in launch_lists.)  T = uint16_t (mcq_search_range_u16_count / _fill): the same
// plan, the two-byte instantiations, and li.probes == NULL for the whole store as one list
template <bool FILL, typename T>
int launch_range_lists(const PartPlan &p, hipStream_t st, const RangeArgsT<T> &a, const ListsIn &li) {
    return pick<1, 2, 4, 8>(a.N < 8 ? a.N : 8, [&](auto ch) {
        return pick_bool(a.mask != nullptr, [&](auto masked) {
            return pick_bool(li.bias != nullptr, [&](auto biased) {
                constexpr int CH = decltype(ch)::value;
                constexpr bool MASKED = masked, BIAS = biased;
                static bool allowed[64] = {};
                if (const int rc = allow_dynamic_lds(allowed, reinterpret_cast<const void *>(&k_range_lists<CH, FILL, MASKED, BIAS, T>),
                                                     lists_lds_bytes(kTableRowsOf<T>, kListMaxProbes)))
                    return rc;
                hipLaunchKernelGGL((k_range_lists<CH, FILL, MASKED, BIAS, T>), dim3((unsigned)a.Q * (unsigned)p.parts),
                                   dim3(64 * kRangeListWaves), p.lds, st, a.tables, a.codes, a.w, a.B, a.N, a.K, a.metric, p.parts,
                                   li.list_offsets, li.L, li.probes, li.P, a.thr, a.ws, a.lims, a.out_s, a.out_i, a.capacity,
                                   reinterpret_cast<const u64 *>(a.mask), li.bias);
                return launch_rc();
            });
        });
    });
}

// rules 9 and 19: what every range entry point rejects -- search_check without k (lims is written even by an empty call),
// then thr and the size of the workspace; nothing touches the device
// code_bytes == 2: a call over the whole store is one list too (launch_range_any), and sized so
int range_check(const float *tables, long Q, const void *codes, const float *w, long B, int N, int K, int metric,
                const uint64_t *mask, const ListsIn *li, const float *thr, const int64_t *lims, const void *workspace,
                size_t workspace_bytes, bool *empty, int code_bytes = 1) {
    if (const int rc = search_check(tables, Q, codes, w, B, N, K, 1, metric, mask, li, lims != nullptr, workspace, empty, code_bytes))
        return rc;
    if (*empty) return 0;
    if (!thr) return MCQ_EINVAL;                     // (after w and the alignment: all three are MCQ_EINVAL, no code moved)
    const size_t need = (li || code_bytes == 2) ? range_lists_plan(Q, li ? li->P : 1, N, K).ws_bytes : range_plan(Q, B, N, K).ws_bytes;
    if (workspace_bytes < need) return MCQ_EWORKSPACE;
    return 0;
}

// the launch of one sweep, over the whole store or list by list (li).  *per: the workspace entries of a query.  Two-byte
// codes go list by list always, the whole store as one list.
template <bool FILL, typename T>
int launch_range_any(hipStream_t st, const RangeArgsT<T> &a, const ListsIn *li, int *per = nullptr) {
    if constexpr (sizeof(T) == 1) {
        if (!li) {
            const RangePlan p = range_plan(a.Q, a.B, a.N, a.K);
            if (per) *per = p.slices * kRangeWaves;
            return launch_range<FILL>(p, st, a);
        }
    }
    const ListsIn &in = li ? *li : kWholeStore;
    const PartPlan p = range_lists_plan(a.Q, in.P, a.N, a.K);
    if (per) *per = p.parts * kRangeListWaves;
    return launch_range_lists<FILL, T>(p, st, a, in);
}

// every count entry point: the COUNT sweep, the counts -> offsets per query, the totals -> lims
template <typename T>
int range_count(const float *tables, long Q, const T *codes, const float *w, long B, int N, int K, int metric,
                const uint64_t *mask, const ListsIn *li, const float *thr, int64_t *lims, void *workspace, size_t workspace_bytes,
                void *stream) {
    bool empty;
    if (const int rc = range_check(tables, Q, codes, w, B, N, K, metric, mask, li, thr, lims, workspace, workspace_bytes, &empty, sizeof(T)))
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!empty) {
        int64_t *ws = static_cast<int64_t *>(workspace);
        const RangeArgsT<T> a{tables, (int)Q, codes, metric == MCQ_SEARCH_IP ? nullptr : w, B, N, K, metric, thr, ws, nullptr,
                              nullptr, nullptr, 0, mask};
        int per = 0;
        if (const int rc = launch_range_any<false>(st, a, li, &per)) return rc;
        hipLaunchKernelGGL(k_range_offsets, dim3((unsigned)Q), dim3(64), 0, st, ws, per, lims);
        if (const int rc = launch_rc()) return rc;
    }
    hipLaunchKernelGGL(k_range_lims, dim3(1), dim3(64), 0, st, lims, Q, empty ? 1 : 0);
    return launch_rc();
}

// every fill entry point: the FILL sweep into out_score / out_index, `capacity` entries each
template <typename T>
int range_fill(const float *tables, long Q, const T *codes, const float *w, long B, int N, int K, int metric,
               const uint64_t *mask, const ListsIn *li, const float *thr, const int64_t *lims, float *out_score, int64_t *out_index,
               long capacity, void *workspace, size_t workspace_bytes, void *stream) {
    bool empty;
    if (const int rc = range_check(tables, Q, codes, w, B, N, K, metric, mask, li, thr, lims, workspace, workspace_bytes, &empty, sizeof(T)))
        return rc;
    if (capacity < 0) return MCQ_EINVAL;
    if (empty || capacity == 0) return 0;                                  // nothing can be stored
    if (!out_score || !out_index) return MCQ_EINVAL;
    const RangeArgsT<T> a{tables, (int)Q, codes, metric == MCQ_SEARCH_IP ? nullptr : w, B, N, K, metric, thr,
                          static_cast<int64_t *>(workspace), lims, out_score, out_index, capacity, mask};
    return launch_range_any<true>(static_cast<hipStream_t>(stream), a, li);
}

}  // namespace

// ---- mcq_decode: a predicate and a launcher per path.  The paths are tried in the order below; the generic kernel takes the rest
namespace {
struct DecodeArgs {
    const void *codes;
    int code_bytes, codes_per_row, rep;       // rep = N / codes_per_row: codebooks that share a code (the generic kernel only)
    long B;
    const float *C;                           // the scaled centers [N * K][Dp]
    int N, K, D, Dp;
    float *out;
    hipStream_t st;
    // hooks: MCQ_DECODE_SLICED=0 (latched on first use) leaves the per-vector kernels only; MCQ_DECODE_BLK=0 skips the block-staged
    // kernel; MCQ_DECODE_LDS_MIN=<n> moves the batch size from which a codebook slice is staged in LDS (both read per call)
    bool sliced_ok, blk_on;
    long lds_min_b;
};

// block-staged LDS-resident kernel (k_decode_blk): packed byte codes, 4, 8 or 16 per vector, 64-byte slices when they fit the
// LDS beside the two code buffers, 32-byte slices otherwise (16 x 256)
constexpr size_t kDecBlkLdsMax = 160 * 1024, kDecBlkCodeBytes = 2 * 16384;
int decode_blk_lpv(int N, int K) {        // lanes per vector: 4 (64-byte slices), 2 (32-byte slices), 0: neither fits
    if ((size_t)N * K * 64 + kDecBlkCodeBytes <= kDecBlkLdsMax) return 4;
    return (size_t)N * K * 32 + kDecBlkCodeBytes <= kDecBlkLdsMax ? 2 : 0;
}
bool decode_blk_applies(const DecodeArgs &a) {
    return a.blk_on && a.sliced_ok && a.rep == 1 && a.code_bytes == 1 && a.B >= a.lds_min_b && a.K >= 32 && (a.D & 3) == 0 &&
           decode_blk_lpv(a.N, a.K) != 0 && (a.N == 4 || a.N == 8 || a.N == 16) &&
           ((reinterpret_cast<uintptr_t>(a.codes) & 15) == 0) && ((reinterpret_cast<uintptr_t>(a.out) & 15) == 0);
}
int launch_decode_blk(const DecodeArgs &a) {
    return pick<4, 8, 16>(a.N, [&](auto nn) {
        return pick<4, 2>(decode_blk_lpv(a.N, a.K), [&](auto ll) {
            constexpr int NN = decltype(nn)::value, LL = decltype(ll)::value, W = 4 * LL;
            static bool allowed[64] = {};
            if (const int rc = allow_dynamic_lds(allowed, reinterpret_cast<const void *>(&k_decode_blk<NN, LL>), (int)kDecBlkLdsMax)) return rc;
            const int ns = a.Dp / W, per_xcd = (ns + 7) / 8;
            int groups = 256 / (8 * per_xcd);            // one workgroup per CU
            groups = groups < 1 ? 1 : groups;
            const long per = (((a.B + groups - 1) / groups) + 255) / 256 * 256;
            hipLaunchKernelGGL((k_decode_blk<NN, LL>), dim3((unsigned)(8 * per_xcd * groups)), dim3(1024),
                               (size_t)a.N * a.K * W * 4 + kDecBlkCodeBytes, a.st, static_cast<const uint8_t *>(a.codes), a.B, a.C, a.K, a.D,
                               a.Dp, groups, per, a.out);
            return launch_rc();
        });
    });
}

// LDS-resident kernel: batches of >= 16,384 vectors whose codebook slice (N*K*64 B) fits the LDS
// (N >= 8: with fewer rows per vector the L2 gathers of the sliced kernel measured faster; 36.9 vs 52.2 us at 8 x 256, 65,536 vectors)
bool decode_lds_applies(const DecodeArgs &a) {
    return a.sliced_ok && a.rep == 1 && a.B >= a.lds_min_b && (size_t)a.N * a.K * 64 <= 144 * 1024 && a.K >= 32 && a.N >= 8;
}
template <typename T>
int launch_decode_lds(const DecodeArgs &a) {
    const int ns = a.Dp / 16, per_xcd = (ns + 7) / 8;
    int groups = 256 / (8 * per_xcd);            // one workgroup per CU
    groups = groups < 1 ? 1 : groups;
    hipLaunchKernelGGL((k_decode_lds<T>), dim3((unsigned)(8 * per_xcd * groups)), dim3(1024), (size_t)a.N * a.K * 64, a.st,
                       static_cast<const T *>(a.codes), a.B, a.C, a.N, a.K, a.D, a.Dp, groups, a.out);
    return launch_rc();
}

// XCD-sliced kernel: unpacked codes, batches big enough to fill the chip (16-entry codebooks: the per-vector kernels measured
// faster), rows that 8 slices x at most 64 lanes x 4 floats cover
int decode_sliced_lpv(int Dp) {
    int lpv = 4;
    while (lpv * 32 < Dp) lpv *= 2;          // 8 slices x lpv lanes x 4 floats cover Dp
    return lpv;
}
bool decode_sliced_applies(const DecodeArgs &a) {
    return a.sliced_ok && a.rep == 1 && a.B >= 4096 && a.K >= 32 && decode_sliced_lpv(a.Dp) <= 64;
}
// rows [at, at + rows) of a call as a call of their own: the per-vector kernels go through launch_in_pieces
inline DecodeArgs decode_piece(const DecodeArgs &a, long at, long rows) {
    DecodeArgs p = a;
    p.codes = static_cast<const char *>(a.codes) + at * a.codes_per_row * a.code_bytes;
    p.out = a.out + at * a.D;
    p.B = rows;
    return p;
}

template <typename T>
int launch_decode_sliced(const DecodeArgs &whole) {
    const int lpv = decode_sliced_lpv(whole.Dp), vpw = 64 / lpv;
    return launch_in_pieces(whole.B, 8 * lpv, [&](long at, long rows) {           // 8 slices x lpv lanes per vector
        const DecodeArgs a = decode_piece(whole, at, rows);
        const dim3 g((unsigned)(((a.B + 4 * vpw - 1) / (4 * vpw)) * 8));
        return pick<4, 8, 16>(a.N <= 4 ? 4 : (a.N <= 8 ? 8 : 16), [&](auto ch) {      // codes of a vector per load
            return pick<4, 8, 16, 32, 64>(lpv, [&](auto ll) {
                constexpr int CHH = decltype(ch)::value, LL = decltype(ll)::value;
                hipLaunchKernelGGL((k_decode_sliced<T, CHH, LL>), g, dim3(256), 0, a.st, static_cast<const T *>(a.codes), a.B, a.C, a.N, a.K,
                                   a.D, a.Dp, a.out);
                return launch_rc();
            });
        });
    });
}

// register kernel (k_decode_reg<N, J>): one-byte codes of 2, 4, 8 or 16 codebooks, J = float4s per lane of a row
constexpr Pair kDecRegShapes[] = {{8, 2}, {8, 1}, {4, 1}, {4, 2}, {4, 4}, {16, 1}, {16, 2}, {2, 1}, {2, 2}};
inline int decode_reg_j(const DecodeArgs &a) { return (a.Dp / 4 + 63) / 64; }
bool decode_reg_applies(const DecodeArgs &a) {
    return a.code_bytes == 1 && a.rep == 1 && in_pairs(kDecRegShapes, a.N, decode_reg_j(a));
}
int launch_decode_reg(const DecodeArgs &whole) {
    return pick_pair<kDecRegShapes>(whole.N, decode_reg_j(whole), [&](auto nn, auto jj) {
        constexpr int NN = nn, JJ = jj;
        return launch_in_pieces(whole.B, 64, [&](long at, long rows) {            // one wave per vector
            const DecodeArgs a = decode_piece(whole, at, rows);
            hipLaunchKernelGGL((k_decode_reg<NN, JJ>), dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, a.st,
                               static_cast<const uint8_t *>(a.codes), a.B, a.C, a.K, a.D, a.Dp, a.out);
            return launch_rc();
        });
    });
}

template <typename T>
int launch_decode_generic(const DecodeArgs &whole) {
    return launch_in_pieces(whole.B, 64, [&](long at, long rows) {                // one wave per vector
        const DecodeArgs a = decode_piece(whole, at, rows);
        hipLaunchKernelGGL((k_decode<T>), dim3((unsigned)((a.B + 3) / 4)), dim3(256), 0, a.st, static_cast<const T *>(a.codes),
                           a.codes_per_row, a.B, a.C, a.N, a.K, a.D, a.Dp, a.out);
        return launch_rc();
    });
}
}  // namespace


extern "C" {

int mcq_abi_version(void) { return MCQ_ABI_VERSION; }

int mcq_padded_dim(int D) { return round_up16(D); }

size_t mcq_prepared_bytes(int N, int K, int D) {
    if (N <= 0 || K <= 0 || D <= 0) return 0;
    return prepared_layout(N, K, D).total;
}

static int prepare_impl(const float *centers, float cscale_exp, const float *scales_dev, const float *weight,
                        const float *bias, int N, int K, int D, void *prepared, void *stream, const float *raw_cs = nullptr,
                        const float *raw_ls = nullptr, float speed = 0.f, float *scales_out2 = nullptr) {
    if (!domain_ok(N, K, D)) return domain_err(N, K, D);
    if (!centers || !prepared || ((weight == nullptr) != (bias == nullptr))) return MCQ_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Prepared P = prepared_view(prepared, N, K, D);       // (filled here: writable() below)
    const long rows = (long)N * K;
    const int Dp = round_up16(D);
    hipLaunchKernelGGL(k_prepare_rows, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, centers, cscale_exp, 1, rows, D, Dp,
                       writable(P.C), static_cast<float *>(nullptr) /* Q: of the centered rows, below */, scales_dev,
                       (scales_dev || raw_cs) ? writable(P.scales) : static_cast<float *>(nullptr), raw_cs, raw_ls, speed, scales_out2);
    if (const int rc = launch_rc()) return rc;
    if (!weight) return 0;      // decode only: the scaled centers are all mcq_decode reads (mcq_prepared_decode_bytes)
    hipLaunchKernelGGL(k_centers_mean, dim3((unsigned)(Dp / 16)), dim3(1024), 0, st, P.C, N, K, Dp, writable(P.mean), writable(P.cmean));
    if (const int rc = launch_rc()) return rc;
    // the scaled centers and the classifier rows as limb planes (the tables of the fixed-point products), one launch; the
    // bias rides along
    // (the centers enter every table of the search with their codebook's mean taken out -- oracle "TABLE FORM", centering; their
    // sums of squares Q come out of the same pass)
    if (const int rc = launch_fix_rows2(
            fix_rows_args(P.C, 0, rows, Dp, Dp, writable(P.Cf), writable(P.Ce), writable(P.Q), nullptr, nullptr, P.cmean, K, Dp),
            fix_rows_args(weight, 0, rows, D, D, writable(P.Wf), writable(P.We), nullptr, bias, writable(P.bias), nullptr, 0, 0, P.mean,
                          writable(P.wmu)), st))
        return rc;
    // Gram matrix of the scaled centers: the x.C product with the centers themselves as the frames
    // (the dense E / R kernels RELY on G[r][c] == G[c][r] bit for bit, mcq_tf_kernels.h: fixdot sums the same integer limb
    // products for (r, c) and (c, r), and the exponent ea + eb commutes; tests/test_gpu_er_dense.py compares G with its transpose)
    return launch_xc(P.Cf, P.Ce, rows, P.Cf, P.Ce, rows, D, writable(P.G), st);
}

size_t mcq_prepared_decode_bytes(int N, int K, int D) {
    if (N <= 0 || K <= 0 || D <= 0) return 0;
    return prepared_layout(N, K, D).offCf;      // scaled centers + their sums of squares
}

size_t mcq_prepared_mean_offset(int N, int K, int D) {
    if (N <= 0 || K <= 0 || D <= 0) return 0;
    return prepared_layout(N, K, D).offMean;
}

int mcq_prepare(const float *centers, float cscale_exp, const float *weight, const float *bias, int N, int K, int D,
                void *prepared, void *stream) {
    return prepare_impl(centers, cscale_exp, nullptr, weight, bias, N, K, D, prepared, stream);
}

int mcq_prepare_dev(const float *centers, const float *scales_exp, const float *weight, const float *bias, int N,
                    int K, int D, void *prepared, void *stream) {
    if (!scales_exp) return MCQ_EINVAL;
    return prepare_impl(centers, 1.0f, scales_exp, weight, bias, N, K, D, prepared, stream);
}

int mcq_prepare_params(const float *centers, const float *centers_scale, const float *logits_scale, float speed,
                       const float *weight, const float *bias, int N, int K, int D, void *prepared, float *scales_exp_out,
                       void *stream) {
    if (!centers_scale || !logits_scale) return MCQ_EINVAL;
    return prepare_impl(centers, 1.0f, nullptr, weight, bias, N, K, D, prepared, stream, centers_scale, logits_scale, speed,
                        scales_exp_out);
}

size_t mcq_encode_workspace_bytes(long B, int N, int K, int D) {
    if (B <= 0 || N <= 0 || K <= 0 || D <= 0 || !domain_ok(N, K, D)) return 48 * 256;
    const long dc = default_chunk(N, K, D), chunk = B < dc ? B : dc;
    return workspace_slack(N, K, D) + workspace_per_vector(N, K, D) * (size_t)chunk;
}

int mcq_encode(const float *x, long B, const void *prepared, float lscale_exp, int N, int K, int D, int refine_iters,
               uint8_t *out_u8, int64_t *out_i64, void *workspace, size_t workspace_bytes, void *stream) {
    return run_encode(x, B, prepared, lscale_exp, N, K, D, refine_iters, out_u8, out_i64, workspace,
                      workspace_bytes, static_cast<hipStream_t>(stream), nullptr);
}

int mcq_encode_ex(const float *x, long B, const void *prepared, float lscale_exp, int N, int K, int D,
                  int refine_iters, uint8_t *out_u8, int64_t *out_i64, void *workspace, size_t workspace_bytes,
                  void *stream, unsigned flags) {
    return run_encode(x, B, prepared, lscale_exp, N, K, D, refine_iters, out_u8, out_i64, workspace,
                      workspace_bytes, static_cast<hipStream_t>(stream), nullptr, nullptr, flags);
}

int mcq_refine_indexes(const float *x, long B, const void *prepared, int N, int K, int D, int refine_iters,
                       const int64_t *idx_in, int64_t *idx_out, void *workspace, size_t workspace_bytes,
                       void *stream) {
    if (B > 0 && (!idx_in || !idx_out)) return MCQ_EINVAL;
    return run_encode(x, B, prepared, 1.0f, N, K, D, refine_iters, nullptr, idx_out, workspace, workspace_bytes,
                      static_cast<hipStream_t>(stream), nullptr, B > 0 ? idx_in : nullptr);
}

int mcq_decode(const void *codes, int code_bytes, int codes_per_row, long B, const void *prepared, int N, int K, int D,
               float *out, void *stream) {
    if (!domain_ok(N, K, D)) return domain_err(N, K);
    if (B < 0 || codes_per_row <= 0 || N % codes_per_row != 0) return MCQ_EINVAL;
    const int rep = N / codes_per_row;
    if (!(rep == 1 || rep == 2 || rep == 4 || rep == 8 || rep == 16)) return MCQ_EINVAL;
    if (code_bytes != 1 && code_bytes != 8) return MCQ_EINVAL;
    if (B == 0) return 0;
    if (!codes || !prepared || !out) return MCQ_EINVAL;
    static const bool sliced_ok = !(getenv("MCQ_DECODE_SLICED") && atoi(getenv("MCQ_DECODE_SLICED")) == 0);
    const char *blk_env = getenv("MCQ_DECODE_BLK"), *lds_env = getenv("MCQ_DECODE_LDS_MIN");
    const DecodeArgs a{codes, code_bytes, codes_per_row, rep, B, prepared_view(prepared, N, K, D).C, N, K, D, round_up16(D), out,
                       static_cast<hipStream_t>(stream), sliced_ok, (blk_env ? atoi(blk_env) : 1) != 0, lds_env ? atol(lds_env) : 16384};
    const bool u8 = code_bytes == 1;
    if (decode_blk_applies(a)) return launch_decode_blk(a);
    if (decode_lds_applies(a)) return u8 ? launch_decode_lds<uint8_t>(a) : launch_decode_lds<int64_t>(a);
    if (decode_sliced_applies(a)) return u8 ? launch_decode_sliced<uint8_t>(a) : launch_decode_sliced<int64_t>(a);
    if (decode_reg_applies(a)) return launch_decode_reg(a);
    return u8 ? launch_decode_generic<uint8_t>(a) : launch_decode_generic<int64_t>(a);
}

int mcq_decode_backward(const float *grad_out, const int64_t *idx, long B, int N, int K, int D, float *gC,
                        void *stream) {
    if (N <= 0 || K <= 0 || D <= 0 || B < 0 || !gC) return MCQ_EINVAL;
    if (B > 0 && (!grad_out || !idx)) return MCQ_EINVAL;
    return launch_decode_backward<int64_t>(grad_out, idx, B, N, K, D, gC, (long)D, 0L, N, static_cast<hipStream_t>(stream));
}

int mcq_decode_backward_u8(const float *grad_out, const uint8_t *codes, long B, int N, int K, int D, float *gC,
                           void *stream) {
    if (K > 256) return MCQ_EUNSUPPORTED;       // (byte codes: the trainer's entry points stay at K <= 256, include/mcq.h)
    if (N <= 0 || K <= 0 || D <= 0 || B < 0 || !gC) return MCQ_EINVAL;
    if (B > 0 && (!grad_out || !codes)) return MCQ_EINVAL;
    return launch_decode_backward<uint8_t>(grad_out, codes, B, N, K, D, gC, (long)D, 0L, N, static_cast<hipStream_t>(stream));
}

int mcq_scatter_rows(const float *grad, long stride_b, long stride_n, const int64_t *idx, int idx_stride, long B, int N,
                     int K, int D, float *out, void *stream) {
    if (N <= 0 || K <= 0 || D <= 0 || B < 0 || !out || idx_stride < N) return MCQ_EINVAL;
    if (B > 0 && (!grad || !idx)) return MCQ_EINVAL;
    return launch_decode_backward<int64_t>(grad, idx, B, N, K, D, out, stride_b, stride_n, idx_stride, static_cast<hipStream_t>(stream));
}

int mcq_jcl_prefix_fwd(const float *hp, const float *emb, const int64_t *idx, long B, int N, int K, int H, float scale,
                       float *A, void *stream) {
    if (N < 2 || K < 1 || H < 1 || B < 0) return MCQ_EINVAL;
    if (B == 0) return 0;
    if (!hp || !emb || !idx || !A) return MCQ_EINVAL;
    hipLaunchKernelGGL(k_jcl_prefix_fwd, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), hp,
                       emb, idx, B, N, K, H, scale, A);
    return launch_rc();
}

int mcq_jcl_prefix_bwd(const float *A, const float *gA, long B, int N, int H, float scale, float *g_hp, float *gE,
                       void *stream) {
    if (N < 2 || H < 1 || B < 0) return MCQ_EINVAL;
    if (B == 0) return 0;
    if (!A || !gA || !g_hp || !gE) return MCQ_EINVAL;
    hipLaunchKernelGGL(k_jcl_prefix_bwd, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), A,
                       gA, B, N, H, scale, g_hp, gE);
    return launch_rc();
}

namespace {
// workspace of the logits entry points: arg max bytes, then the frames as limb planes and their exponents
struct LogitsWs {
    uint8_t *idx8;
    int8_t *xf;
    int *xe;
    size_t total;
};
LogitsWs logits_ws(void *ws, long B, int N, int D) {
    char *p = static_cast<char *>(ws);
    const size_t o1 = align256((size_t)B * N), o2 = align256(o1 + fix_plane_bytes(B, D));
    return LogitsWs{reinterpret_cast<uint8_t *>(p), reinterpret_cast<int8_t *>(p + o1), reinterpret_cast<int *>(p + o2),
                    align256(o2 + (size_t)fix_round_rows(B) * 4)};
}
}  // namespace

size_t mcq_logits_workspace_bytes(long B, int N, int D) {
    if (B <= 0 || N <= 0 || D <= 0) return 256;
    return logits_ws(nullptr, B, N, D).total;
}

// frames to limb planes, then the stored logits (and, with idx8, the arg max bytes): what the two entry points below share
static int run_logits(const float *x, long B, const void *prepared, float lscale_exp, int N, int K, int D, float *out, uint8_t *idx8,
                      const LogitsWs &w, hipStream_t st, unsigned flags) {
    const Prepared P = prepared_view(prepared, N, K, D);
    // (the logits product reads centered frames: FixGemm::wmu)
    if (const int rc = launch_fix_rows(x, (flags & MCQ_ENCODE_X_FP16) ? 1 : 0, B, D, D, w.xf, w.xe, nullptr, st, P.mean)) return rc;
    return launch_logits(w.xf, w.xe, B, P, N, K, D, lscale_exp, (flags & MCQ_ENCODE_LSCALE_FROM_PREPARED) ? P.scales + 1 : nullptr, out,
                         idx8, st);
}

int mcq_logits(const float *x, long B, const void *prepared, float lscale_exp, int N, int K, int D, float *out,
               void *workspace, size_t workspace_bytes, void *stream) {
    if (!domain_ok(N, K, D)) return MCQ_EUNSUPPORTED;        // (for ANY shape outside the domain, N = 3 included)
    if (B == 0) return 0;
    if (!x || !prepared || !out || B < 0 || !workspace) return MCQ_EINVAL;
    if (workspace_bytes < mcq_logits_workspace_bytes(B, N, D)) return MCQ_EWORKSPACE;
    return run_logits(x, B, prepared, lscale_exp, N, K, D, out, nullptr, logits_ws(workspace, B, N, D), static_cast<hipStream_t>(stream), 0);
}

int mcq_test_prepared_layout(int N, int K, int D, size_t *offsets_out, int cap) {
    if (!domain_ok(N, K, D)) return domain_err(N, K, D);
    if (!offsets_out || cap < 0) return MCQ_EINVAL;
    const PreparedLayout l = prepared_layout(N, K, D);
    const size_t offs[] = {l.offC, l.offQ, l.offCf, l.offCe, l.offWf, l.offWe, l.offWmu, l.offBias, l.offScales, l.offMean,
                           l.offCMean, l.offG, l.total};
    constexpr int n = (int)(sizeof(offs) / sizeof(offs[0]));
    for (int i = 0; i < n && i < cap; ++i) offsets_out[i] = offs[i];
    return n;
}

// include/mcq_probe.h: E / R of B slots through launch_tf_er, in the form asked for
size_t mcq_test_er_workspace_bytes(long B, int N) { return (B > 0 && N > 0) ? align256((size_t)B * N * N * 4) : 256; }

int mcq_test_er(const void *prepared, int N, int K, int D, const float *xc, const float *xx, const uint8_t *idx, long B,
                const int *nact, const int *map, int form, float *E_out, float *R_out, void *workspace, size_t workspace_bytes,
                void *stream) {
    if (!domain_ok(N, K, D)) return domain_err(N, K, D);
    if (K > 256) return MCQ_EUNSUPPORTED;
    if (B < 0 || (form != 0 && form != 1)) return MCQ_EINVAL;
    if (B == 0) return 0;
    if (!prepared || !xc || !xx || !idx || !E_out || !R_out || !workspace) return MCQ_EINVAL;
    if (reinterpret_cast<uintptr_t>(idx) % 16 != 0 || reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return MCQ_EINVAL;
    if (workspace_bytes < mcq_test_er_workspace_bytes(B, N)) return MCQ_EWORKSPACE;
    const Prepared P = prepared_view(prepared, N, K, D);
    return launch_tf_er<uint8_t>(N, P.G, xc, idx, xx, B, K, E_out, R_out, static_cast<float *>(workspace), B, nact, map,
                                 static_cast<hipStream_t>(stream), form);
}

// the x.C product as run_encode forms it for a chunk: launch_fix_rows with P.mean (which also leaves |x - mean|^2 where
// `xx` asks for it), then launch_xc
static int test_xc(const float *x, long B, const void *prepared, int N, int K, int D, float *out, float *xx, void *workspace,
                   size_t workspace_bytes, void *stream, unsigned flags) {
    if (!domain_ok(N, K, D)) return MCQ_EUNSUPPORTED;
    if (B == 0) return 0;
    if (!x || !prepared || !out || B < 0 || !workspace || (flags & ~MCQ_ENCODE_X_FP16)) return MCQ_EINVAL;
    if (workspace_bytes < mcq_logits_workspace_bytes(B, N, D)) return MCQ_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Prepared P = prepared_view(prepared, N, K, D);
    const LogitsWs w = logits_ws(workspace, B, N, D);
    if (const int rc = launch_fix_rows(x, (flags & MCQ_ENCODE_X_FP16) ? 1 : 0, B, D, D, w.xf, w.xe, xx, st, P.mean)) return rc;
    return launch_xc(w.xf, w.xe, B, P.Cf, P.Ce, (long)N * K, D, out, st);
}

int mcq_test_xc(const float *x, long B, const void *prepared, int N, int K, int D, float *out, void *workspace,
                size_t workspace_bytes, void *stream, unsigned flags) {
    return test_xc(x, B, prepared, N, K, D, out, nullptr, workspace, workspace_bytes, stream, flags);
}

// include/mcq_probe.h: mcq_test_xc with the frames' |x - mean|^2 as well
int mcq_test_xc_xx(const float *x, long B, const void *prepared, int N, int K, int D, float *xc_out, float *xx_out, void *workspace,
                   size_t workspace_bytes, void *stream, unsigned flags) {
    if (B > 0 && !xx_out) return MCQ_EINVAL;
    return test_xc(x, B, prepared, N, K, D, xc_out, xx_out, workspace, workspace_bytes, stream, flags);
}

// include/mcq_probe.h: where carve() puts every array of one chunk of B vectors
int mcq_test_pass_layout(long B, int N, int K, int D, size_t *out, int cap) {
    if (!domain_ok(N, K, D)) return domain_err(N, K, D);
    if (B < 1 || !out || cap < 0) return MCQ_EINVAL;
    CarveExtents e;
    const TfLists tf = K > 256 ? carve<uint16_t>(nullptr, B, N, K, D, &e).tf : carve<uint8_t>(nullptr, B, N, K, D, &e).tf;
    constexpr int n = 2 * CV_COUNT + kTfLevels + 2;
    static_assert(n == MCQ_TEST_PASS_LAYOUT_VALUES, "include/mcq_probe.h");
    size_t v[n];
    for (int i = 0; i < CV_COUNT; ++i) { v[2 * i] = e.off[i]; v[2 * i + 1] = e.bytes[i]; }
    for (int i = 0; i < kTfLevels; ++i) v[2 * CV_COUNT + i] = (size_t)tf.kc[i];
    v[n - 2] = code_bytes_of(K);
    v[n - 1] = e.total;
    for (int i = 0; i < n && i < cap; ++i) out[i] = v[i];
    return n;
}

// include/mcq_lanes.h: the chunk plan run_encode_t takes for this batch and workspace (host only: nothing touches a device, so
// neither a capturing stream nor a missing side stream is seen here)
int mcq_test_chunk_plan(long B, int N, int K, int D, size_t workspace_bytes, int lanes, long *out, int cap) {
    if (!domain_ok(N, K, D)) return domain_err(N, K, D);
    if (B < 1 || lanes < 0 || lanes > kMaxLanes || !out || cap < 0) return MCQ_EINVAL;
    const size_t per = workspace_per_vector(N, K, D);
    ChunkPlan p;
    bool two = lanes == 0 ? (encode_lanes() == 2 && B >= encode_lanes_min()) : lanes == 2;
    if (two) two = plan_two_lanes(B, workspace_bytes, per, lane_slack(D), &p);
    if (!two && !plan_one_lane(B, workspace_bytes, per, lane_slack(D), &p)) return MCQ_EWORKSPACE;
    const long head[MCQ_TEST_CHUNK_PLAN_HEAD] = {p.lanes, p.chunk, p.chunks, (long)p.lane_off[0], (long)p.lane_off[1], (long)p.lane_bytes};
    for (int i = 0; i < MCQ_TEST_CHUNK_PLAN_HEAD && i < cap; ++i) out[i] = head[i];
    for (long i = 0; i < p.chunks && MCQ_TEST_CHUNK_PLAN_HEAD + 3 * i + 2 < cap; ++i) {
        long *const o = out + MCQ_TEST_CHUNK_PLAN_HEAD + 3 * i;
        o[0] = p.lane_of(i); o[1] = p.first_of(i); o[2] = p.rows_of(i, B);
    }
    return MCQ_TEST_CHUNK_PLAN_HEAD;
}

// include/mcq_probe.h: one refinement pass of B vectors as one chunk (test_pass, beside run_encode)
int mcq_test_pass(const float *x, long B, const void *prepared, int N, int K, int D, const int64_t *idx_in, int64_t *idx_out,
                  const int *nact, const int *map, unsigned flags, void *workspace, size_t workspace_bytes, void *stream) {
    g_last_launches = 0;
    if (!domain_ok(N, K, D)) return domain_err(N, K, D);
    if (N < 2) return MCQ_EUNSUPPORTED;
    if (B < 0 || (flags & ~MCQ_TEST_PASS_CAPPED)) return MCQ_EINVAL;
    if (B == 0) return 0;
    if (!x || !prepared || !idx_in || !idx_out || !workspace) return MCQ_EINVAL;
    if (reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return MCQ_EINVAL;
    const size_t per = workspace_per_vector(N, K, D), slack = workspace_slack(N, K, D);
    if (workspace_bytes < slack + per || (long)((workspace_bytes - slack) / per) < B) return MCQ_EWORKSPACE;     // the encode's chunk rule
    const EncodeCall c{prepared_view(prepared, N, K, D), 1.0f, N, K, D, 1, 0u, static_cast<hipStream_t>(stream), nullptr};
    const bool capped = (flags & MCQ_TEST_PASS_CAPPED) != 0;
    if (K > 256) return test_pass<uint16_t>(c, x, B, idx_in, idx_out, nact, map, capped, workspace);
    return test_pass<uint8_t>(c, x, B, idx_in, idx_out, nact, map, capped, workspace);
}

// include/mcq_probe.h: where the arrays of one record of k_tf_pass16_probe lie (the constants of mcq_pass16_kernels.h)
int mcq_test_pass16_layout(int N, size_t *out, int cap) {
    if (N != 8 && N != 16) return MCQ_EUNSUPPORTED;
    if (!out || cap < 0) return MCQ_EINVAL;
    constexpr int n = 2 * kP16RecArrays + 1;
    static_assert(n == MCQ_TEST_PASS16_LAYOUT_VALUES && kP16RecWritten == MCQ_TEST_PASS16_WRITTEN, "include/mcq_probe.h");
    size_t v[n];
    for (int i = 0; i < kP16RecArrays; ++i) {
        const size_t bytes = (size_t)p16_rec_bytes(N, i);
        v[2 * i] = bytes ? (size_t)kP16RecOff[i] : 0;
        v[2 * i + 1] = bytes;
    }
    v[n - 1] = kP16Rec;
    for (int i = 0; i < n && i < cap; ++i) out[i] = v[i];
    return n;
}

// include/mcq_probe.h: every pass of B vectors of 8 x 16 or 16 x 16 as one chunk from imported codes -- the chunk start, then
// launch_pass16 as the encode calls it, with the record dump and the grid cap the caller asks for
int mcq_test_pass16(const float *x, long B, const void *prepared, int N, int D, int iters, const int64_t *idx_in, int64_t *idx_out,
                    void *dump, size_t dump_bytes, int max_workgroups, void *workspace, size_t workspace_bytes, void *stream) {
    constexpr int K = 16;
    g_last_launches = 0;
    if (!domain_ok(N, K, D)) return domain_err(N, K, D);
    if (N != 8 && N != 16) return MCQ_EUNSUPPORTED;
    if (B < 0 || iters < 1 || iters > 60 || max_workgroups < 0) return MCQ_EINVAL;
    if (B == 0) return 0;
    if (!x || !prepared || !idx_in || !idx_out || !workspace) return MCQ_EINVAL;
    if (reinterpret_cast<uintptr_t>(workspace) % 256 != 0 || reinterpret_cast<uintptr_t>(dump) % 4 != 0) return MCQ_EINVAL;
    const size_t per = workspace_per_vector(N, K, D), slack = workspace_slack(N, K, D);
    if (workspace_bytes < slack + per || (long)((workspace_bytes - slack) / per) < B) return MCQ_EWORKSPACE;     // the encode's chunk rule
    if (dump && dump_bytes / kP16Rec / (size_t)iters < (size_t)B) return MCQ_EWORKSPACE;
    const EncodeCall c{prepared_view(prepared, N, K, D), 1.0f, N, K, D, iters, 0u, static_cast<hipStream_t>(stream), nullptr};
    const WorkspaceT<uint8_t> w = carve<uint8_t>(workspace, B, N, K, D);
    if (const int rc = launch_chunk_start<uint8_t>(c, w, x, B, idx_in, nullptr)) return rc;
    return launch_pass16(c, w, B, ChunkOut{nullptr, idx_out, nullptr, 1}, static_cast<uint8_t *>(dump), max_workgroups);
}

// ------------------------------------------------------------------ trainer pieces
int mcq_logits_argmax(const float *x, long B, const void *prepared, float lscale_exp, int N, int K, int D,
                      float *logits_out, int64_t *argmax_out, void *workspace, size_t workspace_bytes, void *stream,
                      unsigned flags) {
    if (!domain_ok(N, K, D) || K > 256) return MCQ_EUNSUPPORTED;      // (the trainer's entry point: one-byte entries)
    if (B < 0) return MCQ_EINVAL;
    if (B == 0) return 0;
    if (!x || !prepared || !logits_out || !argmax_out || !workspace) return MCQ_EINVAL;
    if (workspace_bytes < mcq_logits_workspace_bytes(B, N, D)) return MCQ_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const LogitsWs w = logits_ws(workspace, B, N, D);
    if (const int rc = run_logits(x, B, prepared, lscale_exp, N, K, D, logits_out, w.idx8, w, st, flags)) return rc;
    hipLaunchKernelGGL(k_export_indexes, dim3((unsigned)((B * N + 255) / 256)), dim3(256), 0, st, w.idx8, B * N, argmax_out);
    return counted_launch_rc();
}

// logits (stored) + arg max + refinement passes in one call: the frames become limb planes once, the indexes stay bytes
// until the end (what QuantizerTrainer.step runs: mcq_logits_argmax followed by mcq_refine_indexes, without the detours)
int mcq_logits_refine(const float *x, long B, const void *prepared, float lscale_exp, int N, int K, int D, int refine_iters,
                      float *logits_out, int64_t *idx_out, void *workspace, size_t workspace_bytes, void *stream,
                      unsigned flags) {
    return mcq_logits_refine_codes(x, B, prepared, lscale_exp, N, K, D, refine_iters, logits_out, idx_out, nullptr, workspace,
                                   workspace_bytes, stream, flags);
}

int mcq_logits_refine_codes(const float *x, long B, const void *prepared, float lscale_exp, int N, int K, int D, int refine_iters,
                            float *logits_out, int64_t *idx_out, uint8_t *codes_out, void *workspace, size_t workspace_bytes,
                            void *stream, unsigned flags) {
    if (K > 256) return MCQ_EUNSUPPORTED;       // a trainer entry point (stored logits for the fused loss kernels): K <= 256
    if (B > 0 && (!logits_out || !idx_out)) return MCQ_EINVAL;
    return run_encode(x, B, prepared, lscale_exp, N, K, D, refine_iters, nullptr, idx_out, workspace, workspace_bytes,
                      static_cast<hipStream_t>(stream), nullptr, nullptr, flags | MCQ_ENCODE_ALL_PASSES, logits_out,
                      codes_out);
}

namespace {
long loss_rows_per_chunk(long B) {   // at most ~1024 chunks, at least 64 rows each
    long r = (B + 1023) / 1024;
    r = r < 64 ? 64 : r;
    return (r + 15) / 16 * 16;
}
long loss_chunks(long B) { const long r = loss_rows_per_chunk(B); return (B + r - 1) / r; }

// the loss kernels' shapes; cap_n: one entropy pair per codebook in shared memory (s_hl / s_hi of loss_tail_body: 64)
bool loss_domain_ok(int N, int K, bool cap_n) { return is_pow2(K) && K >= 16 && K <= 256 && N >= 1 && (!cap_n || N <= 64); }

// workgroups of k_loss_bwd: kLossWaves waves, each on 64 / K rows of the [B * N][K] logits at a time (one row from K = 64 on)
long loss_bwd_blocks(long B, int N, int K) {
    const int rpw = K < 64 ? 64 / K : 1;
    return (B * N + (long)kLossWaves * rpw - 1) / ((long)kLossWaves * rpw);
}

// mcq_loss_bwd, and mcq_loss_bwd_ex (ex: bias and dot_part are required; the kernel's own defaults for them are null)
int launch_loss_bwd(const float *logits, const int64_t *idx, const float *lse, long B, int N, int K, const float *g_chosen,
                    const float *g_prob, float *grad_logits, const float *bias, float *dot_part, bool ex, void *stream) {
    if (!loss_domain_ok(N, K, false)) return MCQ_EUNSUPPORTED;
    if (B <= 0) return MCQ_EINVAL;
    if (!logits || !idx || !lse || !g_chosen || !g_prob || !grad_logits || (ex && (!bias || !dot_part))) return MCQ_EINVAL;
    const dim3 grid((unsigned)loss_bwd_blocks(B, N, K)), block(64 * kLossWaves);
    return pick<16, 32, 64, 128, 256>(K, [&](auto kk) {
        constexpr int KK = kk;
        hipLaunchKernelGGL((k_loss_bwd<KK>), grid, block, 0, static_cast<hipStream_t>(stream), logits, idx, lse, B, N, g_chosen, g_prob,
                           grad_logits, bias, dot_part);
        return counted_launch_rc();
    });
}
}  // namespace

size_t mcq_loss_workspace_bytes(long B, int N, int K) {
    if (B <= 0) return 256;
    return (size_t)loss_chunks(B) * N * (2 * (size_t)K + 1) * sizeof(float) + 256;
}

int mcq_loss_fwd(const float *logits, const int64_t *idx, long B, int N, int K, float *lse, float *chosen_sum,
                 float *prob_sum, float *count, void *workspace, size_t workspace_bytes, void *stream) {
    if (!loss_domain_ok(N, K, false)) return MCQ_EUNSUPPORTED;
    if (B <= 0) return MCQ_EINVAL;
    if (!logits || !idx || !lse || !chosen_sum || !prob_sum || !count || !workspace) return MCQ_EINVAL;
    if (workspace_bytes < mcq_loss_workspace_bytes(B, N, K)) return MCQ_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long rpc = loss_rows_per_chunk(B), chunks = loss_chunks(B);
    float *pp = static_cast<float *>(workspace);
    float *pc = pp + chunks * N * K;
    float *ph = pc + chunks * N * K;
    const dim3 grid((unsigned)(chunks * N)), block(64 * kLossWaves);
    const int rc = pick<16, 32, 64, 128, 256>(K, [&](auto kk) {
        constexpr int KK = kk;
        hipLaunchKernelGGL((k_loss_fwd<KK>), grid, block, 0, st, logits, idx, B, N, rpc, lse, pp, pc, ph);
        return counted_launch_rc();
    });
    if (rc) return rc;
    hipLaunchKernelGGL(k_loss_reduce, dim3((unsigned)N), dim3(256), 0, st, pp, pc, ph, chunks, N, K, prob_sum, count,
                       chosen_sum);
    return counted_launch_rc();
}

int mcq_loss_bwd(const float *logits, const int64_t *idx, const float *lse, long B, int N, int K, const float *g_chosen,
                 const float *g_prob, float *grad_logits, void *stream) {
    return launch_loss_bwd(logits, idx, lse, B, N, K, g_chosen, g_prob, grad_logits, nullptr, nullptr, false, stream);
}

int mcq_loss_tail(const float *sums, const float *prob_sum, const float *count, int N, int K, float entropy_scale,
                  float *losses, float *g, float *g_prob, void *stream) {
    if (!loss_domain_ok(N, K, true)) return MCQ_EUNSUPPORTED;
    if (!sums || !prob_sum || !count || !losses || !g || !g_prob) return MCQ_EINVAL;
    hipLaunchKernelGGL(k_loss_tail, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), sums, prob_sum, count, N, K,
                       entropy_scale, losses, g, g_prob);
    return counted_launch_rc();
}

int mcq_recon_fwd(const float *x, const int64_t *idx, long B, const void *prepared, const float *mean, int N, int K,
                  int D, float *err, float *num_part, float *den_part, void *stream) {
    if (!domain_ok(N, K, D) || K > 256) return MCQ_EUNSUPPORTED;
    if (B <= 0) return MCQ_EINVAL;
    if (!x || !idx || !prepared || !mean || !err || !num_part || !den_part) return MCQ_EINVAL;
    const Prepared P = prepared_view(prepared, N, K, D);
    hipLaunchKernelGGL(k_recon_fwd, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), x, idx, B,
                       P.C, mean, N, K, D, round_up16(D), err, num_part, den_part);
    return counted_launch_rc();
}


// ------------------------------------------------------------ parameter update
namespace {
// the bf16-piece kernel (k_wgrad_bf3: one workgroup of eight waves per CU, 128 x 128 outputs) takes the large tile-aligned
// products -- the trainer's second phase -- with about one workgroup per CU and at least 512 rows of the batch per split
// (dim 512, 2,048 logits, 4,096 frames: 4 splits 70.8 us per call, 8 splits 78.4, 16 splits 90.9; the fp32 kernel 113.9)
bool wgrad_use_bf3(long B, int M, int D) {
    static const bool f32_only = getenv("MCQ_WGRAD_F32") && atoi(getenv("MCQ_WGRAD_F32")) != 0;      // tuning hook: same sums to fp32 accuracy either way
    return !f32_only && (M % kWbM) == 0 && (D % kWbN) == 0 && M >= 1024 && B >= 2048;
}
int wgrad_splits_bf3(long B, int M, int D) {
    const long tiles = (long)(M / kWbM) * (D / kWbN);
    long s = (256 + tiles / 2) / tiles;
    const long max_s = B / 512;
    s = s > max_s ? max_s : s;
    return (int)(s < 1 ? 1 : s);
}

int wgrad_splits(long B, int M, int D) {
    const long tiles = (long)((M + kWgM - 1) / kWgM) * ((D + kWgN - 1) / kWgN);
    long s = 2048 / tiles;                 // ~8 workgroups per CU
    const long max_s = (B + 127) / 128;    // at least 128 rows of the batch per split
    s = s > max_s ? max_s : s;
    return (int)(s < 1 ? 1 : (s > 64 ? 64 : s));
}
}  // namespace

size_t mcq_weight_grad_workspace_bytes(long B, int M, int D) {
    if (B <= 0 || M <= 0 || D <= 0) return 256;
    return (size_t)wgrad_splits(B, M, D) * ((size_t)M * D + M) * sizeof(float) + 256;
}

int mcq_weight_grad(const float *G, const float *x, long B, int M, int D, const float *scale_dev, float *gW, float *gb,
                    void *workspace, size_t workspace_bytes, void *stream) {
    if (B <= 0 || M <= 0 || D <= 0 || (M & 15) != 0) return MCQ_EINVAL;
    if (!G || !x || !scale_dev || !gW || !gb || !workspace) return MCQ_EINVAL;
    if (workspace_bytes < mcq_weight_grad_workspace_bytes(B, M, D)) return MCQ_EWORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool bf3 = wgrad_use_bf3(B, M, D);
    const int splits = bf3 ? wgrad_splits_bf3(B, M, D) : wgrad_splits(B, M, D);      // (never more than the workspace was sized for)
    long rps = (B + splits - 1) / splits;
    rps = (rps + 31) / 32 * 32;
    float *part = static_cast<float *>(workspace);
    float *partb = part + (size_t)splits * M * D;
    if (bf3) {
        hipLaunchKernelGGL(k_wgrad_bf3, dim3((unsigned)((M / kWbM) * (D / kWbN) * splits)), dim3(512), 0, st, G, x, B, M, D, rps, part, partb);
    } else {
        const unsigned grid = (unsigned)(((M + kWgM - 1) / kWgM) * ((D + kWgN - 1) / kWgN) * splits);
        hipLaunchKernelGGL((k_wgrad_tn<16>), dim3(grid), dim3(256), 0, st, G, x, B, M, D, rps, part, partb);   // (32-row stages: 129 vs 115 us)
    }
    MCQ_LAUNCH_CHECK();
    const long MN = (long)M * D;
    hipLaunchKernelGGL(k_wgrad_reduce, dim3((unsigned)((MN / 4 + 255) / 256)), dim3(256), 0, st, part, partb, splits, MN, M,
                       scale_dev, gW, gb);
    return counted_launch_rc();
}

int mcq_adam_step(float *p, const float *g, float *m, float *v, long n, double lr, double beta1, double beta2, double eps,
                  double weight_decay, double bias_correction1, double bias_correction2_sqrt, void *stream) {
    if (n < 0 || (n > 0 && (!p || !g || !m || !v))) return MCQ_EINVAL;
    if (n == 0) return 0;
    long blocks = (n / 4 + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(k_adam, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), p, g, m, v, n,
                       (float)(lr / bias_correction1), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps,
                       (float)weight_decay, (float)bias_correction2_sqrt);
    return counted_launch_rc();
}

int mcq_loss_head_tail(const float *num_part, const float *den_part, long nparts, const float *chosen_n, int N, float batch,
                       float *head, const float *prob_sum, const float *count, int K, float entropy_scale, float *losses,
                       float *g, float *g_prob, void *stream) {
    if (!loss_domain_ok(N, K, true)) return MCQ_EUNSUPPORTED;     // (as mcq_loss_tail)
    if (nparts <= 0 || !num_part || !den_part || !chosen_n || !head || !prob_sum || !count || !losses || !g || !g_prob) return MCQ_EINVAL;
    hipLaunchKernelGGL(k_loss_head_tail, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), num_part, den_part, nparts,
                       chosen_n, N, batch, head, prob_sum, count, K, entropy_scale, losses, g, g_prob);
    return counted_launch_rc();
}
int mcq_loss_head(const float *num_part, const float *den_part, long nparts, const float *chosen_n, int N, float batch,
                  float *head, void *stream) {
    if (nparts <= 0 || N <= 0 || !num_part || !den_part || !chosen_n || !head) return MCQ_EINVAL;
    hipLaunchKernelGGL(k_loss_head, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), num_part, den_part, nparts, chosen_n,
                       N, batch, head);
    return counted_launch_rc();
}

int mcq_scales_exp(const float *centers_scale, const float *logits_scale, float speed, float *out2, void *stream) {
    if (!centers_scale || !logits_scale || !out2) return MCQ_EINVAL;
    hipLaunchKernelGGL(k_scales, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), centers_scale, logits_scale, speed, out2);
    return counted_launch_rc();
}

// decode_backward_u8 with the trainer's epilogue: rows scaled by sa[0]*sb[0]*sc (device floats), and per-wave partials
// of <unscaled sums, dotw> in dot_part[mcq_decode_backward_waves(N, K, D)]
long mcq_decode_backward_waves(int N, int K, int D) { return (long)N * K * db_chunks(D, db_cw_of(D, K)); }

int mcq_decode_backward_u8_ex(const float *grad_out, const uint8_t *codes, long B, int N, int K, int D, float *gC,
                              const float *sa, const float *sb, float sc, const float *dotw, float *dot_part, void *stream) {
    if (K > 256) return MCQ_EUNSUPPORTED;
    if (N <= 0 || K <= 0 || D <= 0 || B < 0 || !gC) return MCQ_EINVAL;
    if (B > 0 && (!grad_out || !codes)) return MCQ_EINVAL;
    if ((dotw == nullptr) != (dot_part == nullptr)) return MCQ_EINVAL;
    // the caller sized dot_part by mcq_decode_backward_waves: the wide kernel must be the one that runs when D % 4 == 0
    if ((D & 3) == 0 && db_cw(grad_out, gC, D, K, D, 0, dotw) != db_cw_of(D, K)) return MCQ_EINVAL;     // misaligned buffers
    const int rc = launch_decode_backward<uint8_t>(grad_out, codes, B, N, K, D, gC, (long)D, 0L, N, static_cast<hipStream_t>(stream),
                                                   sa, sb, sc, dotw, dot_part);
    if (rc) return rc;
    ++g_last_launches;
    return 0;
}

long mcq_loss_bwd_waves(long B, int N, int K) { return loss_bwd_blocks(B, N, K) * kLossWaves; }

int mcq_loss_bwd_ex(const float *logits, const int64_t *idx, const float *lse, long B, int N, int K, const float *g_chosen,
                    const float *g_prob, float *grad_logits, const float *bias, float *dot_part, void *stream) {
    return launch_loss_bwd(logits, idx, lse, B, N, K, g_chosen, g_prob, grad_logits, bias, dot_part, true, stream);
}

int mcq_grad_tail(const float *part_c, long n_c, const float *sa, const float *sb, float sc, const float *part_l, long n_l,
                  float speed, float *out_c, float *out_l, void *stream) {
    if (n_c < 0 || n_l < 0 || (n_c > 0 && !part_c) || (n_l > 0 && !part_l)) return MCQ_EINVAL;
    hipLaunchKernelGGL(k_grad_tail, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), part_c, n_c, sa, sb, sc, part_l, n_l,
                       speed, out_c, out_l);
    return counted_launch_rc();
}

// ---- search over stored codes: mcq_search_kernels.h (the launch arithmetic is above, ahead of the C linkage block)
static int search_tables(int domain_rc, const void *q, int q_is_fp16, long Q, const void *prepared, int N, int K, int D,
                         float *tables_out, void *stream) {
    if (domain_rc) return domain_rc;
    if (Q < 0 || Q > 0x7fffffffL) return MCQ_EINVAL;
    if (Q == 0) return 0;
    if (!q || !prepared || !tables_out) return MCQ_EINVAL;
    const Prepared P = prepared_view(prepared, N, K, D);
    const int NK = N * K;
    hipLaunchKernelGGL(k_search_tables, dim3((unsigned)((Q + kTabQueries - 1) / kTabQueries), (unsigned)((NK + kTabRows - 1) / kTabRows)),
                       dim3(256), 0, static_cast<hipStream_t>(stream), q, q_is_fp16 ? 1 : 0, (int)Q, P.C, NK, D, round_up16(D),
                       tables_out);
    return launch_rc();
}

int mcq_search_tables(const void *q, int q_is_fp16, long Q, const void *prepared, int N, int K, int D, float *tables_out,
                      void *stream) {
    return search_tables(search_domain(N, K, D), q, q_is_fp16, Q, prepared, N, K, D, tables_out, stream);
}

int mcq_code_norms(const uint8_t *codes, long B, const void *prepared, int N, int K, int D, float *norms_out, void *stream) {
    return code_norms<false>(codes, B, prepared, N, K, D, norms_out, stream);
}

size_t mcq_search_workspace_bytes(long Q, long B, int N, int K, int k) {
    return sized(Q, B, 0x7fffffffL, N, K, k, 64) ? scan_plan(Q, B, N, K, k).ws_bytes : 256;
}

int mcq_code_rnorms(const uint8_t *codes, long B, const void *prepared, int N, int K, int D, float *rnorms_out, void *stream) {
    return code_norms<true>(codes, B, prepared, N, K, D, rnorms_out, stream);
}

int mcq_rnorms_from_norms(const float *norms, long B, float *rnorms_out, void *stream) {
    if (B < 0) return MCQ_EINVAL;
    if (B > 0x7fffffffL) return MCQ_EUNSUPPORTED;
    if (B == 0) return 0;
    if (!norms || !rnorms_out) return MCQ_EINVAL;
    hipLaunchKernelGGL(k_rnorms_from_norms, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       norms, B, rnorms_out);
    return launch_rc();
}

int mcq_search_scan(const float *tables, long Q, const uint8_t *codes, const float *norms, long B, int N, int K, int k,
                    float *out_score, int64_t *out_index, void *workspace, size_t workspace_bytes, void *stream) {
    return mcq_search_scan_metric(tables, Q, codes, norms, B, N, K, k, MCQ_SEARCH_L2, out_score, out_index, workspace,
                                  workspace_bytes, stream);
}

int mcq_search_scan_metric(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K, int k,
                           int metric, float *out_score, int64_t *out_index, void *workspace, size_t workspace_bytes,
                           void *stream) {
    return mcq_search_scan_masked(tables, Q, codes, w, B, N, K, k, metric, nullptr, out_score, out_index, workspace,
                                  workspace_bytes, stream);
}

// rules 10-12: the scan over the stored vectors whose bit is set (mask == NULL: over all of them)
int mcq_search_scan_masked(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K, int k,
                           int metric, const uint64_t *mask, float *out_score, int64_t *out_index, void *workspace,
                           size_t workspace_bytes, void *stream) {
    return search_topk(tables, Q, codes, w, B, N, K, k, metric, mask, nullptr, out_score, out_index, workspace, workspace_bytes,
                       stream);
}

// rules 13-16: the search list by list.  The size depends on neither B nor L: the parts of a query are cut on the device.
size_t mcq_search_lists_workspace_bytes(long Q, int P, int N, int K, int k) {
    return sized(Q, P, kListMaxProbes, N, K, k, 64) ? lists_plan(Q, P, N, K, k).ws_bytes : 256;
}

int mcq_search_scan_lists(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K, int k,
                          int metric, const uint64_t *mask, const int64_t *list_offsets, long L, const int32_t *probes, int P,
                          float *out_score, int64_t *out_index, void *workspace, size_t workspace_bytes, void *stream) {
    const ListsIn li{list_offsets, L, probes, P};
    return search_topk(tables, Q, codes, w, B, N, K, k, metric, mask, &li, out_score, out_index, workspace, workspace_bytes, stream);
}

// ---- range search over stored codes: mcq_range_kernels.h (rules 7-9 of include/mcq.h)
size_t mcq_search_range_workspace_bytes(long Q, long B, int N, int K) {
    return sized(Q, B, 0x7fffffffL, N, K, 1, 1) ? range_plan(Q, B, N, K).ws_bytes : 256;
}

int mcq_search_range_count(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K, int metric,
                           const float *thr, int64_t *lims, void *workspace, size_t workspace_bytes, void *stream) {
    return mcq_search_range_count_masked(tables, Q, codes, w, B, N, K, metric, nullptr, thr, lims, workspace, workspace_bytes,
                                         stream);
}

int mcq_search_range_count_masked(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K,
                                  int metric, const uint64_t *mask, const float *thr, int64_t *lims, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    return range_count(tables, Q, codes, w, B, N, K, metric, mask, nullptr, thr, lims, workspace, workspace_bytes, stream);
}

int mcq_search_range_fill(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K, int metric,
                          const float *thr, const int64_t *lims, float *out_score, int64_t *out_index, long capacity,
                          void *workspace, size_t workspace_bytes, void *stream) {
    return mcq_search_range_fill_masked(tables, Q, codes, w, B, N, K, metric, nullptr, thr, lims, out_score, out_index, capacity,
                                        workspace, workspace_bytes, stream);
}

int mcq_search_range_fill_masked(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K,
                                 int metric, const uint64_t *mask, const float *thr, const int64_t *lims, float *out_score,
                                 int64_t *out_index, long capacity, void *workspace, size_t workspace_bytes, void *stream) {
    return range_fill(tables, Q, codes, w, B, N, K, metric, mask, nullptr, thr, lims, out_score, out_index, capacity, workspace,
                      workspace_bytes, stream);
}

// ---- rules 17-20: the range search list by list.  The size depends on neither B nor L: the parts of a query are cut on the device.
size_t mcq_search_range_lists_workspace_bytes(long Q, int P, int N, int K) {
    return sized(Q, P, kListMaxProbes, N, K, 1, 1) ? range_lists_plan(Q, P, N, K).ws_bytes : 256;
}

int mcq_search_range_lists_count(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K,
                                 int metric, const uint64_t *mask, const int64_t *list_offsets, long L, const int32_t *probes,
                                 int P, const float *thr, int64_t *lims, void *workspace, size_t workspace_bytes, void *stream) {
    const ListsIn li{list_offsets, L, probes, P};
    return range_count(tables, Q, codes, w, B, N, K, metric, mask, &li, thr, lims, workspace, workspace_bytes, stream);
}

int mcq_search_range_lists_fill(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K,
                                int metric, const uint64_t *mask, const int64_t *list_offsets, long L, const int32_t *probes,
                                int P, const float *thr, const int64_t *lims, float *out_score, int64_t *out_index, long capacity,
                                void *workspace, size_t workspace_bytes, void *stream) {
    const ListsIn li{list_offsets, L, probes, P};
    return range_fill(tables, Q, codes, w, B, N, K, metric, mask, &li, thr, lims, out_score, out_index, capacity, workspace,
                      workspace_bytes, stream);
}

// ---- rules 21-23: residual codes list by list.  probe_bias == NULL is the entry without one: the same launches
int mcq_search_scan_lists_bias(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K, int k,
                               int metric, const uint64_t *mask, const int64_t *list_offsets, long L, const int32_t *probes, int P,
                               const float *probe_bias, float *out_score, int64_t *out_index, void *workspace,
                               size_t workspace_bytes, void *stream) {
    const ListsIn li{list_offsets, L, probes, P, probe_bias};
    return search_topk(tables, Q, codes, w, B, N, K, k, metric, mask, &li, out_score, out_index, workspace, workspace_bytes, stream);
}

int mcq_search_range_lists_bias_count(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K,
                                      int metric, const uint64_t *mask, const int64_t *list_offsets, long L,
                                      const int32_t *probes, int P, const float *probe_bias, const float *thr, int64_t *lims,
                                      void *workspace, size_t workspace_bytes, void *stream) {
    const ListsIn li{list_offsets, L, probes, P, probe_bias};
    return range_count(tables, Q, codes, w, B, N, K, metric, mask, &li, thr, lims, workspace, workspace_bytes, stream);
}

int mcq_search_range_lists_bias_fill(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K,
                                     int metric, const uint64_t *mask, const int64_t *list_offsets, long L, const int32_t *probes,
                                     int P, const float *probe_bias, const float *thr, const int64_t *lims, float *out_score,
                                     int64_t *out_index, long capacity, void *workspace, size_t workspace_bytes, void *stream) {
    const ListsIn li{list_offsets, L, probes, P, probe_bias};
    return range_fill(tables, Q, codes, w, B, N, K, metric, mask, &li, thr, lims, out_score, out_index, capacity, workspace,
                      workspace_bytes, stream);
}

int mcq_code_norms_based(const uint8_t *codes, long B, const void *prepared, int N, int K, int D, const float *base, long L,
                         const int32_t *assign, float *norms_out, void *stream) {
    return code_norms<false, true>(codes, B, prepared, N, K, D, norms_out, stream, base, L, assign);
}

int mcq_code_rnorms_based(const uint8_t *codes, long B, const void *prepared, int N, int K, int D, const float *base, long L,
                          const int32_t *assign, float *rnorms_out, void *stream) {
    return code_norms<true, true>(codes, B, prepared, N, K, D, rnorms_out, stream, base, L, assign);
}

// ---- rules 24-27 (include/mcq_wide.h): the search past 64 neighbours, 1 <= k <= 1,024
size_t mcq_search_wide_workspace_bytes(long Q, long B, int N, int K, int k) {
    return sized(Q, B, 0x7fffffffL, N, K, k, kWideMaxK) ? wide_plan(Q, 1, N, K, k).ws_bytes : 256;
}

int mcq_search_wide(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K, int k, int metric,
                    const uint64_t *mask, float *out_score, int64_t *out_index, void *workspace, size_t workspace_bytes,
                    void *stream) {
    return search_wide(tables, Q, codes, w, B, N, K, k, metric, mask, nullptr, out_score, out_index, workspace, workspace_bytes,
                       stream);
}

size_t mcq_search_wide_lists_workspace_bytes(long Q, int P, int N, int K, int k) {
    return sized(Q, P, kListMaxProbes, N, K, k, kWideMaxK) ? wide_plan(Q, P, N, K, k).ws_bytes : 256;
}

int mcq_search_wide_lists(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K, int k,
                          int metric, const uint64_t *mask, const int64_t *list_offsets, long L, const int32_t *probes, int P,
                          const float *probe_bias, float *out_score, int64_t *out_index, void *workspace,
                          size_t workspace_bytes, void *stream) {
    const ListsIn li{list_offsets, L, probes, P, probe_bias};
    return search_wide(tables, Q, codes, w, B, N, K, k, metric, mask, &li, out_score, out_index, workspace, workspace_bytes, stream);
}

// ---- rules 28-31 (include/mcq_rerank.h): the exact re-ranking of a shortlist
size_t mcq_rerank_workspace_bytes(long Q, long S, int D, int k) {
    if (Q <= 0 || S <= 0 || rerank_domain(Q, S, 0, 0, D, k, MCQ_SEARCH_L2) != 0) return 256;
    return rerank_plan(Q, S, D, k).ws_bytes;
}

int mcq_rerank(const void *queries, int queries_half, long Q, const void *vectors, int vectors_half, long B, int D,
               const int64_t *shortlist, long S, const int64_t *row_of, long Bs, int k, int metric, float *out_score,
               int64_t *out_index, void *workspace, size_t workspace_bytes, void *stream) {
    return rerank(queries, queries_half != 0, Q, vectors, vectors_half != 0, B, D, shortlist, S, row_of, Bs, k, metric, out_score,
                  out_index, workspace, workspace_bytes, stream);
}

// ---- rules 32-35 (include/mcq_code16.h): stores of two-byte codes.  probes == NULL: the whole store
int mcq_search_tables_u16(const void *q, int q_is_fp16, long Q, const void *prepared, int N, int K, int D, float *tables_out,
                          void *stream) {
    return search_tables(code16_domain(N, K, D), q, q_is_fp16, Q, prepared, N, K, D, tables_out, stream);
}

int mcq_code_norms_u16(const uint16_t *codes, long B, const void *prepared, int N, int K, int D, int rnorm, const float *base,
                       long L, const int32_t *assign, float *out, void *stream) {
    if (!base && !assign)
        return rnorm ? code_norms<true, false>(codes, B, prepared, N, K, D, out, stream)
                     : code_norms<false, false>(codes, B, prepared, N, K, D, out, stream);
    return rnorm ? code_norms<true, true>(codes, B, prepared, N, K, D, out, stream, base, L, assign)
                 : code_norms<false, true>(codes, B, prepared, N, K, D, out, stream, base, L, assign);
}

size_t mcq_search_topk_u16_workspace_bytes(long Q, int P, int N, int K, int k) {
    return sized(Q, P, kListMaxProbes, N, K, k, kWideMaxK, 2) ? wide_plan(Q, P, N, K, k).ws_bytes : 256;
}

int mcq_search_topk_u16(const float *tables, long Q, const uint16_t *codes, const float *w, long B, int N, int K, int k, int metric,
                        const uint64_t *mask, const int64_t *list_offsets, long L, const int32_t *probes, int P,
                        const float *probe_bias, float *out_score, int64_t *out_index, void *workspace, size_t workspace_bytes,
                        void *stream) {
    const ListsIn li{list_offsets, L, probes, P, probe_bias};
    return search_wide(tables, Q, codes, w, B, N, K, k, metric, mask, probes ? &li : nullptr, out_score, out_index, workspace,
                       workspace_bytes, stream);
}

size_t mcq_search_range_u16_workspace_bytes(long Q, int P, int N, int K) {
    return sized(Q, P, kListMaxProbes, N, K, 1, 1, 2) ? range_lists_plan(Q, P, N, K).ws_bytes : 256;
}

int mcq_search_range_u16_count(const float *tables, long Q, const uint16_t *codes, const float *w, long B, int N, int K, int metric,
                               const uint64_t *mask, const int64_t *list_offsets, long L, const int32_t *probes, int P,
                               const float *probe_bias, const float *thr, int64_t *lims, void *workspace, size_t workspace_bytes,
                               void *stream) {
    const ListsIn li{list_offsets, L, probes, P, probe_bias};
    return range_count(tables, Q, codes, w, B, N, K, metric, mask, probes ? &li : nullptr, thr, lims, workspace, workspace_bytes,
                       stream);
}

int mcq_search_range_u16_fill(const float *tables, long Q, const uint16_t *codes, const float *w, long B, int N, int K, int metric,
                              const uint64_t *mask, const int64_t *list_offsets, long L, const int32_t *probes, int P,
                              const float *probe_bias, const float *thr, const int64_t *lims, float *out_score, int64_t *out_index,
                              long capacity, void *workspace, size_t workspace_bytes, void *stream) {
    const ListsIn li{list_offsets, L, probes, P, probe_bias};
    return range_fill(tables, Q, codes, w, B, N, K, metric, mask, probes ? &li : nullptr, thr, lims, out_score, out_index, capacity,
                      workspace, workspace_bytes, stream);
}

// ---- rules 36-39 (include/mcq_shortlist.h): the search over a shortlist
size_t mcq_search_shortlist_workspace_bytes(long Q, long S, int N, int K, int k) {
    if (Q <= 0 || S <= 0 || short_domain(Q, S, 0, 0, N, K, k, MCQ_SEARCH_L2, 2) != 0) return 256;
    return short_plan(Q, S, N, K, k).ws_bytes;
}

int mcq_search_shortlist(const float *tables, long Q, const uint8_t *codes, const float *w, long B, int N, int K, int k,
                         int metric, const int64_t *shortlist, long S, const int64_t *row_of, long Bs, const float *bias,
                         float *out_score, int64_t *out_index, void *workspace, size_t workspace_bytes, void *stream) {
    return search_shortlist(tables, Q, codes, w, B, N, K, k, metric, shortlist, S, row_of, Bs, bias, out_score, out_index, workspace,
                            workspace_bytes, stream);
}

int mcq_search_shortlist_u16(const float *tables, long Q, const uint16_t *codes, const float *w, long B, int N, int K, int k,
                             int metric, const int64_t *shortlist, long S, const int64_t *row_of, long Bs, const float *bias,
                             float *out_score, int64_t *out_index, void *workspace, size_t workspace_bytes, void *stream) {
    return search_shortlist(tables, Q, codes, w, B, N, K, k, metric, shortlist, S, row_of, Bs, bias, out_score, out_index, workspace,
                            workspace_bytes, stream);
}

// rule 10: a byte per stored vector -> a bit per stored vector
int mcq_search_pack_mask(const uint8_t *flags, long B, uint64_t *mask_out, void *stream) {
    if (B < 0) return MCQ_EINVAL;
    if (B > 0x7fffffffL) return MCQ_EUNSUPPORTED;
    if (B == 0) return 0;
    if (!flags || !mask_out || reinterpret_cast<uintptr_t>(mask_out) % 8 != 0) return MCQ_EINVAL;
    const long words = (B + 63) / 64;
    hipLaunchKernelGGL(k_pack_mask, dim3((unsigned)((words + kPackWaves - 1) / kPackWaves)), dim3(64 * kPackWaves), 0,
                       static_cast<hipStream_t>(stream), flags, B, reinterpret_cast<u64 *>(mask_out));
    return launch_rc();
}

int mcq_last_encode_launches(void) { return g_last_launches; }
int mcq_last_encode_lanes(void) { return g_last_lanes; }

int mcq_test_select(const float *scores, int cases, int per_lane, int cnt, float *out_v, int *out_p, void *stream) {
    if (!scores || !out_v || !out_p || cases <= 0 || cnt < 1 || cnt > 64) return MCQ_EINVAL;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // per_lane < 0: the same number of keys per lane in the slot-major layout, key i of a lane at position 64 * i + lane; -1004:
    // four keys per lane, positions in any order (the general form followed by a rank by position)
    static constexpr Pair kShapes[] = {{1, kLaneMajor}, {4, kLaneMajor}, {16, kLaneMajor}, {4, kSlotMajor}, {16, kSlotMajor}, {4, kAnyOrder}};
    const int vpl = per_lane == -1004 ? 4 : (per_lane < 0 ? -per_lane : per_lane);
    const int layout = per_lane == -1004 ? kAnyOrder : (per_lane < 0 ? kSlotMajor : kLaneMajor);
    const int rc = pick_pair<kShapes>(vpl, layout, [&](auto v, auto l) {
        constexpr int VPL = v, LAYOUT = l;
        hipLaunchKernelGGL((k_test_select<VPL, LAYOUT>), dim3(cases), dim3(64), 0, st, scores, cnt, out_v, out_p);
        return launch_rc();
    });
    return rc == MCQ_EUNSUPPORTED ? MCQ_EINVAL : rc;
}

#ifdef MCQ_STAMPS
// debug build only (-DMCQ_STAMPS, tools/exp_stamps.py): the phase stamps of the sampled waves, [kernel][wave][slot] u64 -> host
int mcq_debug_stamps(unsigned long long *host_dst, long count, int clear) {
    const long total = (long)kStampKernels * kStampWaves * kStampSlots;
    if (count > total) count = total;
    if (hipDeviceSynchronize() != hipSuccess) return MCQ_EINVAL;
    if (host_dst && count > 0 &&
        hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(g_stamps), (size_t)count * 8, 0, hipMemcpyDeviceToHost) != hipSuccess) return MCQ_EINVAL;
    if (clear) {
        void *p = nullptr;
        if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_stamps)) != hipSuccess || hipMemset(p, 0, (size_t)total * 8) != hipSuccess) return MCQ_EINVAL;
    }
    return (int)kStampSlots;
}
#endif

const char *mcq_profile_category_name(int category) {
    return (category >= 0 && category < CAT_COUNT) ? kCatNames[category] : nullptr;
}

int mcq_profile_encode(const float *x, long B, const void *prepared, float lscale_exp, int N, int K, int D,
                       int refine_iters, void *workspace, size_t workspace_bytes, void *stream, float *ms_out,
                       int *launches_out, int cap) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool wide = K > 256;                // (entries of more than 256-entry codebooks leave as int64: no byte form)
    const size_t need = (size_t)B * N * (wide ? 8 : 1);
    uint8_t *dummy = nullptr;                 // the codes of the profiled encodes (this entry point is a measurement tool: it allocates)
    if (!ms_out || cap <= 0) return MCQ_EINVAL;
    const hipError_t me = hipMalloc(reinterpret_cast<void **>(&dummy), need ? need : 1);
    if (me != hipSuccess) return (int)me;
    for (int i = 0; i < cap; ++i) { ms_out[i] = 0.f; if (launches_out) launches_out[i] = 0; }
    int rc = 0;
    for (int only = 0; only < CAT_COUNT && rc == 0; ++only) {      // one encode per category: see Prof
        Prof prof;
        prof.stream = st;
        prof.only = only;
        rc = run_encode(x, B, prepared, lscale_exp, N, K, D, refine_iters, wide ? nullptr : dummy,
                        wide ? reinterpret_cast<int64_t *>(dummy) : nullptr, workspace, workspace_bytes, st, &prof, nullptr,
                        MCQ_ENCODE_ALL_PASSES);
        (void)hipStreamSynchronize(st);
        for (size_t i = 0; rc == 0 && i < prof.cat.size(); ++i) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, prof.ev[prof.first[i]], prof.ev[prof.last[i]]);
            if (prof.cat[i] < cap) { ms_out[prof.cat[i]] += ms; if (launches_out) launches_out[prof.cat[i]] += 1; }
        }
        for (hipEvent_t e : prof.ev) (void)hipEventDestroy(e);
    }
    (void)hipFree(dummy);
    return rc == 0 ? CAT_COUNT : rc;
}

}  // extern "C"
