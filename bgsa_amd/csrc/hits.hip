// hits.hip — hit selection on a device score tile: the K best subjects per query, or every subject within a cutoff,
// without the [queries][subjects] matrix ever leaving HBM (include/bgsa_hip.h "hit selection").
//
// A separate memory-bound pass behind the row kernels: it reads the tile once (top-K) or twice (threshold: count, then
// write) with 16-byte loads per lane.  The row kernels are not touched.
//
// One total order makes every result unique.  A candidate is (score, subject id); better = larger score (smaller with
// `smallest`), among equal scores the smaller subject id.  As one 64-bit key, larger = better:
//
//     key = (ord + 32769) << 46  |  (2^46 - 1 - subject id)        ord = smallest ? -score : score,  key 0 = empty slot
//
// Top-K.  A row is cut into segments; one WAVE owns one (row, segment) and keeps its 64 best keys sorted, one per lane.
// Its cutoff is the key of lane K-1.  Columns arrive in ascending order, so once the list is full a later column can
// only enter with a strictly better score: nearly every element costs one compare of its score with the cutoff score.
// The rare survivors go through a per-wave LDS queue (full keys) and are inserted one by one: a shift by one lane behind
// the insertion point.  A second kernel, one wave per row, merges the segment lists (and, with `accumulate`, the lists
// already in the output) with the same insertion and full-key compares, and writes scores and subject ids.
//
// Threshold.  Count per (row, segment) -> exclusive scan per row (plus the row's current count with `accumulate`) ->
// the same scan of the tile again, each wave writing its hits in column order from its segment's offset.
//
// Every word of the workspace is written before it is read: no memset, no allocation, no synchronisation in the calls.
#include "bgsa_common.h"

namespace bgsa {

namespace {

constexpr int kIdBits = 46;
constexpr unsigned long long kIdMask = (1ull << kIdBits) - 1;
constexpr int kOrdBias = 32769;            // ord in [-32768, 32768] -> [1, 65537]; 0 is the empty slot
constexpr int64_t kMinSegCols = 8192;      // shortest segment worth a wave of its own
constexpr int64_t kTargetWaves = 32768;    // four waves per wave slot of a 256-CU part
constexpr int kUnroll = 4;                 // 16-byte loads a lane has in flight

using u64 = unsigned long long;
typedef int int4v __attribute__((ext_vector_type(4)));

// Segments per row of a launch over `cols` columns: enough waves to fill the chip, no segment below kMinSegCols.
inline int64_t segments_for(int n_queries, int64_t cols)
{
    const int64_t by_len = cols > kMinSegCols ? (cols + kMinSegCols - 1) / kMinSegCols : 1;
    const int64_t by_waves = (kTargetWaves + n_queries - 1) / n_queries;
    return by_len < by_waves ? by_len : by_waves;
}

struct Segs {
    int n;          // segments per row
    int64_t len;    // columns per segment: whole wave-loads, so every segment starts on a 16-byte boundary of its row
};
inline Segs plan_segments(int n_queries, int64_t valid_count, int elem_bytes)
{
    const int64_t unit = kLanes * (16 / elem_bytes);
    const int64_t want = segments_for(n_queries, valid_count);
    int64_t len = (valid_count + want - 1) / want;
    len = (len + unit - 1) / unit * unit;
    if (len < unit) len = unit;
    const int64_t n = valid_count > 0 ? (valid_count + len - 1) / len : 1;
    return {static_cast<int>(n), len};
}

// ---- the tile, 16 bytes per lane ------------------------------------------------------------------------------------
template <int EB> struct Elem;
template <> struct Elem<2> { using type = int16_t; };
template <> struct Elem<1> { using type = int8_t; };

// element j of a 16-byte vector
template <int EB> __device__ __forceinline__ int elem_of(const int4v &v, int j)
{
    if (EB == 2) {
        const int w = v[j >> 1];
        return (j & 1) ? (w >> 16) : static_cast<int>(static_cast<short>(w));
    }
    return static_cast<int>(static_cast<signed char>(v[j >> 2] >> (8 * (j & 3))));
}

// The 16 / EB elements of `row` from column `col` on.  aligned: one 16-byte load (the whole vector lies inside the
// row's stride); otherwise element loads of the columns below `limit` only (a tile whose rows do not start on 16-byte
// boundaries, and the ragged end of a row).  Elements at or beyond `limit` read as 0 and are masked by the callers.
template <int EB> __device__ __forceinline__ int4v load_vec(const typename Elem<EB>::type *row, int64_t col, int64_t limit, bool aligned)
{
    if (aligned) return *reinterpret_cast<const int4v *>(row + col);
    int4v v = {0, 0, 0, 0};
    constexpr int n = 16 / EB;
#pragma unroll
    for (int j = 0; j < n; j++) {
        const unsigned e = (col + j < limit) ? static_cast<unsigned>(row[col + j]) & (EB == 2 ? 0xffffu : 0xffu) : 0u;
        v[j / (4 / EB)] |= static_cast<int>(e << (8 * EB * (j % (4 / EB))));
    }
    return v;
}

__device__ __forceinline__ u64 encode_key(int ord, u64 subject) { return (static_cast<u64>(ord + kOrdBias) << kIdBits) | (kIdMask - subject); }
__device__ __forceinline__ int key_ord(u64 key) { return static_cast<int>(key >> kIdBits) - kOrdBias; }   // empty: -32769, below every score

__device__ __forceinline__ u64 uniform_key(u64 v, int lane)
{
    const unsigned lo = __builtin_amdgcn_readlane(static_cast<unsigned>(v), lane);
    const unsigned hi = __builtin_amdgcn_readlane(static_cast<unsigned>(v >> 32), lane);
    return (static_cast<u64>(hi) << 32) | lo;
}
__device__ __forceinline__ u64 lane_above(u64 v)   // lane i gets lane i-1's value; lane 0 gets "better than anything"
{
    const unsigned lo = __shfl_up(static_cast<unsigned>(v), 1, kLanes);
    const unsigned hi = __shfl_up(static_cast<unsigned>(v >> 32), 1, kLanes);
    return (threadIdx.x & (kLanes - 1)) ? ((static_cast<u64>(hi) << 32) | lo) : ~0ull;
}

// Inserts the `count` keys of the wave's queue into its sorted list (lane i = i-th best); k_lane = K - 1.
__device__ __forceinline__ void drain_queue(u64 &list, const u64 *queue, int count, int k_lane)
{
    for (int q = 0; q < count; q++) {
        const u64 c = uniform_u64(queue[q]);
        if (c > uniform_key(list, k_lane)) {           // wave-uniform: it may have been overtaken meanwhile
            const u64 above = lane_above(list);
            list = list > c ? list : (above > c ? c : above);
        }
    }
}

// Lanes with pass[j] append key[j]; returns the new count.  The order in the queue does not matter.
__device__ __forceinline__ int push_queue(u64 *queue, int count, bool pass, u64 key)
{
    const u64 b = __ballot(pass);
    if (pass) queue[count + __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(b >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(b), 0u))] = key;
    return count + __popcll(b);
}

// ---- top-K: one wave per (row, segment) -----------------------------------------------------------------------------
// One vector of the scan: its elements against the cutoff score; survivors through the queue.  The whole vector is one
// batch: every column of an earlier batch is below every column of this one, which is what makes the strict compare exact.
template <int EB, bool Smallest, bool Masked>
__device__ __forceinline__ void offer_vec(const int4v &v, int64_t col, int64_t limit, int64_t subject_base, u64 &list, int &thr,
                                          u64 *queue, int k_lane)
{
    constexpr int n = 16 / EB;
    bool pass[n];
    bool any = false;
#pragma unroll
    for (int j = 0; j < n; j++) {
        const int s = elem_of<EB>(v, j);
        pass[j] = (Smallest ? s < thr : s > thr) && (!Masked || col + j < limit);
        any |= pass[j];
    }
    if (__ballot(any) == 0) return;                // nearly always
    int count = 0;
#pragma unroll
    for (int j = 0; j < n; j++) {
        const int s = elem_of<EB>(v, j);
        count = push_queue(queue, count, pass[j], encode_key(Smallest ? -s : s, static_cast<u64>(subject_base + col + j)));
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the queue is written and read by different lanes of this wave
    __builtin_amdgcn_wave_barrier();
    drain_queue(list, queue, count, k_lane);
    __builtin_amdgcn_wave_barrier();
    const int cut = key_ord(uniform_key(list, k_lane));
    thr = Smallest ? -cut : cut;
}

template <int EB, bool Smallest>
__global__ __launch_bounds__(256) void top_hits_scan_kernel(const typename Elem<EB>::type *tile, int n_queries, int64_t row_stride,
                                                            int64_t valid_count, int64_t subject_base, int k_best, int n_segs,
                                                            int64_t seg_len, bool aligned, u64 *seg_lists)
{
    __shared__ u64 s_queue[kWavesPerBlock][kLanes * (16 / EB)];
    const int lane = threadIdx.x & (kLanes - 1);
    const int wave = threadIdx.x >> 6;
    const int64_t task = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave;
    if (task >= static_cast<int64_t>(n_queries) * n_segs) return;   // wave-uniform
    const int row = static_cast<int>(task / n_segs), seg = static_cast<int>(task % n_segs);
    const auto *base = tile + static_cast<int64_t>(row) * row_stride;
    u64 *queue = s_queue[wave];
    constexpr int per_lane = 16 / EB;
    constexpr int64_t per_wave = static_cast<int64_t>(kLanes) * per_lane;
    const int k_lane = k_best - 1;

    const int64_t lo = seg * seg_len;
    int64_t hi = lo + seg_len;
    if (hi > valid_count) hi = valid_count;
    u64 list = 0;
    int thr = Smallest ? -key_ord(0) : key_ord(0);    // everything passes while the list is not full
    int64_t col = lo;
    if (aligned) {
        for (; col + kUnroll * per_wave <= hi; col += kUnroll * per_wave) {      // whole loads, all columns valid
            int4v v[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; u++) v[u] = load_vec<EB>(base, col + u * per_wave + lane * per_lane, hi, true);
#pragma unroll
            for (int u = 0; u < kUnroll; u++)
                offer_vec<EB, Smallest, false>(v[u], col + u * per_wave + lane * per_lane, hi, subject_base, list, thr, queue, k_lane);
        }
    }
    for (; col < hi; col += per_wave) {                                          // the ragged end (and unaligned tiles)
        const int64_t c = col + lane * per_lane;
        // an aligned vector that starts below `hi` lies inside the row's stride: hi <= valid_count <= row_stride, both
        // the stride and c are multiples of the vector
        const int4v v = (c < hi) ? load_vec<EB>(base, c, hi, aligned) : int4v{0, 0, 0, 0};
        offer_vec<EB, Smallest, true>(v, c, hi, subject_base, list, thr, queue, k_lane);
    }
    seg_lists[task * kLanes + lane] = lane < k_best ? list : 0ull;
}

// One wave per row: the segment lists (and with `accumulate` the output's own K entries) -> the output, best first.
template <bool Smallest>
__global__ __launch_bounds__(256) void top_hits_merge_kernel(const u64 *seg_lists, int n_queries, int n_segs, int k_best, int accumulate,
                                                             int32_t *hit_scores, int64_t *hit_subjects)
{
    __shared__ u64 s_queue[kWavesPerBlock][kLanes];
    const int lane = threadIdx.x & (kLanes - 1);
    const int wave = threadIdx.x >> 6;
    const int row = blockIdx.x * kWavesPerBlock + wave;
    if (row >= n_queries) return;
    u64 *queue = s_queue[wave];
    const int k_lane = k_best - 1;
    u64 list = 0;
    auto offer = [&](u64 key) {
        const bool pass = key > uniform_key(list, k_lane);
        if (__ballot(pass) == 0) return;
        const int count = push_queue(queue, 0, pass, key);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        drain_queue(list, queue, count, k_lane);
        __builtin_amdgcn_wave_barrier();
    };
    const int64_t out = static_cast<int64_t>(row) * k_best + lane;
    if (accumulate) {
        u64 key = 0;
        if (lane < k_best) {
            const int64_t subject = hit_subjects[out];
            int s = hit_scores[out];
            s = s < -32768 ? -32768 : (s > 32767 ? 32767 : s);
            if (subject >= 0 && static_cast<u64>(subject) <= kIdMask) key = encode_key(Smallest ? -s : s, static_cast<u64>(subject));
        }
        offer(key);
    }
    const u64 *lists = seg_lists + static_cast<int64_t>(row) * n_segs * kLanes;
    for (int seg = 0; seg < n_segs; seg++) offer(lane < k_best ? lists[static_cast<int64_t>(seg) * kLanes + lane] : 0ull);
    if (lane < k_best) {
        if (list == 0) {
            hit_scores[out] = Smallest ? INT32_MAX : INT32_MIN;
            hit_subjects[out] = -1;
        } else {
            const int ord = key_ord(list);
            hit_scores[out] = Smallest ? -ord : ord;
            hit_subjects[out] = static_cast<int64_t>(kIdMask - (list & kIdMask));
        }
    }
}

// ---- threshold hits -------------------------------------------------------------------------------------------------
template <int EB, bool Smallest> __device__ __forceinline__ bool within(int s, int cutoff) { return Smallest ? s <= cutoff : s >= cutoff; }

// Walks one (row, segment) in column order and hands every vector to `f(vector, first column, masked)`.
template <int EB, typename F>
__device__ __forceinline__ void walk_segment(const typename Elem<EB>::type *base, int64_t lo, int64_t hi, bool aligned, int lane, F &&f)
{
    constexpr int per_lane = 16 / EB;
    constexpr int64_t per_wave = static_cast<int64_t>(kLanes) * per_lane;
    int64_t col = lo;
    if (aligned) {
        for (; col + kUnroll * per_wave <= hi; col += kUnroll * per_wave) {
            int4v v[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; u++) v[u] = load_vec<EB>(base, col + u * per_wave + lane * per_lane, hi, true);
#pragma unroll
            for (int u = 0; u < kUnroll; u++)
                if (!f(v[u], col + u * per_wave + lane * per_lane, false)) return;
        }
    }
    for (; col < hi; col += per_wave) {
        const int64_t c = col + lane * per_lane;
        const int4v v = (c < hi) ? load_vec<EB>(base, c, hi, aligned) : int4v{0, 0, 0, 0};
        if (!f(v, c, true)) return;
    }
}

template <int EB, bool Smallest>
__global__ __launch_bounds__(256) void threshold_count_kernel(const typename Elem<EB>::type *tile, int n_queries, int64_t row_stride,
                                                              int64_t valid_count, int cutoff, int n_segs, int64_t seg_len, bool aligned,
                                                              int *seg_counts)
{
    const int lane = threadIdx.x & (kLanes - 1);
    const int64_t task = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
    if (task >= static_cast<int64_t>(n_queries) * n_segs) return;
    const int row = static_cast<int>(task / n_segs), seg = static_cast<int>(task % n_segs);
    const int64_t lo = seg * seg_len;
    const int64_t hi = lo + seg_len < valid_count ? lo + seg_len : valid_count;
    int count = 0;   // wave-uniform: the ballots are counted on the scalar side
    walk_segment<EB>(tile + static_cast<int64_t>(row) * row_stride, lo, hi, aligned, lane, [&](const int4v &v, int64_t c, bool masked) {
#pragma unroll
        for (int j = 0; j < 16 / EB; j++)
            count += __popcll(__ballot(within<EB, Smallest>(elem_of<EB>(v, j), cutoff) && (!masked || c + j < hi)));
        return true;
    });
    if (lane == 0) seg_counts[task] = count;
}

// One wave per row: the segment counts become the segments' first output slots; the row's count becomes the true total.
__global__ __launch_bounds__(256) void threshold_scan_kernel(int *seg_counts, int n_queries, int n_segs, int32_t *counts_before, int32_t *counts)
{
    const int lane = threadIdx.x & (kLanes - 1);
    const int row = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (row >= n_queries) return;
    int *c = seg_counts + static_cast<int64_t>(row) * n_segs;
    long long run = counts_before ? counts[row] : 0;   // with accumulate: the row's count before this call, kept for the writer
    if (run < 0) run = 0;
    const long long first = run;
    if (counts_before && lane == 0) counts_before[row] = static_cast<int32_t>(first);
    for (int s0 = 0; s0 < n_segs; s0 += kLanes) {
        const int mine = (s0 + lane < n_segs) ? c[s0 + lane] : 0;
        int incl = mine;
        for (int d = 1; d < kLanes; d <<= 1) {
            const int t = __shfl_up(incl, d, kLanes);
            if (lane >= d) incl += t;
        }
        // the offset inside this call's hits fits 31 bits (valid_count < 2^31); the row's earlier count is added by the writer
        if (s0 + lane < n_segs) c[s0 + lane] = static_cast<int>(run - first) + incl - mine;
        run += __builtin_amdgcn_readlane(incl, kLanes - 1);
    }
    if (lane == 0) counts[row] = run > INT32_MAX ? INT32_MAX : static_cast<int32_t>(run);
}

template <int EB, bool Smallest>
__global__ __launch_bounds__(256) void threshold_write_kernel(const typename Elem<EB>::type *tile, int n_queries, int64_t row_stride,
                                                              int64_t valid_count, int64_t subject_base, int cutoff, int n_segs,
                                                              int64_t seg_len, bool aligned, const int *seg_offsets, long long cap,
                                                              const int32_t *counts_before, int32_t *hit_scores, int64_t *hit_subjects)
{
    const int lane = threadIdx.x & (kLanes - 1);
    const int64_t task = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
    if (task >= static_cast<int64_t>(n_queries) * n_segs) return;
    const int row = static_cast<int>(task / n_segs), seg = static_cast<int>(task % n_segs);
    const int64_t lo = seg * seg_len;
    const int64_t hi = lo + seg_len < valid_count ? lo + seg_len : valid_count;
    // slot of this segment's first hit: the row's count before this call (saved by the scan kernel in
    // counts_before, null without accumulate) + the hits of the segments in front
    long long slot = static_cast<long long>(seg_offsets[task]) + (counts_before ? counts_before[row] : 0);
    if (slot >= cap) return;
    int32_t *out_scores = hit_scores + static_cast<int64_t>(row) * cap;
    int64_t *out_subjects = hit_subjects + static_cast<int64_t>(row) * cap;
    walk_segment<EB>(tile + static_cast<int64_t>(row) * row_stride, lo, hi, aligned, lane, [&](const int4v &v, int64_t c, bool masked) {
        constexpr int n = 16 / EB;
        bool pass[n];
        int before = 0, total = 0;   // hits in the lanes below this one; hits of the whole vector
#pragma unroll
        for (int j = 0; j < n; j++) {
            pass[j] = within<EB, Smallest>(elem_of<EB>(v, j), cutoff) && (!masked || c + j < hi);
            const u64 b = __ballot(pass[j]);
            before += __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(b >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(b), 0u));
            total += __popcll(b);
        }
        if (total == 0) return true;
        long long at = slot + before;
#pragma unroll
        for (int j = 0; j < n; j++) {
            if (pass[j]) {
                if (at < cap) {
                    out_scores[at] = elem_of<EB>(v, j);
                    out_subjects[at] = subject_base + c + j;
                }
                at++;
            }
        }
        slot += total;
        return slot < cap;     // wave-uniform: a full list ends the walk
    });
}

// ---- host side ------------------------------------------------------------------------------------------------------
size_t hits_workspace_bytes(int n_queries, int64_t row_stride)
{
    // lists: n_queries x segments x 64 keys.  segments <= ceil(target / n_queries) and <= ceil(stride / min length);
    // both bounds below grow with either argument, so the size never shrinks when one of them grows.
    const unsigned long long nq = static_cast<unsigned long long>(n_queries);
    const unsigned long long by_waves = static_cast<unsigned long long>(kTargetWaves) + nq;
    const unsigned long long by_len = nq * static_cast<unsigned long long>((row_stride + kMinSegCols - 1) / kMinSegCols);
    const unsigned long long lists = by_waves < by_len ? by_waves : by_len;
    return static_cast<size_t>(lists * kLanes * sizeof(u64) + 256);
}

bool tile_is_aligned(const void *tile, int64_t row_stride, int elem_bytes)
{
    return (reinterpret_cast<uintptr_t>(tile) & 15) == 0 && ((row_stride * elem_bytes) & 15) == 0;
}

struct TopArgs {
    const void *tile; int elem_bytes, n_queries; int64_t row_stride, valid_count, subject_base; int k_best, smallest, accumulate;
    int32_t *scores; int64_t *subjects; hipStream_t stream;
};

template <int EB, bool Smallest> int launch_top(const TopArgs &a, void *ws)
{
    const Segs sg = plan_segments(a.n_queries, a.valid_count, EB);
    const int64_t waves = static_cast<int64_t>(a.n_queries) * sg.n;
    u64 *lists = static_cast<u64 *>(ws);
    hipLaunchKernelGGL((top_hits_scan_kernel<EB, Smallest>), dim3(static_cast<unsigned>((waves + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(256), 0,
                       a.stream, static_cast<const typename Elem<EB>::type *>(a.tile), a.n_queries, a.row_stride, a.valid_count, a.subject_base,
                       a.k_best, sg.n, sg.len, tile_is_aligned(a.tile, a.row_stride, EB), lists);
    BGSA_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((top_hits_merge_kernel<Smallest>), dim3((a.n_queries + kWavesPerBlock - 1) / kWavesPerBlock), dim3(256), 0, a.stream, lists,
                       a.n_queries, sg.n, a.k_best, a.accumulate, a.scores, a.subjects);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

int run_top(void *ws, void *ctx)
{
    const TopArgs &a = *static_cast<const TopArgs *>(ctx);
    if (a.elem_bytes == 2) return a.smallest ? launch_top<2, true>(a, ws) : launch_top<2, false>(a, ws);
    return a.smallest ? launch_top<1, true>(a, ws) : launch_top<1, false>(a, ws);
}

struct ThresholdArgs {
    const void *tile; int elem_bytes, n_queries; int64_t row_stride, valid_count, subject_base; int cutoff, smallest, accumulate;
    int64_t cap; int32_t *counts, *scores; int64_t *subjects; hipStream_t stream;
};

template <int EB, bool Smallest> int launch_threshold(const ThresholdArgs &a, void *ws)
{
    const Segs sg = plan_segments(a.n_queries, a.valid_count, EB);
    const int64_t waves = static_cast<int64_t>(a.n_queries) * sg.n;
    const dim3 grid(static_cast<unsigned>((waves + kWavesPerBlock - 1) / kWavesPerBlock)), rows((a.n_queries + kWavesPerBlock - 1) / kWavesPerBlock);
    const auto *tile = static_cast<const typename Elem<EB>::type *>(a.tile);
    const bool aligned = tile_is_aligned(a.tile, a.row_stride, EB);
    // workspace: [n_queries][segments] counts -> offsets, then (accumulate) the rows' counts before this call
    int *seg_counts = static_cast<int *>(ws);
    int32_t *before = nullptr;
    hipLaunchKernelGGL((threshold_count_kernel<EB, Smallest>), grid, dim3(256), 0, a.stream, tile, a.n_queries, a.row_stride, a.valid_count, a.cutoff,
                       sg.n, sg.len, aligned, seg_counts);
    BGSA_HIP_TRY(hipGetLastError());
    if (a.accumulate) before = reinterpret_cast<int32_t *>(seg_counts + waves);
    hipLaunchKernelGGL(threshold_scan_kernel, rows, dim3(256), 0, a.stream, seg_counts, a.n_queries, sg.n, before, a.counts);
    BGSA_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((threshold_write_kernel<EB, Smallest>), grid, dim3(256), 0, a.stream, tile, a.n_queries, a.row_stride, a.valid_count,
                       a.subject_base, a.cutoff, sg.n, sg.len, aligned, seg_counts, static_cast<long long>(a.cap), before, a.scores, a.subjects);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

int run_threshold(void *ws, void *ctx)
{
    const ThresholdArgs &a = *static_cast<const ThresholdArgs *>(ctx);
    if (a.elem_bytes == 2) return a.smallest ? launch_threshold<2, true>(a, ws) : launch_threshold<2, false>(a, ws);
    return a.smallest ? launch_threshold<1, true>(a, ws) : launch_threshold<1, false>(a, ws);
}

// The checks both calls share; everything here comes before the first HIP call.
int check_tile_args(const char *who, const void *tile, int elem_bytes, int n_queries, int64_t row_stride, int64_t valid_count,
                    int64_t subject_base, const void *d_workspace, size_t workspace_bytes)
{
    const char *why = nullptr;
    if (!tile) why = "the tile is NULL";
    else if (elem_bytes != 1 && elem_bytes != 2) why = "elem_bytes must be 1 or 2";
    else if (n_queries <= 0 || row_stride <= 0) why = "n_queries and row_stride must be positive";
    else if (valid_count < 0 || valid_count > row_stride) why = "valid_count must lie in [0, row_stride]";
    else if (valid_count >= (int64_t(1) << 31)) why = "valid_count must be below 2^31";
    else if (subject_base < 0 || subject_base > static_cast<int64_t>(kIdMask) - valid_count) why = "subject ids must lie in [0, 2^46)";
    else if (d_workspace && workspace_bytes < hits_workspace_bytes(n_queries, row_stride)) why = "workspace smaller than bgsa_hip_hits_workspace_bytes()";
    if (!why) return BGSA_HIP_OK;
    char msg[160];
    snprintf(msg, sizeof msg, "%s: %s", who, why);
    set_error_text(msg);
    return BGSA_HIP_EINVAL;
}

}  // namespace

}  // namespace bgsa

using namespace bgsa;

extern "C" {

size_t bgsa_hip_hits_workspace_bytes(int n_queries, int64_t row_stride, int elem_bytes, int k_best)
{
    if (n_queries <= 0 || row_stride <= 0 || (elem_bytes != 1 && elem_bytes != 2) || k_best < 1) return 0;
    return hits_workspace_bytes(n_queries, row_stride);
}

int bgsa_hip_top_hits_dev(const void *d_results, int elem_bytes, int n_queries, int64_t row_stride, int64_t valid_count,
                          int64_t subject_base, int k_best, int smallest, int accumulate, int32_t *d_hit_scores,
                          int64_t *d_hit_subjects, void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (!d_hit_scores || !d_hit_subjects) {
        set_error_text("top_hits_dev: an output list is NULL");
        return BGSA_HIP_EINVAL;
    }
    if (int rc = check_tile_args("top_hits_dev", d_results, elem_bytes, n_queries, row_stride, valid_count, subject_base, d_workspace, workspace_bytes))
        return rc;
    if (k_best < 1 || k_best > HIP_V_NUM) {
        set_error_text("top_hits_dev: k_best must lie in 1..64 (one wavefront holds the sorted list, one entry per lane)");
        return BGSA_HIP_EUNSUPPORTED;
    }
    TopArgs a{d_results, elem_bytes, n_queries, row_stride, valid_count, subject_base, k_best, smallest != 0, accumulate != 0,
              d_hit_scores, d_hit_subjects, static_cast<hipStream_t>(stream)};
    if (d_workspace) return run_top(d_workspace, &a);
    return with_own_scratch(a.stream, hits_workspace_bytes(n_queries, row_stride), run_top, &a);
}

int bgsa_hip_threshold_hits_dev(const void *d_results, int elem_bytes, int n_queries, int64_t row_stride, int64_t valid_count,
                                int64_t subject_base, int cutoff, int smallest, int accumulate, int64_t cap_per_query,
                                int32_t *d_counts, int32_t *d_hit_scores, int64_t *d_hit_subjects, void *d_workspace,
                                size_t workspace_bytes, void *stream)
{
    if (!d_counts || !d_hit_scores || !d_hit_subjects || cap_per_query <= 0) {
        set_error_text("threshold_hits_dev: an output is NULL or cap_per_query is not positive");
        return BGSA_HIP_EINVAL;
    }
    if (int rc = check_tile_args("threshold_hits_dev", d_results, elem_bytes, n_queries, row_stride, valid_count, subject_base, d_workspace,
                                 workspace_bytes))
        return rc;
    ThresholdArgs a{d_results, elem_bytes, n_queries, row_stride, valid_count, subject_base, cutoff, smallest != 0, accumulate != 0,
                    cap_per_query, d_counts, d_hit_scores, d_hit_subjects, static_cast<hipStream_t>(stream)};
    if (d_workspace) return run_threshold(d_workspace, &a);
    return with_own_scratch(a.stream, hits_workspace_bytes(n_queries, row_stride), run_threshold, &a);
}

}  // extern "C"
