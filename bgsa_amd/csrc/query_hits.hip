// query_hits.hip — hit lists per SUBJECT: the K best queries of every column of a device score tile, or every query within a
// cutoff, without the [queries][subjects] matrix leaving HBM (include/bgsa_hip.h "hit lists per subject").
// The column counterpart of hits.hip, which reduces the same tile along its rows.
//
// One total order makes every result unique.  A candidate is (score, query id); better = larger score (smaller with `smallest`),
// among equal scores the smaller query id.  As one 64-bit key, larger = better:
//
//     key = (ord + 32769) << 32  |  (2^31 - 1 - query id)          ord = smallest ? -score : score,  key 0 = empty slot
//
// Layout.  The tile is row-major, so a LANE owns PL adjacent columns — one dword of a row: two int16 or four int8 scores — and a
// wave owns 64 * PL adjacent columns and walks down ALL rows of the call: every load of a wave is one contiguous 256-byte piece
// of a row, kRows of them in flight.  Rows are not split among waves, so nothing has to be merged and no workspace is used; the
// parallelism is the tile's width (a 1M-subject tile has 7,813 waves of int16 columns).
//
// Top-K.  Every column keeps its K best keys as a binary min-heap (root = the worst of the kept) in LDS, entry h of column slot j
// at [(h * PL + j) * 64 + lane]: whatever h a lane is at, the 64 lanes of one access fall on 64 different 8-byte slots of a
// 512-byte line — no bank conflict.  Only the owning lane touches a heap, so no barrier is needed.  The column's cutoff — the
// root's score — sits in a register.  Rows arrive in ascending id order, so a candidate enters only with a strictly better
// SCORE: nearly every element costs one compare.  (With `accumulate` a stored id may lie above the call's ids; such a column
// lets equal scores through to the full-key compare.)  The elements of kRows rows that pass are noted as one bit mask per column
// and inserted afterwards, lowest row first, each lane working through its own mask: the divergent loop runs as often as the
// busiest lane has survivors in kRows rows, not once per row with a survivor anywhere in the wave.  An insert replaces the root
// and sifts down, log2 K steps.  At the end every heap is sorted in place (heap sort) and written best first.
//
// Threshold.  One pass: every lane appends its columns' hits behind the column's count, which it keeps in a register.
//
// No allocation, no synchronisation, no workspace word read.
#include "bgsa_common.h"

namespace bgsa {

namespace {

using u64 = unsigned long long;

constexpr int kOrdBias = 32769;            // ord in [-32768, 32768] -> [1, 65537]; 0 is the empty slot
constexpr unsigned kIdTop = 0x7fffffffu;   // ids are non-negative int32
constexpr int kRows = 16;                  // rows (dword loads) a lane has in flight, and the width of the survivor mask
constexpr size_t kLdsLimit = 65536;        // dynamic LDS a launch may ask for without opting in to more
constexpr size_t kWorkspaceBytes = 256;    // nothing is kept there today; the ABI's size for a caller that allocates one

template <int EB> struct Elem;
template <> struct Elem<2> { using type = int16_t; };
template <> struct Elem<1> { using type = int8_t; };

// element j of a packed load
template <int EB> __device__ __forceinline__ int elem_of(unsigned w, int j)
{
    if (EB == 2) return static_cast<int>(static_cast<short>(w >> (16 * j)));
    return static_cast<int>(static_cast<signed char>(w >> (8 * j)));
}

// The PL elements of a row from `p` on, packed.  whole: one PL * EB-byte load (the tile is aligned for it and all PL columns
// are candidates); otherwise element loads of the first n_valid columns only — an unaligned tile and the ragged end.  A column
// at or beyond valid_count is never read.
template <int EB, int PL> __device__ __forceinline__ unsigned load_cols(const typename Elem<EB>::type *p, int n_valid, bool whole)
{
    if (whole) {
        if (EB * PL == 4) return *reinterpret_cast<const unsigned *>(p);
        return *reinterpret_cast<const unsigned short *>(p);
    }
    unsigned w = 0;
#pragma unroll
    for (int j = 0; j < PL; j++)
        if (j < n_valid) w |= (static_cast<unsigned>(p[j]) & (EB == 2 ? 0xffffu : 0xffu)) << (8 * EB * j);
    return w;
}

// kRows rows from `first` on (`left` rows remain).  wave_whole: every lane of the wave takes whole loads — then a full batch is
// kRows loads with nothing to decide between them (wave-uniform); otherwise each row and lane is decided on its own.
template <int EB, int PL>
__device__ __forceinline__ void load_rows(const typename Elem<EB>::type *first, int64_t row_stride, int left, int n_valid, bool whole, bool wave_whole,
                                          unsigned (&v)[kRows])
{
    if (wave_whole && left >= kRows) {
#pragma unroll
        for (int u = 0; u < kRows; u++) v[u] = load_cols<EB, PL>(first + u * row_stride, PL, true);
        return;
    }
#pragma unroll
    for (int u = 0; u < kRows; u++) v[u] = (u < left && n_valid > 0) ? load_cols<EB, PL>(first + u * row_stride, n_valid, whole) : 0u;
}

__device__ __forceinline__ u64 encode_key(int ord, int id) { return (static_cast<u64>(ord + kOrdBias) << 32) | (kIdTop - static_cast<unsigned>(id)); }
__device__ __forceinline__ int key_ord(u64 key) { return static_cast<int>(key >> 32) - kOrdBias; }   // empty: -32769, below every score
__device__ __forceinline__ int key_id(u64 key) { return static_cast<int>(kIdTop - static_cast<unsigned>(key)); }

// `key` takes the root's place in the min-heap of `size` entries (entry h at heap[h * stride]) and sinks to where it belongs.
__device__ __forceinline__ void sift_down(u64 *heap, int stride, int size, u64 key)
{
    int pos = 0;
    for (;;) {
        int child = 2 * pos + 1;
        if (child >= size) break;
        u64 least = heap[child * stride];
        if (child + 1 < size) {
            const u64 right = heap[(child + 1) * stride];
            if (right < least) {
                least = right;
                child++;
            }
        }
        if (least >= key) break;
        heap[pos * stride] = least;
        pos = child;
    }
    heap[pos * stride] = key;
}

// v[u] for a per-lane u in [0, 16): a select tree over VALUES (a ?: between two array elements is an lvalue, which turns the tree
// into an indexed load and the array into scratch memory)
__device__ __forceinline__ unsigned pick(bool second, unsigned x, unsigned y) { return second ? y : x; }
__device__ __forceinline__ unsigned pick_row(const unsigned (&v)[kRows], int u)
{
    static_assert(kRows == 16, "pick_row selects among 16 rows");
    unsigned a[8], b[4], c[2];
#pragma unroll
    for (int i = 0; i < 8; i++) a[i] = pick(u & 1, v[2 * i], v[2 * i + 1]);
#pragma unroll
    for (int i = 0; i < 4; i++) b[i] = pick(u & 2, a[2 * i], a[2 * i + 1]);
#pragma unroll
    for (int i = 0; i < 2; i++) c[i] = pick(u & 4, b[2 * i], b[2 * i + 1]);
    return pick(u & 8, c[0], c[1]);
}

// What a score has to beat to be looked at: the root's score, or one worse where equal scores go to the full-key compare.
template <bool Smallest> __device__ __forceinline__ int bar_of(u64 root, int loose)
{
    const int ord = key_ord(root) - loose;
    return Smallest ? -ord : ord;
}

// ---- top-K: one lane per PL columns, all rows --------------------------------------------------------------------------
template <int EB, int PL, bool Smallest>
__global__ __launch_bounds__(256) void top_queries_kernel(const typename Elem<EB>::type *tile, int n_queries, int64_t row_stride, int64_t valid_count,
                                                          int query_base, int k_best, int accumulate, bool aligned, int32_t *hit_scores,
                                                          int32_t *hit_queries)
{
    extern __shared__ __attribute__((aligned(16))) u64 s_heaps[];   // [waves of the block][k_best][PL][64 lanes]
    constexpr int stride = PL * kLanes;
    const int lane = threadIdx.x & (kLanes - 1);
    const int wave = threadIdx.x >> 6;
    const int64_t group = static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + wave;
    if (group * stride >= valid_count) return;                            // wave-uniform
    const int64_t c0 = group * stride + static_cast<int64_t>(lane) * PL;   // this lane's first column
    const int n_valid = valid_count - c0 >= PL ? PL : (valid_count > c0 ? static_cast<int>(valid_count - c0) : 0);
    const bool whole = aligned && n_valid == PL;
    const bool wave_whole = __ballot(!whole) == 0;
    u64 *heaps = s_heaps + static_cast<size_t>(wave) * k_best * stride + lane;    // column slot j: heaps + j * 64

    for (int h = 0; h < k_best * PL; h++) heaps[h * kLanes] = 0;
    int loose[PL], bar[PL];
#pragma unroll
    for (int j = 0; j < PL; j++) loose[j] = 0;
    if (accumulate) {
#pragma unroll
        for (int j = 0; j < PL; j++) {
            if (j >= n_valid) continue;
            u64 *heap = heaps + j * kLanes;
            const int64_t out = (c0 + j) * k_best;
            for (int slot = 0; slot < k_best; slot++) {
                const int id = hit_queries[out + slot];
                if (id < 0) continue;
                int s = hit_scores[out + slot];
                s = s < -32768 ? -32768 : (s > 32767 ? 32767 : s);
                const u64 key = encode_key(Smallest ? -s : s, id);
                if (key > heap[0]) sift_down(heap, stride, k_best, key);
                if (id >= query_base) loose[j] = 1;    // this call may bring an equal score with a smaller id
            }
        }
    }
#pragma unroll
    for (int j = 0; j < PL; j++) bar[j] = bar_of<Smallest>(heaps[j * kLanes], loose[j]);

    const auto *col = tile + c0;
    unsigned v[kRows], ahead[kRows];     // the batch at hand and the next one, loaded while this one is looked at
    load_rows<EB, PL>(col, row_stride, n_queries, n_valid, whole, wave_whole, ahead);
    for (int r0 = 0; r0 < n_queries; r0 += kRows) {
        const int left = n_queries - r0;
#pragma unroll
        for (int u = 0; u < kRows; u++) v[u] = ahead[u];
        if (left > kRows) load_rows<EB, PL>(col + static_cast<int64_t>(r0 + kRows) * row_stride, row_stride, left - kRows, n_valid, whole, wave_whole, ahead);
        const unsigned rows = left >= kRows ? 0xffffu : ((1u << left) - 1u);
#pragma unroll
        for (int j = 0; j < PL; j++) {
            unsigned mask = 0;
#pragma unroll
            for (int u = 0; u < kRows; u++) {
                const int s = elem_of<EB>(v[u], j);
                mask |= (Smallest ? s < bar[j] : s > bar[j]) ? (1u << u) : 0u;
            }
            mask &= (j < n_valid) ? rows : 0u;
            if (__ballot(mask != 0) == 0) continue;     // nearly always once the lists are full
            u64 *heap = heaps + j * kLanes;
            while (mask) {                              // per lane: its own survivors, lowest row first
                const int u = __builtin_ctz(mask);
                mask &= mask - 1;
                const int s = elem_of<EB>(pick_row(v, u), j);
                const u64 key = encode_key(Smallest ? -s : s, query_base + r0 + u);
                if (key > heap[0]) {                    // the root may have risen since the mask was formed
                    sift_down(heap, stride, k_best, key);
                    bar[j] = bar_of<Smallest>(heap[0], loose[j]);
                }
            }
        }
    }

#pragma unroll
    for (int j = 0; j < PL; j++) {
        if (j >= n_valid) continue;
        u64 *heap = heaps + j * kLanes;
        for (int size = k_best - 1; size > 0; size--) {     // heap sort: the worst of what is left goes behind it
            const u64 last = heap[size * stride];
            heap[size * stride] = heap[0];
            sift_down(heap, stride, size, last);
        }
        const int64_t out = (c0 + j) * k_best;
        for (int h = 0; h < k_best; h++) {
            const u64 key = heap[h * stride];
            if (key == 0) {
                hit_scores[out + h] = Smallest ? INT32_MAX : INT32_MIN;
                hit_queries[out + h] = -1;
            } else {
                const int ord = key_ord(key);
                hit_scores[out + h] = Smallest ? -ord : ord;
                hit_queries[out + h] = key_id(key);
            }
        }
    }
}

// ---- threshold lists: one pass, every lane appends behind its columns' counts -------------------------------------------
template <int EB, int PL, bool Smallest>
__global__ __launch_bounds__(256) void threshold_queries_kernel(const typename Elem<EB>::type *tile, int n_queries, int64_t row_stride,
                                                                int64_t valid_count, int query_base, int cutoff, int accumulate, int cap,
                                                                bool aligned, int32_t *counts, int32_t *hit_scores, int32_t *hit_queries)
{
    constexpr int stride = PL * kLanes;
    const int lane = threadIdx.x & (kLanes - 1);
    const int64_t group = static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (group * stride >= valid_count) return;
    const int64_t c0 = group * stride + static_cast<int64_t>(lane) * PL;
    const int n_valid = valid_count - c0 >= PL ? PL : (valid_count > c0 ? static_cast<int>(valid_count - c0) : 0);
    const bool whole = aligned && n_valid == PL;
    const bool wave_whole = __ballot(!whole) == 0;
    long long count[PL];
#pragma unroll
    for (int j = 0; j < PL; j++) {
        count[j] = 0;
        if (accumulate && j < n_valid) {
            const int before = counts[c0 + j];
            count[j] = before > 0 ? before : 0;
        }
    }
    const auto *col = tile + c0;
    for (int r0 = 0; r0 < n_queries; r0 += kRows) {
        unsigned v[kRows];
        load_rows<EB, PL>(col + static_cast<int64_t>(r0) * row_stride, row_stride, n_queries - r0, n_valid, whole, wave_whole, v);
#pragma unroll
        for (int j = 0; j < PL; j++) {
#pragma unroll
            for (int u = 0; u < kRows; u++) {
                const int s = elem_of<EB>(v[u], j);
                if ((Smallest ? s <= cutoff : s >= cutoff) && j < n_valid && r0 + u < n_queries) {
                    if (count[j] < cap) {
                        const int64_t at = (c0 + j) * cap + count[j];
                        hit_scores[at] = s;
                        hit_queries[at] = query_base + r0 + u;
                    }
                    count[j]++;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < PL; j++)
        if (j < n_valid) counts[c0 + j] = count[j] > INT32_MAX ? INT32_MAX : static_cast<int32_t>(count[j]);
}

// ---- host side ------------------------------------------------------------------------------------------------------------
struct Args {
    const void *tile; int elem_bytes, n_queries; int64_t row_stride, valid_count; int query_base, k_or_cutoff, smallest, accumulate, cap;
    int32_t *counts, *scores, *queries; hipStream_t stream;
};

// A wave's heaps take k_best * PL * 512 bytes of LDS; the block holds as many waves (at most four) as fit the LDS a launch gets.
inline int waves_per_block(int k_best, int pl)
{
    const size_t per_wave = static_cast<size_t>(k_best) * pl * kLanes * sizeof(u64);
    const size_t fit = kLdsLimit / per_wave;
    return fit >= static_cast<size_t>(kWavesPerBlock) ? kWavesPerBlock : static_cast<int>(fit);
}

template <int EB, int PL> bool tile_is_aligned(const Args &a)
{
    constexpr int bytes = EB * PL;
    return (reinterpret_cast<uintptr_t>(a.tile) % bytes) == 0 && ((a.row_stride * EB) % bytes) == 0;
}

template <int EB, int PL, bool Smallest> int launch_top(const Args &a)
{
    const int waves = waves_per_block(a.k_or_cutoff, PL);
    const int64_t groups = (a.valid_count + PL * kLanes - 1) / (PL * kLanes);
    const size_t lds = static_cast<size_t>(waves) * a.k_or_cutoff * PL * kLanes * sizeof(u64);
    hipLaunchKernelGGL((top_queries_kernel<EB, PL, Smallest>), dim3(static_cast<unsigned>((groups + waves - 1) / waves)), dim3(waves * kLanes), lds,
                       a.stream, static_cast<const typename Elem<EB>::type *>(a.tile), a.n_queries, a.row_stride, a.valid_count, a.query_base,
                       a.k_or_cutoff, a.accumulate, tile_is_aligned<EB, PL>(a), a.scores, a.queries);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

template <int EB, int PL, bool Smallest> int launch_threshold(const Args &a)
{
    const int64_t groups = (a.valid_count + PL * kLanes - 1) / (PL * kLanes);
    hipLaunchKernelGGL((threshold_queries_kernel<EB, PL, Smallest>), dim3(static_cast<unsigned>((groups + kWavesPerBlock - 1) / kWavesPerBlock)),
                       dim3(256), 0, a.stream, static_cast<const typename Elem<EB>::type *>(a.tile), a.n_queries, a.row_stride, a.valid_count,
                       a.query_base, a.k_or_cutoff, a.accumulate, a.cap, tile_is_aligned<EB, PL>(a), a.counts, a.scores, a.queries);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

// The checks both calls share; everything here comes before the first HIP call.
int check_args(const char *who, const void *tile, int elem_bytes, int n_queries, int64_t row_stride, int64_t valid_count, int query_base,
               const void *d_workspace, size_t workspace_bytes)
{
    const char *why = nullptr;
    if (!tile) why = "the tile is NULL";
    else if (elem_bytes != 1 && elem_bytes != 2) why = "elem_bytes must be 1 or 2";
    else if (n_queries <= 0 || row_stride <= 0) why = "n_queries and row_stride must be positive";
    else if (valid_count < 0 || valid_count > row_stride) why = "valid_count must lie in [0, row_stride]";
    else if (query_base < 0 || static_cast<int64_t>(query_base) + n_queries > static_cast<int64_t>(INT32_MAX)) why = "query ids must lie in [0, 2^31 - 1]";
    else if (d_workspace && workspace_bytes < kWorkspaceBytes) why = "workspace smaller than bgsa_hip_query_hits_workspace_bytes()";
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

size_t bgsa_hip_query_hits_workspace_bytes(int n_queries, int64_t row_stride, int elem_bytes, int k_best)
{
    if (n_queries <= 0 || row_stride <= 0 || (elem_bytes != 1 && elem_bytes != 2) || k_best < 1) return 0;
    return kWorkspaceBytes;
}

int bgsa_hip_top_queries_dev(const void *d_results, int elem_bytes, int n_queries, int64_t row_stride, int64_t valid_count, int query_base,
                             int k_best, int smallest, int accumulate, int32_t *d_hit_scores, int32_t *d_hit_queries, void *d_workspace,
                             size_t workspace_bytes, void *stream)
{
    if (!d_hit_scores || !d_hit_queries) {
        set_error_text("top_queries_dev: an output list is NULL");
        return BGSA_HIP_EINVAL;
    }
    if (int rc = check_args("top_queries_dev", d_results, elem_bytes, n_queries, row_stride, valid_count, query_base, d_workspace, workspace_bytes))
        return rc;
    if (k_best < 1 || k_best > HIP_V_NUM) {
        set_error_text("top_queries_dev: k_best must lie in 1..64");
        return BGSA_HIP_EUNSUPPORTED;
    }
    if (valid_count == 0) return BGSA_HIP_OK;
    const Args a{d_results, elem_bytes, n_queries, row_stride, valid_count, query_base, k_best, smallest != 0, accumulate != 0, 0,
                 nullptr, d_hit_scores, d_hit_queries, static_cast<hipStream_t>(stream)};
    if (elem_bytes == 2) return a.smallest ? launch_top<2, 2, true>(a) : launch_top<2, 2, false>(a);
    // int8: four columns per lane while their heaps fit the LDS of one wave (k_best <= 32), two (a 16-bit load) beyond
    if (waves_per_block(k_best, 4) >= 1) return a.smallest ? launch_top<1, 4, true>(a) : launch_top<1, 4, false>(a);
    return a.smallest ? launch_top<1, 2, true>(a) : launch_top<1, 2, false>(a);
}

int bgsa_hip_threshold_queries_dev(const void *d_results, int elem_bytes, int n_queries, int64_t row_stride, int64_t valid_count,
                                   int query_base, int cutoff, int smallest, int accumulate, int cap_per_subject, int32_t *d_counts,
                                   int32_t *d_hit_scores, int32_t *d_hit_queries, void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (!d_counts || !d_hit_scores || !d_hit_queries || cap_per_subject <= 0) {
        set_error_text("threshold_queries_dev: an output is NULL or cap_per_subject is not positive");
        return BGSA_HIP_EINVAL;
    }
    if (int rc = check_args("threshold_queries_dev", d_results, elem_bytes, n_queries, row_stride, valid_count, query_base, d_workspace,
                            workspace_bytes))
        return rc;
    if (valid_count == 0) return BGSA_HIP_OK;
    const Args a{d_results, elem_bytes, n_queries, row_stride, valid_count, query_base, cutoff, smallest != 0, accumulate != 0, cap_per_subject,
                 d_counts, d_hit_scores, d_hit_queries, static_cast<hipStream_t>(stream)};
    if (elem_bytes == 2) return a.smallest ? launch_threshold<2, 2, true>(a) : launch_threshold<2, 2, false>(a);
    return a.smallest ? launch_threshold<1, 4, true>(a) : launch_threshold<1, 4, false>(a);
}

}  // extern "C"
