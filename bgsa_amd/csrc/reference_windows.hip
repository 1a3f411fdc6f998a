// reference_windows.hip — a reference sequence as the query set of a read placer: its overlapping windows cut on the device, on
// both strands, and the placements of the pair calls turned into reference coordinates (include/bgsa_hip.h "a reference as the
// query set").  Two small kernels; no scoring, selection or pair kernel knows about them.
//
// Geometry (the header states it; window_plan in bgsa_amd/reference.py restates it).  L mapped bytes, 1 <= S <= W <= L,
// n_windows = 1 + ceil((L - W) / S), start(w) = min(w * S, L - W).  Window id g in [0, n_windows) is forward window g; id
// n_windows + w is the reverse complement of window w: row i = comp(reference[start(w) + W - 1 - i]), comp(c) = 3 - c below 4,
// else 4.
//
// Window rows.  The output is ONE flat byte string of n_rows * (W + 1) bytes (W codes and '\n' per row) that may start at any
// byte address.  A thread owns one aligned dword of it: it divides once (flat offset -> row, column), walks its four bytes with
// a carry into the next row, and stores the dword — every store of a wave is one contiguous 256-byte piece.  The bytes in
// front of the first aligned dword and behind the last one are written byte by byte, by the threads that own those (partial)
// dwords, so nothing outside [0, n_rows * (W + 1)) is touched.  The reads are bytes of the reference: adjacent lanes read
// adjacent (forward) or mirrored (reverse) bytes, and every reference byte is read W / S times from the caches.  A window id
// only ever forms a value: an id outside [0, 2 n_windows) gives a row of code 4.
//
// Placements.  One wave per read, lane r = hit r of its list (k <= 64).  Coordinates and the reversal of a reverse hit's runs
// are per lane; `keep` walks the list once, hit r broadcasting its interval to the lanes behind it.
//
// No allocation, no synchronisation, no workspace.
#include "reference_geometry.h"   // Geometry, window_start, make_geometry

namespace bgsa {

namespace {

constexpr int kNewline = '\n';
constexpr int kCodeN = 4;
constexpr unsigned kMaxBlocks = 2048;   // a memory-bound grid: beyond it the threads stride

// Code `col` of the row of window id `id`; an id outside [0, 2 n_windows) is a row of N.
__device__ __forceinline__ unsigned window_code(const char *__restrict__ reference, const Geometry &g, int64_t id, int col)
{
    if (id < 0 || id >= 2 * g.n_windows) return kCodeN;
    if (id < g.n_windows) return static_cast<unsigned char>(reference[window_start(g, id) + col]);
    const unsigned c = static_cast<unsigned char>(reference[window_start(g, id - g.n_windows) + g.window_len - 1 - col]);
    return c < 4u ? 3u - c : static_cast<unsigned>(kCodeN);
}

__device__ __forceinline__ int64_t row_id(const int32_t *__restrict__ ids, int64_t first_id, int64_t row)
{
    return ids ? static_cast<int64_t>(ids[row]) : first_id + row;
}

// total = n_rows * (W + 1) bytes; lead = the output's address & 3.  Dword d covers the flat offsets [4d - lead, 4d - lead + 4):
// content + 4d - lead is dword aligned.  What lies below 0 (d == 0 only) or at and beyond `total` (the last dword only) belongs
// to somebody else and is not written; there are n_dwords = ceil((lead + total) / 4) of them, each with at least one own byte.
__global__ __launch_bounds__(256) void reference_windows_kernel(const char *__restrict__ reference, Geometry g, const int32_t *__restrict__ ids,
                                                                int64_t first_id, int64_t total, int lead, int64_t n_dwords,
                                                                char *__restrict__ content)
{
    const int row_bytes = g.window_len + 1;
    const int64_t step = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t d = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; d < n_dwords; d += step) {
        const int64_t lo = 4 * d - lead;                 // flat offset of the dword's first byte; negative only for d == 0
        const int64_t first = lo < 0 ? 0 : lo;
        int64_t row = first / row_bytes;
        int col = static_cast<int>(first - row * row_bytes);
        int64_t id = row_id(ids, first_id, row);         // first < total: the row exists
        unsigned word = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int64_t at = lo + b;
            if (at < 0 || at >= total) continue;
            const unsigned code = col == g.window_len ? static_cast<unsigned>(kNewline) : window_code(reference, g, id, col);
            word |= code << (8 * b);
            if (++col == row_bytes) {
                col = 0;
                row++;
                if (at + 1 < total) id = row_id(ids, first_id, row);   // the next row exists: its id may be read
            }
        }
        if (lo >= 0 && lo + 4 <= total) {
            *reinterpret_cast<unsigned *>(content + lo) = word;        // content + lo is dword aligned by the choice of lead
        } else {
#pragma unroll
            for (int b = 0; b < 4; b++)
                if (lo + b >= 0 && lo + b < total) content[lo + b] = static_cast<char>(word >> (8 * b));
        }
    }
}

// ---- placements: one wave per read, one lane per hit ----------------------------------------------------------------------
__global__ __launch_bounds__(256) void reference_placements_kernel(Geometry g, const int32_t *__restrict__ hit_windows, int64_t n_reads, int k,
                                                                   const int32_t *__restrict__ span, const int32_t *__restrict__ n_ops,
                                                                   int32_t *__restrict__ cigar, int cigar_cap, int32_t *__restrict__ strand_out,
                                                                   int64_t *__restrict__ begin_out, int64_t *__restrict__ end_out,
                                                                   int32_t *__restrict__ keep_out)
{
    const int lane = threadIdx.x & (kLanes - 1);
    const int64_t read = static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (read >= n_reads) return;     // wave-uniform
    const bool mine = lane < k;
    const int64_t p = read * k + lane;
    int strand = -1;
    long long begin = -1, end = -1;
    if (mine) {
        const int64_t id = hit_windows[p];
        if (id >= 0 && id < 2 * g.n_windows) {
            strand = id >= g.n_windows;
            const int qb = span[4 * p], qe = span[4 * p + 1];
            if (qb >= 0) {
                const int64_t at = window_start(g, strand ? id - g.n_windows : id);
                begin = strand ? at + g.window_len - qe : at + qb;
                end = strand ? at + g.window_len - qb : at + qe;
                if (strand && cigar) {
                    const int n = n_ops[p];
                    if (n > 1 && n <= cigar_cap) {
                        int32_t *runs = cigar + p * cigar_cap;
                        for (int a = 0, b = n - 1; a < b; a++, b--) {
                            const int32_t t = runs[a];
                            runs[a] = runs[b];
                            runs[b] = t;
                        }
                    }
                }
            }
        }
    }
    const bool placed = begin >= 0;
    bool hidden = false;             // a kept hit in front of this one has its strand and meets its interval
    bool keep = false;
    for (int r = 0; r < k; r++) {    // k is wave-uniform: every lane takes part in the shuffles
        const int kept = __shfl(static_cast<int>(placed && !hidden), r);   // lane r has heard from all lanes in front of it
        const int r_strand = __shfl(strand, r);
        const long long r_begin = __shfl(begin, r), r_end = __shfl(end, r);
        if (lane == r) keep = kept != 0;
        if (kept && lane > r && placed && strand == r_strand && begin < r_end && r_begin < end) hidden = true;
    }
    if (mine) {
        strand_out[p] = strand;
        begin_out[p] = begin;
        end_out[p] = end;
        keep_out[p] = keep ? 1 : 0;
    }
}

// The geometry's own checks with this file's longer word on a wide stride, shared by all four entry points.
int windows_geometry(const char *who, int64_t ref_len, int window_len, int stride, Geometry *out)
{
    return make_geometry(who, ref_len, window_len, stride, out, "the stride exceeds the window length (reference bases no window would hold)");
}

// ... and what the device calls add: window ids are int32.
int check_ids_fit(const char *who, const Geometry &g)
{
    if (2 * g.n_windows <= static_cast<int64_t>(INT32_MAX)) return BGSA_HIP_OK;
    char msg[200];
    snprintf(msg, sizeof msg, "%s: %lld windows on two strands do not fit int32 window ids (a larger stride, or the reference in parts)",
             who, static_cast<long long>(g.n_windows));
    set_error_text(msg);
    return BGSA_HIP_EINVAL;
}

}  // namespace

}  // namespace bgsa

using namespace bgsa;

extern "C" {

int64_t bgsa_hip_reference_window_count(int64_t ref_len, int window_len, int stride)
{
    Geometry g;
    return windows_geometry("reference_window_count", ref_len, window_len, stride, &g) ? -1 : g.n_windows;
}

int64_t bgsa_hip_reference_window_start(int64_t ref_len, int window_len, int stride, int64_t window)
{
    Geometry g;
    if (windows_geometry("reference_window_start", ref_len, window_len, stride, &g)) return -1;
    if (window < 0 || window >= g.n_windows) {
        set_error_text("reference_window_start: the window lies outside [0, n_windows)");
        return -1;
    }
    return window_start(g, window);
}

int bgsa_hip_reference_windows_dev(const char *d_reference, int64_t ref_len, int window_len, int stride, const int32_t *d_window_ids,
                                   int64_t first_id, int64_t n_rows, char *d_content, void *stream)
{
    if (!d_reference || !d_content) {
        set_error_text("reference_windows_dev: the reference or the content buffer is NULL");
        return BGSA_HIP_EINVAL;
    }
    Geometry g;
    if (int rc = windows_geometry("reference_windows_dev", ref_len, window_len, stride, &g)) return rc;
    if (int rc = check_ids_fit("reference_windows_dev", g)) return rc;
    if (n_rows < 0 || n_rows > static_cast<int64_t>(INT32_MAX)) {
        set_error_text("reference_windows_dev: n_rows must lie in [0, 2^31 - 1] (rows are query indices)");
        return BGSA_HIP_EINVAL;
    }
    if (!d_window_ids && (first_id < 0 || first_id > 2 * g.n_windows || n_rows > 2 * g.n_windows - first_id)) {
        set_error_text("reference_windows_dev: the id range must lie in [0, 2 * n_windows)");
        return BGSA_HIP_EINVAL;
    }
    if (n_rows == 0) return BGSA_HIP_OK;
    const int64_t total = n_rows * (static_cast<int64_t>(window_len) + 1);
    const int lead = static_cast<int>(reinterpret_cast<uintptr_t>(d_content) & 3);
    const int64_t n_dwords = (lead + total + 3) / 4;
    const int64_t blocks = (n_dwords + 255) / 256;
    hipLaunchKernelGGL(reference_windows_kernel, dim3(static_cast<unsigned>(blocks < kMaxBlocks ? blocks : kMaxBlocks)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), d_reference, g, d_window_ids, d_window_ids ? 0 : first_id, total, lead, n_dwords,
                       d_content);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

int bgsa_hip_reference_placements_dev(int64_t ref_len, int window_len, int stride, const int32_t *d_hit_windows, int64_t n_reads, int k,
                                      const int32_t *d_span, const int32_t *d_n_ops, int32_t *d_cigar, int cigar_cap, int32_t *d_strand,
                                      int64_t *d_ref_begin, int64_t *d_ref_end, int32_t *d_keep, void *stream)
{
    if (!d_hit_windows || !d_span || !d_strand || !d_ref_begin || !d_ref_end || !d_keep) {
        set_error_text("reference_placements_dev: the hit windows, the spans or an output is NULL");
        return BGSA_HIP_EINVAL;
    }
    if ((d_cigar != nullptr) != (d_n_ops != nullptr) || (d_cigar && cigar_cap < 1)) {
        set_error_text("reference_placements_dev: d_n_ops and d_cigar come together (both NULL: no runs to reverse), with a positive cigar_cap");
        return BGSA_HIP_EINVAL;
    }
    Geometry g;
    if (int rc = windows_geometry("reference_placements_dev", ref_len, window_len, stride, &g)) return rc;
    if (int rc = check_ids_fit("reference_placements_dev", g)) return rc;
    if (k < 1 || k > HIP_V_NUM) {
        set_error_text("reference_placements_dev: k must lie in 1..64 (one wavefront holds a read's list, one hit per lane)");
        return BGSA_HIP_EINVAL;
    }
    if (n_reads < 0 || n_reads > static_cast<int64_t>(INT32_MAX) * kWavesPerBlock) {
        set_error_text("reference_placements_dev: n_reads is negative or beyond one launch");
        return BGSA_HIP_EINVAL;
    }
    if (n_reads == 0) return BGSA_HIP_OK;
    hipLaunchKernelGGL(reference_placements_kernel, dim3(static_cast<unsigned>((n_reads + kWavesPerBlock - 1) / kWavesPerBlock)),
                       dim3(kWavesPerBlock * kLanes), 0, static_cast<hipStream_t>(stream), g, d_hit_windows, n_reads, k, d_span, d_n_ops,
                       d_cigar, cigar_cap, d_strand, d_ref_begin, d_ref_end, d_keep);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

}  // extern "C"
