// contigs.hip — a reference of several contigs (include/bgsa_hip.h "a reference of several contigs"): the
// layout of the contigs in ONE mapped reference, and the kernel that rewrites every placed hit so that it lies inside its contig.
// Every scoring, selection and placement call runs unchanged on the padded reference; what is new sits behind them.
//
// Layout (the header states it; bgsa_amd/reference.py: contig_layout and tests/contig_reference.py restate it).  Contigs i =
// 0..C-1 of len_i >= 1 bases, P >= W bytes of 'N' between neighbours: start_0 = 0, start_{i+1} = start_i + len_i + P, total =
// start_{C-1} + len_{C-1}.  With P >= W no window holds bases of two contigs.
//
// clip   one wave per read, one lane per slot of its hit list.  A lane finds its hit's contig by binary search on the starts,
//        walks its runs from the front for the columns in front of the contig and from the back for those behind it — both
//        walks only read, and leave what they found in registers: how many runs they passed, the read bases they turned into
//        read-only ones, the rest of the run they split —, moves the untouched middle by at most one place and writes the at
//        most two new runs on either side.  keep is then walked once more over the clipped intervals, as
//        reference_placements_kernel walks it.  Ids, coordinates and run lengths are values until compared with the extents the
//        caller states; a run index never leaves [0, min(n_ops, cigar_cap)).  No LDS, no scratch, vector stores only.
#include "bgsa_common.h"

#include <limits.h>

namespace bgsa {

namespace {

constexpr int kOpRefOnly = 1, kOpReadOnly = 2, kOpEqual = 7;      // the project's run codes; 8 (X) is what is left

__device__ __forceinline__ uint32_t run_word(long long len, int op) { return static_cast<uint32_t>(len) << 4 | static_cast<uint32_t>(op); }

// What one walk over the columns outside the contig found.  `passed` runs were consumed or split; `read` read bases became (or
// were, and merge into) the read-only run at that edge; `rest` bases of the split run, of op `rest_op`, stay; `delta` is what
// the distance changes by.
struct Edge {
    int passed;
    long long read, rest, delta;
    int rest_op;
};

// `columns` reference columns of one run, (len, op), leave the hit: a reference-only column is dropped, an X or = column becomes a
// read-only base.  Returns the columns taken.
__device__ __forceinline__ long long take_columns(long long len, int op, long long columns, Edge &e)
{
    const long long t = len < columns ? len : columns;
    if (op == kOpRefOnly) {
        e.delta -= t;
    } else {
        e.read += t;
        if (op == kOpEqual) e.delta += t;
    }
    e.rest = len - t;
    e.rest_op = op;
    return t;
}

__global__ __launch_bounds__(256) void contig_clip_kernel(const int64_t *__restrict__ starts, const int64_t *__restrict__ lens, int n_contigs,
                                                          int64_t ref_len, int64_t n_reads, int k, int32_t *__restrict__ scores,
                                                          const int32_t *__restrict__ strand_in, int64_t *__restrict__ begin_io,
                                                          int64_t *__restrict__ end_io, int32_t *__restrict__ keep_out,
                                                          int32_t *__restrict__ n_ops_io, uint32_t *__restrict__ cigar, int cigar_cap,
                                                          int32_t *__restrict__ contig_out)
{
    const int lane = threadIdx.x & (kLanes - 1);
    const int64_t read = static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (read >= n_reads) return;     // wave-uniform
    const bool mine = lane < k;
    const int64_t p = read * k + lane;
    int strand = -1, contig = -1;
    long long begin = -1, end = -1;
    if (mine) {
        strand = strand_in[p];
        begin = begin_io[p];
        end = end_io[p];
    }
    if (mine && begin >= 0) {
        const int n_old = n_ops_io[p];
        long long c_start = 0, c_end = 0;
        if (begin <= end && end <= ref_len) {
            int lo = 0, hi = n_contigs;             // the contigs whose start is <= begin are [0, lo)
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if (starts[mid] <= begin) lo = mid + 1; else hi = mid;
            }
            for (int c = lo - 1; c <= lo && contig < 0; c++) {      // the one that holds begin, or the first one behind it
                if (c < 0 || c >= n_contigs) continue;
                const long long s = starts[c], n = lens[c];
                const bool meets = begin < end ? begin < s + n && s < end : s <= begin && begin <= s + n;   // an empty interval: in or at the contig
                if (n >= 1 && s >= 0 && s <= ref_len - n && meets) {
                    contig = c;
                    c_start = s;
                    c_end = s + n;
                }
            }
        }
        if (contig < 0) {                                           // no contig base: unplaced
            begin = end = -1;
            n_ops_io[p] = 0;
        } else if (n_old >= 0 && n_old <= cigar_cap) {              // (a row that overflowed before is left as it is)
            const long long lead = c_start > begin ? c_start - begin : 0, trail = end > c_end ? end - c_end : 0;
            uint32_t *runs = cigar + p * cigar_cap;
            Edge front{0, 0, 0, 0, 0}, back{0, 0, 0, 0, 0};
            if (lead > 0) {
                long long left = lead;
                while (front.passed < n_old && (left > 0 || (front.rest == 0 && (runs[front.passed] & 15u) == kOpReadOnly))) {
                    const uint32_t word = runs[front.passed++];
                    const int op = static_cast<int>(word & 15u);
                    const long long len = word >> 4;
                    if (op == kOpReadOnly) front.read += len;
                    else left -= take_columns(len, op, left, front);
                }
            }
            // the walk from the back sees the front's result: the runs [front.passed, n_old), and below them the rest of its split run
            const int floor = front.passed;
            int top = n_old;                                        // the runs [floor, top) are untouched by both walks
            if (trail > 0) {
                long long left = trail;
                while (top > floor && (left > 0 || (back.rest == 0 && (runs[top - 1] & 15u) == kOpReadOnly))) {
                    const uint32_t word = runs[--top];
                    const int op = static_cast<int>(word & 15u);
                    const long long len = word >> 4;
                    back.passed++;
                    if (op == kOpReadOnly) back.read += len;
                    else left -= take_columns(len, op, left, back);
                }
                if (left > 0 && front.rest > 0) {                   // one run holds the contig: its rest is cut once more
                    take_columns(front.rest, front.rest_op, left, back);
                    front.rest = back.rest;
                    back.rest = 0;
                }
            }
            const int head = (front.read > 0) + (front.rest > 0), tail = (back.rest > 0) + (back.read > 0);
            const int middle = top - floor;
            const int n_new = head + middle + tail;
            begin += lead;
            end -= trail;
            scores[p] = static_cast<int32_t>(static_cast<long long>(scores[p]) - front.delta - back.delta);
            n_ops_io[p] = n_new;
            if (n_new <= cigar_cap && (lead > 0 || trail > 0)) {
                if (head < floor) {
                    for (int i = 0; i < middle; i++) runs[head + i] = runs[floor + i];
                } else if (head > floor) {
                    for (int i = middle - 1; i >= 0; i--) runs[head + i] = runs[floor + i];
                }
                int at = 0;
                if (front.read > 0) runs[at++] = run_word(front.read, kOpReadOnly);
                if (front.rest > 0) runs[at++] = run_word(front.rest, front.rest_op);
                at += middle;
                if (back.rest > 0) runs[at++] = run_word(back.rest, back.rest_op);
                if (back.read > 0) runs[at++] = run_word(back.read, kOpReadOnly);
            }
        }
    }
    const bool placed = begin >= 0;
    bool hidden = false, keep = false;       // reference_placements_kernel's walk, on the clipped intervals
    for (int r = 0; r < k; r++) {            // k is wave-uniform: every lane takes part in the shuffles
        const int kept = __shfl(static_cast<int>(placed && !hidden), r);
        const int r_strand = __shfl(strand, r);
        const long long r_begin = __shfl(begin, r), r_end = __shfl(end, r);
        if (lane == r) keep = kept != 0;
        if (kept && lane > r && placed && strand == r_strand && begin < r_end && r_begin < end) hidden = true;
    }
    if (mine) {
        begin_io[p] = begin;
        end_io[p] = end;
        keep_out[p] = keep ? 1 : 0;
        contig_out[p] = contig;
    }
}

}  // namespace

}  // namespace bgsa

using namespace bgsa;

extern "C" {

int bgsa_hip_contig_layout(const int64_t *lens, int64_t n_contigs, int window_len, int64_t padding, int64_t *starts_out, int64_t *total_out)
{
    const char *who = "contig_layout";
    if (!lens || !starts_out || !total_out) return refuse(who, BGSA_HIP_EINVAL, "a NULL pointer");
    if (n_contigs < 1) return refuse(who, BGSA_HIP_EINVAL, "n_contigs is not positive");
    if (window_len < 1 || padding < window_len)
        return refuse(who, BGSA_HIP_EINVAL, "padding is below window_len (a window would hold bases of two contigs), or window_len is not positive");
    int64_t at = 0;
    for (int64_t i = 0; i < n_contigs; i++) {
        if (lens[i] < 1) return refuse(who, BGSA_HIP_EINVAL, "a contig length is below 1");
        if (i > 0) {
            if (at > INT64_MAX - padding) return refuse(who, BGSA_HIP_EINVAL, "the padded contigs do not fit int64");
            at += padding;
        }
        starts_out[i] = at;
        if (at > INT64_MAX - lens[i]) return refuse(who, BGSA_HIP_EINVAL, "the padded contigs do not fit int64");
        at += lens[i];
    }
    *total_out = at;
    return BGSA_HIP_OK;
}

int bgsa_hip_contig_clip_dev(const int64_t *d_starts, const int64_t *d_lens, int64_t n_contigs, int64_t ref_len, int64_t n_reads, int k,
                             int32_t *d_scores, const int32_t *d_strand, int64_t *d_ref_begin, int64_t *d_ref_end, int32_t *d_keep,
                             int32_t *d_n_ops, int32_t *d_cigar, int cigar_cap, int32_t *d_contig, void *stream)
{
    const char *who = "contig_clip_dev";
    if (!d_starts || !d_lens || !d_scores || !d_strand || !d_ref_begin || !d_ref_end || !d_keep || !d_n_ops || !d_cigar || !d_contig)
        return refuse(who, BGSA_HIP_EINVAL, "a NULL pointer (only the stream may be NULL)");
    if (n_contigs < 1 || n_contigs > static_cast<int64_t>(INT32_MAX)) return refuse(who, BGSA_HIP_EINVAL, "n_contigs must lie in [1, 2^31 - 1]");
    if (ref_len < 1) return refuse(who, BGSA_HIP_EINVAL, "ref_len is not positive");
    if (k < 1 || k > HIP_V_NUM) return refuse(who, BGSA_HIP_EINVAL, "k must lie in 1..64 (one wavefront holds a read's list, one slot per lane)");
    if (cigar_cap < 1) return refuse(who, BGSA_HIP_EINVAL, "cigar_cap is not positive");
    if (n_reads < 0 || n_reads > static_cast<int64_t>(INT32_MAX) * kWavesPerBlock) return refuse(who, BGSA_HIP_EINVAL, "n_reads is negative or beyond one launch");
    if (n_reads == 0) return BGSA_HIP_OK;
    hipLaunchKernelGGL(contig_clip_kernel, dim3(static_cast<unsigned>((n_reads + kWavesPerBlock - 1) / kWavesPerBlock)),
                       dim3(kWavesPerBlock * kLanes), 0, static_cast<hipStream_t>(stream), d_starts, d_lens, static_cast<int>(n_contigs), ref_len,
                       n_reads, k, d_scores, d_strand, d_ref_begin, d_ref_end, d_keep, d_n_ops, reinterpret_cast<uint32_t *>(d_cigar), cigar_cap,
                       d_contig);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

}  // extern "C"
