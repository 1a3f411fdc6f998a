// pair_trace.h — what the two pair tracebacks share (align_pairs.hip: the Myers bit-parallel forward; trace_pairs.hip: the
// scalar forward of every linear-gap score set and the semi-global modes): the argument block, which pairs a call owns, the
// history's addressing and the run-length tail.  Internal, not installed.
#pragma once

#include "bgsa_common.h"

namespace bgsa {

constexpr int kOpI = 1, kOpD = 2, kOpEq = 7, kOpX = 8;   // BAM op codes
constexpr int kRowBlock = 8;                             // query characters fetched ahead of their rows
constexpr int64_t kMaxChunkWaves = 1 << 22;              // waves of one launch, whatever the workspace would hold

struct PairArgs {
    const char *content;
    const uint32_t *peq;
    int ref_len, read_len;
    int64_t read_count;
    int word_num;
    const int32_t *pair_query;
    const int64_t *pair_subject;
    int64_t n_pairs;
    int n_queries;
    int64_t subject_base;
    int32_t *distance, *n_ops;       // trace_pairs: `distance` is d_score
    uint32_t *cigar;
    int cigar_cap;
    unsigned char *workspace;
    size_t wave_bytes, hist_bytes;   // one wave's slice, and the history at its head (the op bytes follow)
    unsigned *fault_word;
    const int32_t *read_lens;        // a bucket of mixed subject lengths: one entry per column (read_len = the longest), or nullptr
};

// The subject length of the pair in column `col`: its own in a mixed-length bucket (lane_read_len: clamped to [0, read_len]).
__device__ __forceinline__ int pair_read_len(const PairArgs &a, int64_t col)
{
    return a.read_lens ? lane_read_len(a.read_lens, static_cast<size_t>(col), a.read_len) : a.read_len;
}

// History: two bit vectors per row and word, [chunk wave][row][vector A|B][word][lane] uint32.  A bit j = the step at
// (row, column j) is diagonal; B bit j = on a diagonal step '=' (1) or 'X' (0), otherwise up 'I' (1) or left 'D' (0).
inline size_t pair_hist_bytes(int ref_len, int read_len)
{
    return static_cast<size_t>(ref_len) * 2 * ((read_len + 31) / 32) * kLanes * sizeof(uint32_t);
}
inline size_t pair_wave_bytes(int ref_len, int read_len)
{
    const size_t ops = (static_cast<size_t>(ref_len) + static_cast<size_t>(read_len)) * kLanes;   // one byte per step and lane
    return (pair_hist_bytes(ref_len, read_len) + ops + 255) & ~static_cast<size_t>(255);
}

// Whether this call owns pair p, and its query and column.  A pair of another bucket (or the unused slot -1) is not
// owned; an owned pair whose query index is out of range is skipped too and — in the forward kernel — reported.
__device__ __forceinline__ bool owned_pair(const PairArgs &a, int64_t p, bool report, int *q, int64_t *col)
{
    if (p >= a.n_pairs) return false;
    const int64_t s = a.pair_subject[p];
    if (s < a.subject_base || static_cast<unsigned long long>(s) - static_cast<unsigned long long>(a.subject_base) >=
                                  static_cast<unsigned long long>(a.read_count))
        return false;
    *col = s - a.subject_base;
    *q = a.pair_query[p];
    if (*q < 0 || *q >= a.n_queries) {
        if (report) atomicOr(a.fault_word, static_cast<unsigned>(BGSA_HIP_FAULT_PAIR));
        return false;
    }
    return true;
}

// The canonical step at the interior cell (i, j), i, j > 0, from the lane's history (hist = the wave's slice + lane):
// the op, and i / j moved to the cell the step came from.
__device__ __forceinline__ int history_step(const uint32_t *hist, size_t row_words, int wn, int *i, int *j)
{
    const uint32_t *cell = hist + static_cast<size_t>(*i - 1) * row_words + static_cast<size_t>((*j - 1) >> 5) * kLanes;
    const uint32_t diag = (cell[0] >> ((*j - 1) & 31)) & 1u;
    const uint32_t which = (cell[static_cast<size_t>(wn) * kLanes] >> ((*j - 1) & 31)) & 1u;
    if (diag) {
        (*i)--;
        (*j)--;
        return which ? kOpEq : kOpX;
    }
    if (which) {
        (*i)--;
        return kOpI;
    }
    (*j)--;
    return kOpD;
}

// Run-length encodes the lane's op bytes ops[step * kLanes] forwards — the last step written is the first column — into
// at most `cap` runs at `out`; returns the true number of runs.
__device__ __forceinline__ int encode_runs(const unsigned char *ops, size_t steps, uint32_t *out, int cap)
{
    int n_runs = 0;
    uint32_t run_op = 0, run_len = 0;
    for (size_t t = steps; t-- > 0;) {
        const uint32_t op = ops[t * kLanes];
        if (op == run_op) {
            run_len++;
            continue;
        }
        if (run_len) {
            if (n_runs < cap) out[n_runs] = (run_len << 4) | run_op;
            n_runs++;
        }
        run_op = op;
        run_len = 1;
    }
    if (run_len) {
        if (n_runs < cap) out[n_runs] = (run_len << 4) | run_op;
        n_runs++;
    }
    return n_runs;
}

}  // namespace bgsa
