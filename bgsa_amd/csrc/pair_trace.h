// pair_trace.h — what the pair kernels share (align_pairs.hip, trace_pairs.hip, align_pairs_banded.hip, place_pairs_banded.hip
// and the verify kernel of seed_map.hip): the argument block, which pairs a call owns, a lane's class as masks over the Peq
// planes (the Myers word itself is myers_word of bgsa_common.h), the stored state of the windowed kernels and its score, the
// history's addressing, the run-length tail, and on the host the chunk loop, the workspace rule and the entry prologue.
// Internal, not installed.
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

// The lane's class nibble as five all-or-nothing masks: the Eq word is a branch-free and/or over the subject's planes.
// Exact == true: a code above 4 — block_classes' 15, a row that does not exist — matches nothing.  Exact == false: class 0
// stands for "none of 1..4", which is the same for the codes 0..4 of the global kernels and keeps their registers as they were
// (LABNOTES §31.2).
struct ClassMasks {
    uint32_t k[kChars];
};
template <bool Exact>
__device__ __forceinline__ ClassMasks class_masks(uint32_t c)
{
    if (Exact) return {{0u - (c == 0), 0u - (c == 1), 0u - (c == 2), 0u - (c == 3), 0u - (c == 4)}};
    const uint32_t k1 = 0u - (c == 1), k2 = 0u - (c == 2), k3 = 0u - (c == 3), k4 = 0u - (c == 4);
    return {{~(k1 | k2 | k3 | k4), k1, k2, k3, k4}};
}
template <int NW>
__device__ __forceinline__ uint32_t class_eq(const uint32_t (&peq)[kChars][NW], int w, const ClassMasks &m)
{
    return (peq[0][w] & m.k[0]) | (peq[1][w] & m.k[1]) | (peq[2][w] & m.k[2]) | (peq[3][w] & m.k[3]) | (peq[4][w] & m.k[4]);
}

// The next row's class from a block's 32 nibbles.
__device__ __forceinline__ uint32_t next_class(unsigned long long &lo, unsigned long long &hi)
{
    const uint32_t c = static_cast<uint32_t>(lo) & 15u;
    lo = (lo >> 4) | (hi << 60);
    hi >>= 4;
    return c;
}

// A stored state [pv | mv][word][lane] at its start ...
__device__ __forceinline__ void state_init(uint32_t *state, int wn)
{
    for (int w = 0; w < wn; w++) {
        state[static_cast<size_t>(w) * kLanes] = ~0u;
        state[static_cast<size_t>(wn + w) * kLanes] = 0u;
    }
}
// ... and its score at column n: `rows`, the rows run with hp_in = 1, plus the sum over all words of popc(pv & mask) - popc(mv & mask).
__device__ __forceinline__ int state_score(const uint32_t *state, int wn, int n, int rows)
{
    int score = rows;
    for (int w = 0; w < wn; w++) {
        const int rem = n - 32 * w;
        const uint32_t mask = rem >= 32 ? ~0u : ((1u << rem) - 1u);   // rem >= 1: w < word_num
        score += __popc(state[static_cast<size_t>(w) * kLanes] & mask) - __popc(state[static_cast<size_t>(wn + w) * kLanes] & mask);
    }
    return score;
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

// ---- host: the chunk loop, the workspace rule, the entry prologue --------------------------------------------------------------
// The pair list in chunks of as many whole waves as the workspace holds, launch(grid, first) one after the other.
// wave_bytes == 0: the kernels need no workspace, a chunk is the most waves of one launch.
template <typename F>
int for_each_chunk(int64_t n_pairs, size_t wave_bytes, size_t workspace_bytes, F &&launch)
{
    int64_t chunk_waves = wave_bytes ? static_cast<int64_t>(workspace_bytes / wave_bytes) : kMaxChunkWaves;
    if (chunk_waves > kMaxChunkWaves) chunk_waves = kMaxChunkWaves;
    for (int64_t first = 0; first < n_pairs; first += chunk_waves * kLanes) {
        const int64_t left = (n_pairs - first + kLanes - 1) / kLanes;
        if (int rc = launch(dim3(static_cast<unsigned>(left < chunk_waves ? left : chunk_waves)), first)) return rc;
    }
    return BGSA_HIP_OK;
}

// What a call without a workspace of the caller's takes for n_pairs pairs at `per` bytes a wave.
inline size_t pair_workspace_for(size_t per, int64_t n_pairs)
{
    const size_t cap = BGSA_HIP_ALIGN_PAIRS_MAX_WORKSPACE;
    const unsigned long long waves = n_pairs > 0 ? (static_cast<unsigned long long>(n_pairs) + kLanes - 1) / kLanes : 1;
    const size_t want = waves > cap / per ? cap : static_cast<size_t>(waves) * per;   // min(all pairs in one pass, the cap)
    return want > per ? want : per;                                                    // one wave always fits
}

// The chunk loop on the caller's workspace, or on the library's own scratch of pair_workspace_for(per, n_pairs) bytes:
// launch(workspace, grid, first) per chunk.
template <typename F>
int run_pair_chunks(void *d_workspace, size_t workspace_bytes, size_t per, int64_t n_pairs, hipStream_t stream, F &&launch)
{
    auto run = [&](void *workspace, size_t bytes) {
        return for_each_chunk(n_pairs, per, bytes,
                              [&](dim3 grid, int64_t first) { return launch(static_cast<unsigned char *>(workspace), grid, first); });
    };
    if (d_workspace) return run(d_workspace, workspace_bytes);
    const size_t own = pair_workspace_for(per, n_pairs);
    auto on_own = [&](void *workspace) { return run(workspace, own); };
    return with_own_scratch(stream, own, [](void *workspace, void *ctx) { return (*static_cast<decltype(on_own) *>(ctx))(workspace); }, &on_own);
}

// The head of the four pair entries' checks, in their order; the caller says whether one of its pointers is NULL and how it
// words that.  The word_num and workspace checks follow in each entry, trace_pairs.hip's params checks between them.
inline int check_pair_call(const char *who, bool null_pointer, const char *null_text, int64_t n_pairs, int ref_len, int read_len, int n_queries,
                           int cigar_cap, int64_t read_count)
{
    if (null_pointer) return refuse(who, BGSA_HIP_EINVAL, null_text);
    if (n_pairs < 0) return refuse(who, BGSA_HIP_EINVAL, "n_pairs is negative");
    if (ref_len <= 0 || read_len <= 0 || n_queries <= 0 || cigar_cap <= 0)
        return refuse(who, BGSA_HIP_EINVAL, "ref_len, read_len, n_queries and cigar_cap must be positive");
    if (read_count <= 0 || read_count % HIP_V_NUM != 0) return refuse(who, BGSA_HIP_EINVAL, "read_count must be a positive multiple of 64");
    return BGSA_HIP_OK;
}

}  // namespace bgsa
