// trace_pairs.hip — score, aligned span and canonical edit script (CIGAR) of a list of (query, subject) pairs for every
// aligner that has an alignment to report: any linear-gap score set in global mode, BitPAl semi-global (query end to end,
// free subject overhangs) and Myers semi-global (subject end to end inside the query)
// (include/bgsa_hip.h "score, span and edit script of selected pairs").
//
// As in align_pairs.hip a lane owns one PAIR and a wave 64 of them, and a chunk of pairs runs two kernels:
//
//   forward    a plain scalar DP per lane, row by row: H[i][j] = max(H[i-1][j-1] + s, H[i-1][j] + gap, H[i][j-1] + gap).
//              The lane's DP row lives in LDS as int16 [column][lane] (conflict-free: the lanes of a column are
//              contiguous), H[i-1][j-1] and H[i][j-1] travel in registers.  The scores are kernel arguments, so one body
//              serves every score set and nothing here depends on the BitPAl sets the library was built with.  Whether
//              q_i matches s_j is bit j of the lane's word of the Peq plane of class q_i, gathered from the (L2-resident)
//              Peq block one word ahead of its use.  Per row and 32 columns the two history words of align_pairs.hip are
//              accumulated in registers and stored once: the history has exactly that file's layout, and every wave store
//              is a coalesced 256-byte row.  The kernel also finds the end cell of its mode and leaves the score in
//              d_score and (q_end, s_end) in d_span.
//   traceback  the walk of align_pairs.hip, started at the end cell read from d_span and stopped where the mode says;
//              fills q_begin / s_begin, then run-length encodes forwards under cigar_cap.
//
// A scalar DP because of proportion: the traced pairs are ~1e-5 of the cells a job scores, and a per-lane BitPAl row would
// need the generated body rewritten for per-lane query characters once per score set (LABNOTES §16).
#include "pair_trace.h"

#include <algorithm>
#include <cstdlib>
#include <mutex>

namespace bgsa {

namespace {

// What is free.  kGlobal: nothing.  kFreeQuery (Myers semi-global): the first column is 0 and the best cell of the last
// column ends the alignment.  kFreeSubject (BitPAl semi-global): the first row is 0 and the best cell of the last row does.
enum TraceMode { kGlobal = 0, kFreeQuery = 1, kFreeSubject = 2 };

constexpr size_t kLdsOptIn = 64 * 1024;   // dynamic LDS beyond this needs hipFuncAttributeMaxDynamicSharedMemorySize

struct TraceArgs {
    PairArgs p;          // p.distance = d_score
    int32_t *span;       // [pair][q_begin, q_end, s_begin, s_end]
    int match, mismatch, gap;
    int mode;
};

inline size_t trace_lds_bytes(int read_len) { return (static_cast<size_t>(read_len) + 1) * kLanes * sizeof(int16_t); }

template <int MODE>
__global__ __launch_bounds__(kLanes) void trace_pairs_forward_kernel(TraceArgs t, int64_t first)
{
    extern __shared__ int16_t dp_row[];   // [column 0..n][lane]: |H| <= max|score| * (m + n) <= 32767 (checked by the entry point)
    const PairArgs &a = t.p;
    const int lane = threadIdx.x;
    const int64_t p = first + static_cast<int64_t>(blockIdx.x) * kLanes + lane;
    int q = 0;
    int64_t col = 0;
    if (!owned_pair(a, p, true, &q, &col)) return;   // no barrier below: a lane's DP row is its own
    const int wn = a.word_num, m = a.ref_len, n = pair_read_len(a, col);   // a mixed-length bucket (global mode): the pair's own n
    const int match = t.match, mismatch = t.mismatch, gap = t.gap;

    int16_t *hrow = dp_row + lane;
    for (int j = 0; j <= n; j++) hrow[static_cast<size_t>(j) * kLanes] = static_cast<int16_t>(MODE == kFreeSubject ? 0 : j * gap);

    // the subject's Peq planes: [group][class][word][lane]
    const uint32_t *g = a.peq + static_cast<size_t>(col >> 6) * kChars * wn * kLanes + (col & (kLanes - 1));
    const unsigned char *row = reinterpret_cast<const unsigned char *>(a.content) + static_cast<size_t>(q) * (m + 1);
    uint32_t *h = reinterpret_cast<uint32_t *>(a.workspace + static_cast<size_t>(blockIdx.x) * a.wave_bytes) + lane;
    const size_t row_words = static_cast<size_t>(2) * wn * kLanes;

    int last = n * gap;                 // H[i][n] of the row just finished
    int best = last, best_i = 0;        // kFreeQuery: the running best of the last column, the smallest such row
    for (int i0 = 0; i0 < m; i0 += kRowBlock) {
        // the block's characters first, four bits each: a load waits for every older store of the wave, so one wait per
        // block instead of one per row
        uint32_t codes = 0;
#pragma unroll
        for (int r = 0; r < kRowBlock; r++) {
            uint32_t c = i0 + r < m ? row[i0 + r] : 0u;
            if (c > 4) c = 0;   // as the packed streams: out-of-alphabet bytes behave as 'A'
            codes |= c << (4 * r);
        }
        const int rows = m - i0 < kRowBlock ? m - i0 : kRowBlock;
#pragma unroll 1
        for (int r = 0; r < rows; r++) {
            const int i = i0 + r + 1;
            const uint32_t c = (codes >> (4 * r)) & 15u;
            const uint32_t *eqp = g + static_cast<size_t>(c) * wn * kLanes;   // the lane's words of plane class(q_i)
            uint32_t eq_next = eqp[0];
            int diag = hrow[0];                               // H[i-1][0]
            int left = MODE == kFreeQuery ? 0 : i * gap;      // H[i][0]
            hrow[0] = static_cast<int16_t>(left);
#pragma unroll 1
            for (int w = 0; w < wn; w++) {
                const uint32_t eq = eq_next;
                if (w + 1 < wn) eq_next = eqp[static_cast<size_t>(w + 1) * kLanes];   // one word ahead of its use
                const int cols = n - 32 * w < 32 ? n - 32 * w : 32;
                int16_t *cell = hrow + (static_cast<size_t>(32) * w + 1) * kLanes;
                uint32_t step_diag = 0, step_which = 0;
#pragma unroll 4
                for (int b = 0; b < cols; b++) {
                    const int up = cell[static_cast<size_t>(b) * kLanes];          // H[i-1][j]
                    const uint32_t e = (eq >> b) & 1u;
                    const int d = diag + (e ? match : mismatch);
                    const int u = up + gap;
                    const int l = left + gap;
                    const int hv = max(d, max(u, l));
                    const uint32_t is_d = d == hv, is_u = u == hv;
                    step_diag |= is_d << b;
                    step_which |= (is_d ? e : is_u) << b;
                    cell[static_cast<size_t>(b) * kLanes] = static_cast<int16_t>(hv);
                    diag = up;
                    left = hv;
                }
                h[static_cast<size_t>(w) * kLanes] = step_diag;
                h[static_cast<size_t>(wn + w) * kLanes] = step_which;
            }
            h += row_words;
            last = left;
            if (MODE == kFreeQuery && last > best) {   // strict: the smallest row among equals
                best = last;
                best_i = i;
            }
        }
    }

    int q_end = m, s_end = n;
    if (MODE == kGlobal) best = last;
    if (MODE == kFreeQuery) q_end = best_i;
    if (MODE == kFreeSubject) {   // the best cell of the last row, the smallest such column
        best = hrow[0];
        s_end = 0;
        for (int j = 1; j <= n; j++) {
            const int v = hrow[static_cast<size_t>(j) * kLanes];
            if (v > best) {
                best = v;
                s_end = j;
            }
        }
    }
    a.distance[p] = best;
    t.span[4 * p + 1] = q_end;
    t.span[4 * p + 3] = s_end;
}

__global__ __launch_bounds__(kLanes) void trace_pairs_traceback_kernel(TraceArgs t, int64_t first)
{
    const PairArgs &a = t.p;
    const int lane = threadIdx.x;
    const int64_t p = first + static_cast<int64_t>(blockIdx.x) * kLanes + lane;
    int q = 0;
    int64_t col = 0;
    if (!owned_pair(a, p, false, &q, &col)) return;
    const int wn = a.word_num;
    unsigned char *slice = a.workspace + static_cast<size_t>(blockIdx.x) * a.wave_bytes;
    const uint32_t *hist = reinterpret_cast<const uint32_t *>(slice) + lane;
    unsigned char *ops = slice + a.hist_bytes + lane;   // [step][lane]
    const size_t row_words = static_cast<size_t>(2) * wn * kLanes;

    // the end cell the forward kernel of this chunk left: 0 <= i <= m, 0 <= j <= n, so at most m + n steps
    int i = t.span[4 * p + 1], j = t.span[4 * p + 3];
    size_t steps = 0;
    for (;;) {
        // where the walk stops: the origin, or the first cell of the free edge
        if (t.mode == kGlobal ? (i == 0 && j == 0) : (t.mode == kFreeQuery ? j == 0 : i == 0)) break;
        int op;
        if (i == 0) {
            op = kOpD;
            j--;
        } else if (j == 0) {
            op = kOpI;
            i--;
        } else {
            op = history_step(hist, row_words, wn, &i, &j);
        }
        ops[steps * kLanes] = static_cast<unsigned char>(op);
        steps++;
    }
    t.span[4 * p + 0] = i;
    t.span[4 * p + 2] = j;
    a.n_ops[p] = encode_runs(ops, steps, a.cigar + static_cast<size_t>(p) * a.cigar_cap, a.cigar_cap);
}

template <int MODE>
int launch_forward(const TraceArgs &t, dim3 grid, size_t lds, hipStream_t stream, int64_t first)
{
    hipLaunchKernelGGL((trace_pairs_forward_kernel<MODE>), grid, dim3(kLanes), lds, stream, t, first);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

// One chunk: the forward kernel of the mode, then the traceback.
int launch_trace(const TraceArgs &t, dim3 grid, int64_t first, hipStream_t stream)
{
    const size_t lds = trace_lds_bytes(t.p.read_len);
    const int rc = t.mode == kGlobal      ? launch_forward<kGlobal>(t, grid, lds, stream, first)
                   : t.mode == kFreeQuery ? launch_forward<kFreeQuery>(t, grid, lds, stream, first)
                                          : launch_forward<kFreeSubject>(t, grid, lds, stream, first);
    if (rc) return rc;
    hipLaunchKernelGGL(trace_pairs_traceback_kernel, grid, dim3(kLanes), 0, stream, t, first);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

// A DP row beyond 64 KiB of LDS (subjects from 512 bp) needs the kernel's dynamic-LDS limit raised.  Done here, ahead of
// the row of launches and once per (device, mode): after a first call of that width a captured call only launches kernels.
int allow_wide_rows(int mode, size_t lds)
{
    if (lds <= kLdsOptIn) return BGSA_HIP_OK;
    static std::mutex mu;
    static size_t allowed[64][3] = {};
    int dev = 0;
    BGSA_HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    const bool cached = dev >= 0 && dev < 64;
    if (cached && allowed[dev][mode] >= lds) return BGSA_HIP_OK;
    const void *fn = mode == kGlobal      ? reinterpret_cast<const void *>(trace_pairs_forward_kernel<kGlobal>)
                     : mode == kFreeQuery ? reinterpret_cast<const void *>(trace_pairs_forward_kernel<kFreeQuery>)
                                          : reinterpret_cast<const void *>(trace_pairs_forward_kernel<kFreeSubject>);
    const size_t widest = trace_lds_bytes(kMaxWords * 32);
    BGSA_HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(widest)));
    if (cached) allowed[dev][mode] = widest;
    return BGSA_HIP_OK;
}

constexpr const char *kWho = "trace_pairs_dev";

}  // namespace

}  // namespace bgsa

using namespace bgsa;

extern "C" {

int bgsa_hip_trace_pairs_dev(const bgsa_hip_params_t *params, const char *d_content, const hip_read_t *d_peq, int ref_len, int read_len,
                             int64_t read_count, int word_num, const int32_t *d_pair_query, const int64_t *d_pair_subject,
                             int64_t n_pairs, int n_queries, int64_t subject_base, int32_t *d_score, int32_t *d_span, int32_t *d_n_ops,
                             uint32_t *d_cigar, int cigar_cap, void *d_workspace, size_t workspace_bytes, void *stream)
{
    return bgsa_hip_trace_pairs_lens_dev(params, d_content, d_peq, nullptr, ref_len, read_len, read_count, word_num, d_pair_query,
                                         d_pair_subject, n_pairs, n_queries, subject_base, d_score, d_span, d_n_ops, d_cigar, cigar_cap,
                                         d_workspace, workspace_bytes, stream);
}

// The entry shared by the three calls.  semi_lens: the caller is bgsa_hip_myers_place_trace_pairs_lens_dev, whose semi-global
// pairs carry lengths of their own (the forward kernel takes pair_read_len whatever the mode).
static int trace_pairs_entry(const bgsa_hip_params_t *params, const char *d_content, const hip_read_t *d_peq,
                             const int32_t *d_read_lens, int ref_len, int read_len, int64_t read_count, int word_num,
                             const int32_t *d_pair_query, const int64_t *d_pair_subject, int64_t n_pairs, int n_queries,
                             int64_t subject_base, int32_t *d_score, int32_t *d_span, int32_t *d_n_ops, uint32_t *d_cigar,
                             int cigar_cap, void *d_workspace, size_t workspace_bytes, void *stream, bool semi_lens);

int bgsa_hip_trace_pairs_lens_dev(const bgsa_hip_params_t *params, const char *d_content, const hip_read_t *d_peq,
                                  const int32_t *d_read_lens, int ref_len, int read_len, int64_t read_count, int word_num,
                                  const int32_t *d_pair_query, const int64_t *d_pair_subject, int64_t n_pairs, int n_queries,
                                  int64_t subject_base, int32_t *d_score, int32_t *d_span, int32_t *d_n_ops, uint32_t *d_cigar,
                                  int cigar_cap, void *d_workspace, size_t workspace_bytes, void *stream)
{
    return trace_pairs_entry(params, d_content, d_peq, d_read_lens, ref_len, read_len, read_count, word_num, d_pair_query, d_pair_subject,
                             n_pairs, n_queries, subject_base, d_score, d_span, d_n_ops, d_cigar, cigar_cap, d_workspace, workspace_bytes,
                             stream, false);
}

int bgsa_hip_myers_place_trace_pairs_lens_dev(const char *d_content, const hip_read_t *d_peq, const int32_t *d_read_lens, int ref_len,
                                              int read_len, int64_t read_count, int word_num, const int32_t *d_pair_query,
                                              const int64_t *d_pair_subject, int64_t n_pairs, int n_queries, int64_t subject_base,
                                              int32_t *d_score, int32_t *d_span, int32_t *d_n_ops, uint32_t *d_cigar, int cigar_cap,
                                              void *d_workspace, size_t workspace_bytes, void *stream)
{
    const bgsa_hip_params_t params = {BGSA_ALGO_MYERS, BGSA_ALIGN_SEMIGLOBAL, 0, -1, -1, 0};
    if (!d_read_lens)
        return refuse(kWho, BGSA_HIP_EINVAL, "d_read_lens is NULL (bgsa_hip_myers_place_trace_pairs_lens_dev takes the bucket's lengths; "
                                       "equal lengths: bgsa_hip_trace_pairs_dev)");
    return trace_pairs_entry(&params, d_content, d_peq, d_read_lens, ref_len, read_len, read_count, word_num, d_pair_query, d_pair_subject,
                             n_pairs, n_queries, subject_base, d_score, d_span, d_n_ops, d_cigar, cigar_cap, d_workspace, workspace_bytes,
                             stream, true);
}

static int trace_pairs_entry(const bgsa_hip_params_t *params, const char *d_content, const hip_read_t *d_peq,
                             const int32_t *d_read_lens, int ref_len, int read_len, int64_t read_count, int word_num,
                             const int32_t *d_pair_query, const int64_t *d_pair_subject, int64_t n_pairs, int n_queries,
                             int64_t subject_base, int32_t *d_score, int32_t *d_span, int32_t *d_n_ops, uint32_t *d_cigar,
                             int cigar_cap, void *d_workspace, size_t workspace_bytes, void *stream, bool semi_lens)
{
    if (int rc = check_pair_call(kWho, !params || !d_content || !d_peq || !d_pair_query || !d_pair_subject || !d_score || !d_span || !d_n_ops || !d_cigar,
                                 "a NULL pointer (only the workspace and the stream may be NULL)", n_pairs, ref_len, read_len, n_queries, cigar_cap,
                                 read_count))
        return rc;
    if (params->algo == BGSA_ALGO_BANDED)
        return refuse(kWho, BGSA_HIP_EUNSUPPORTED, "the banded filter's pairs are not traced back (it reports a thresholded distance, not an alignment)");
    if (params->algo != BGSA_ALGO_MYERS && params->algo != BGSA_ALGO_BITPAL) return refuse(kWho, BGSA_HIP_EINVAL, "unknown algorithm");
    if (params->alignment != BGSA_ALIGN_GLOBAL && params->alignment != BGSA_ALIGN_SEMIGLOBAL)
        return refuse(kWho, BGSA_HIP_EINVAL, "alignment is neither global nor semi-global");
    if (params->algo == BGSA_ALGO_MYERS && params->match == 0 && params->mismatch == 1 && params->gap == 1)
        return refuse(kWho, BGSA_HIP_EUNSUPPORTED, "Myers +distance (0, 1, 1) aligns the same as -distance: use the (0, -1, -1) aligner");
    if (params->gap >= 0 || params->match <= params->mismatch)
        return refuse(kWho, BGSA_HIP_EINVAL, "scores need gap < 0 and match > mismatch");
    if (word_num != bgsa_hip_word_num(params->algo, ref_len, read_len, params->k))
        return refuse(kWho, BGSA_HIP_EINVAL, "word_num is not bgsa_hip_word_num(params->algo, ...)");
    if (word_num > kMaxWords) return refuse(kWho, BGSA_HIP_EUNSUPPORTED, "subjects beyond 1,024 bp (word_num > 32) are not covered");
    if (d_read_lens && params->alignment != BGSA_ALIGN_GLOBAL && !semi_lens)
        return refuse(kWho, BGSA_HIP_EUNSUPPORTED, "per-subject lengths are traced in global mode only (semi-global buckets take subjects of one length)");
    // Myers scores -distance whatever the three ints hold (as the scoring calls: make_plan)
    const bool myers = params->algo == BGSA_ALGO_MYERS;
    const int match = myers ? 0 : params->match, mismatch = myers ? -1 : params->mismatch, gap = myers ? -1 : params->gap;
    const long long widest = std::max(std::llabs(static_cast<long long>(match)),
                                      std::max(std::llabs(static_cast<long long>(mismatch)), std::llabs(static_cast<long long>(gap))));
    if (widest * (static_cast<long long>(ref_len) + read_len) > 32767) {
        char why[200];
        snprintf(why, sizeof why, "max(|match|, |mismatch|, |gap|) * (ref_len + read_len) = %lld exceeds 32767: the DP row is kept in 16 bits",
                 widest * (static_cast<long long>(ref_len) + read_len));
        return refuse(kWho, BGSA_HIP_EUNSUPPORTED, why);
    }
    const size_t per = pair_wave_bytes(ref_len, read_len);
    if (d_workspace && workspace_bytes < per) return refuse(kWho, BGSA_HIP_EINVAL, "workspace smaller than bgsa_hip_align_pairs_min_workspace_bytes()");
    if (n_pairs == 0) return BGSA_HIP_OK;

    TraceArgs args{};
    args.p = PairArgs{d_content, d_peq, ref_len, read_len, read_count, word_num, d_pair_query, d_pair_subject, n_pairs, n_queries,
                      subject_base, d_score, d_n_ops, d_cigar, cigar_cap, nullptr, per, pair_hist_bytes(ref_len, read_len), device_fault_word(), d_read_lens};
    if (!args.p.fault_word) return BGSA_HIP_EHIP;
    args.span = d_span;
    args.match = match;
    args.mismatch = mismatch;
    args.gap = gap;
    args.mode = params->alignment == BGSA_ALIGN_GLOBAL ? kGlobal : (myers ? kFreeQuery : kFreeSubject);
    if (int rc = allow_wide_rows(args.mode, trace_lds_bytes(read_len))) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return run_pair_chunks(d_workspace, workspace_bytes, per, n_pairs, s, [&](unsigned char *workspace, dim3 grid, int64_t first) {
        args.p.workspace = workspace;
        return launch_trace(args, grid, first, s);
    });
}

}  // extern "C"
