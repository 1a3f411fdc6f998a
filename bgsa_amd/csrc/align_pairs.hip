// align_pairs.hip — edit scripts (CIGAR) for a list of (query, subject) pairs, traced back on the GPU
// (include/bgsa_hip.h "alignment of selected pairs").
//
// Myers unit-cost GLOBAL alignment, subjects of up to 32 words.  The row kernels score one query against 64 subjects
// per wave with a wave-uniform query character; here a lane owns one PAIR, so every lane has its own query character
// and its own subject, and the threaded-code row loops do not apply.  Two kernels per chunk of pairs:
//
//   forward    the 8-operation Myers row in compiler-scheduled C++, the subject's five Peq planes held in
//              VGPRs and selected per lane by the lane's query class.  After every row the lane stores, per word, the
//              two bit vectors the traceback needs (below) and at the end the distance.
//   traceback  walks back from (m, n), one history bit pair per step, writes one op byte per step backwards into the
//              pair's scratch and then run-length encodes forwards into the cigar row.
//
// History.  With D0 = [D[i][j] == D[i-1][j-1]], Eq = [q_i matches s_j] and Hp = [D[i][j] - D[i-1][j] == +1] of the row
// recurrence, the canonical step at a cell (i, j > 0) is: diagonal iff Eq | ~D0 (a mismatch is taken exactly when the
// diagonal delta is 1), else up iff Hp, else left.  Four outcomes are two bits, so a row keeps two vectors per word:
//     A = Eq | ~D0           the step is diagonal
//     B = Eq | (D0 & Hp)     diagonal: '=' (1) or 'X' (0); otherwise: up 'I' (1) or left 'D' (0)
// 8 * word_num bytes per row and pair, laid out [chunk wave][row][vector][word][lane] uint32: every wave store is one
// coalesced 256-byte row, and a traceback step is two loads and two bit tests.
#include "pair_trace.h"   // the argument block, owned_pair, the Myers word and the class masks, the history, the chunk loop

namespace bgsa {

namespace {

// one instantiation per word count: the row loop is straight-line code over exactly the subject's words
using PairWidths = Widths<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32>;

template <int NW>
__global__ __launch_bounds__(kLanes) void align_pairs_forward_kernel(PairArgs a, int64_t first)
{
    const int lane = threadIdx.x;
    const int64_t p = first + static_cast<int64_t>(blockIdx.x) * kLanes + lane;
    int q = 0;
    int64_t col = 0;
    if (!owned_pair(a, p, true, &q, &col)) return;
    constexpr int wn = NW;   // == a.word_num: the launcher dispatches on it
    const int m = a.ref_len;

    // the subject's Peq planes: [group][class][word][lane]
    const uint32_t *g = a.peq + static_cast<size_t>(col >> 6) * kChars * wn * kLanes + (col & (kLanes - 1));
    uint32_t peq[kChars][NW], pv[NW], mv[NW];
#pragma unroll
    for (int w = 0; w < NW; w++) {
#pragma unroll
        for (int c = 0; c < kChars; c++) peq[c][w] = g[(static_cast<size_t>(c) * wn + w) * kLanes];
        pv[w] = ~0u;
        mv[w] = 0u;
    }

    const unsigned char *row = reinterpret_cast<const unsigned char *>(a.content) + static_cast<size_t>(q) * (m + 1);
    uint32_t *h = reinterpret_cast<uint32_t *>(a.workspace + static_cast<size_t>(blockIdx.x) * a.wave_bytes) + lane;
    const size_t row_words = static_cast<size_t>(2) * wn * kLanes;
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
            const uint32_t c = (codes >> (4 * r)) & 15u;
            const ClassMasks k = class_masks<false>(c);
            uint32_t carry = 0, hp_in = 1, hn_in = 0;
#pragma unroll
            for (int w = 0; w < NW; w++) {
                const uint32_t e = class_eq(peq, w, k);
                const MyersWord s = myers_word(e, pv[w], mv[w], carry, hp_in, hn_in);
                h[static_cast<size_t>(w) * kLanes] = e | ~s.d0;
                h[static_cast<size_t>(wn + w) * kLanes] = e | (s.d0 & s.hp);
            }
            h += row_words;
        }
    }

    int score = m;
    const int n = pair_read_len(a, col);   // the columns behind the subject's own end never enter: column j depends on columns <= j
#pragma unroll
    for (int w = 0; w < NW; w++) {
        const int rem = n - 32 * w;
        const uint32_t mask = rem >= 32 ? ~0u : (rem <= 0 ? 0u : ((1u << rem) - 1u));
        score += __popc(pv[w] & mask) - __popc(mv[w] & mask);
    }
    a.distance[p] = score;
}

__global__ __launch_bounds__(kLanes) void align_pairs_traceback_kernel(PairArgs a, int64_t first)
{
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

    int i = a.ref_len, j = pair_read_len(a, col);
    size_t steps = 0;
    while (i > 0 || j > 0) {
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

    a.n_ops[p] = encode_runs(ops, steps, a.cigar + static_cast<size_t>(p) * a.cigar_cap, a.cigar_cap);
}

// One chunk: the forward kernel of the subject's width, then the traceback.
int launch_pairs(const PairArgs &a, dim3 grid, int64_t first, hipStream_t stream)
{
    const int rc = PairWidths::dispatch(a.word_num, "myers_align_pairs", [&](auto width) {
        hipLaunchKernelGGL((align_pairs_forward_kernel<decltype(width)::value>), grid, dim3(kLanes), 0, stream, a, first);
        BGSA_HIP_TRY(hipGetLastError());
        return BGSA_HIP_OK;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(align_pairs_traceback_kernel, grid, dim3(kLanes), 0, stream, a, first);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

}  // namespace

}  // namespace bgsa

using namespace bgsa;

extern "C" {

size_t bgsa_hip_align_pairs_min_workspace_bytes(int ref_len, int read_len)
{
    if (ref_len <= 0 || read_len <= 0) return 0;
    return pair_wave_bytes(ref_len, read_len);
}

size_t bgsa_hip_align_pairs_workspace_bytes(int ref_len, int read_len, int64_t n_pairs)
{
    if (ref_len <= 0 || read_len <= 0 || n_pairs < 0) return 0;
    return pair_workspace_for(pair_wave_bytes(ref_len, read_len), n_pairs);
}

int bgsa_hip_myers_align_pairs_dev(const char *d_content, const hip_read_t *d_peq, int ref_len, int read_len, int64_t read_count,
                                   int word_num, const int32_t *d_pair_query, const int64_t *d_pair_subject, int64_t n_pairs,
                                   int n_queries, int64_t subject_base, int32_t *d_distance, int32_t *d_n_ops, uint32_t *d_cigar,
                                   int cigar_cap, void *d_workspace, size_t workspace_bytes, void *stream)
{
    return bgsa_hip_myers_align_pairs_lens_dev(d_content, d_peq, nullptr, ref_len, read_len, read_count, word_num, d_pair_query,
                                               d_pair_subject, n_pairs, n_queries, subject_base, d_distance, d_n_ops, d_cigar, cigar_cap,
                                               d_workspace, workspace_bytes, stream);
}

int bgsa_hip_myers_align_pairs_lens_dev(const char *d_content, const hip_read_t *d_peq, const int32_t *d_read_lens, int ref_len,
                                        int read_len, int64_t read_count, int word_num, const int32_t *d_pair_query,
                                        const int64_t *d_pair_subject, int64_t n_pairs, int n_queries, int64_t subject_base,
                                        int32_t *d_distance, int32_t *d_n_ops, uint32_t *d_cigar, int cigar_cap, void *d_workspace,
                                        size_t workspace_bytes, void *stream)
{
    const char *who = "myers_align_pairs_dev";
    if (int rc = check_pair_call(who, !d_content || !d_peq || !d_pair_query || !d_pair_subject || !d_distance || !d_n_ops || !d_cigar,
                                 "a NULL pointer (only the workspace may be NULL)", n_pairs, ref_len, read_len, n_queries, cigar_cap, read_count))
        return rc;
    if (word_num != bgsa_hip_word_num(BGSA_ALGO_MYERS, ref_len, read_len, 0))
        return refuse(who, BGSA_HIP_EINVAL, "word_num is not bgsa_hip_word_num(BGSA_ALGO_MYERS, ...)");
    if (word_num > kMaxWords) return refuse(who, BGSA_HIP_EUNSUPPORTED, "subjects beyond 1,024 bp (word_num > 32) are not covered");
    const size_t per = pair_wave_bytes(ref_len, read_len);
    if (d_workspace && workspace_bytes < per) return refuse(who, BGSA_HIP_EINVAL, "workspace smaller than bgsa_hip_align_pairs_min_workspace_bytes()");
    if (n_pairs == 0) return BGSA_HIP_OK;

    PairArgs args{d_content, d_peq, ref_len, read_len, read_count, word_num, d_pair_query, d_pair_subject, n_pairs, n_queries,
                  subject_base, d_distance, d_n_ops, d_cigar, cigar_cap, nullptr, per, pair_hist_bytes(ref_len, read_len), device_fault_word(), d_read_lens};
    if (!args.fault_word) return BGSA_HIP_EHIP;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return run_pair_chunks(d_workspace, workspace_bytes, per, n_pairs, s, [&](unsigned char *workspace, dim3 grid, int64_t first) {
        args.workspace = workspace;
        return launch_pairs(args, grid, first, s);
    });
}

}  // extern "C"
