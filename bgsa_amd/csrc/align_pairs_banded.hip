// align_pairs_banded.hip — edit scripts (CIGAR) of selected pairs for subjects of ANY length, the history limited to the
// diagonal band of a caller-given max_distance (include/bgsa_hip.h "band-limited history").
//
// align_pairs.hip keeps the whole subject's Peq planes and state in VGPRs (32 words) and a history of m x 2 x word_num x 256 B
// per wave.  A pair whose distance is <= B = max_distance has all its optimal paths inside the band |d| + |d - (n - m)| <= B,
// d = j - i (myers_band.h), so here a block of 32 rows runs on the words that hold the band's columns only — its WINDOW — and
// only those words get history.  Everything that is wider than the window lives in the wave's workspace slice.
//
// THE RULE (tests/banded_align_reference.py restates it on Python integers).  delta = n - m, dlo = -((B - delta) / 2),
// dhi = (delta + B) / 2 as in band_schedule.  The block of 0-based rows i0 .. last - 1, i0 % 32 == 0, last = min(i0 + 32, m),
// has the window of words [a, b], a = (max(1, i0 + 1 + dlo) - 1) / 32, b = (min(n, last + dhi) - 1) / 32.  Every row of the
// block is the 8-operation Myers row on exactly these words: the lowest window word takes the row-edge carry-ins
// (hp_in = 1, hn_in = 0, add-carry 0) whether or not a == 0, words left of the window keep their last deltas, words right of
// it their initial state (pv = ~0, mv = 0).  Every column so holds the cost of a real path: D' = m + sum over ALL words of
// popc(pv & mask) - popc(mv & mask) >= D, and D' <= B certifies D' = D.  A certified pair is traced back from (m, n) through
// the two history vectors of align_pairs.hip (A = Eq | ~D0, B = Eq | (D0 & Hp)) with the same preference, so the script is
// that call's; any other pair is beyond the bound.  The windows depend on (m, n, B) only: they are wave-uniform.
// The row's word is myers_word of bgsa_common.h; the class masks and the score of the stored state are class_masks and
// state_score of pair_trace.h.
//
// One wave's slice: [history][state][op bytes].
//   history  [row][vector A|B][window word][lane] uint32, the word stride band_words = the widest block window of the shape;
//            the traceback finds a cell from (i, j) and its block's a by arithmetic
//   state    [vector pv|mv][word][lane] uint32, all word_num words, initialised once per wave
//   op bytes [step][lane], as in align_pairs.hip
#include "pair_trace.h"

namespace bgsa {

namespace {

constexpr int kBandRows = 32;            // rows of a block: one window, one load of the query's characters
constexpr int kBandTraceMaxWords = 32;   // widest window with a kernel: 5 Peq planes + pv + mv of 32 words stay in registers

// one instantiation per window width: the rows are straight-line code over at most WB words
using BandWidths = Widths<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32>;

struct BandArgs {
    PairArgs p;                  // hist_bytes: the history at the slice's head
    int max_distance;            // B, at most ref_len + read_len (a larger bound certifies nothing more)
    int dlo, dhi;                // the band's diagonals
    int band_words;              // the history's word stride
    size_t state_off, ops_off;   // the state and the op bytes inside a slice
};

// The window [*a, *b] of the block of rows i0 .. min(i0 + 32, m) - 1.  a <= b <= word_num - 1 whenever |n - m| <= B.
__host__ __device__ inline void block_window(int m, int n, int dlo, int dhi, int i0, int *a, int *b)
{
    const int last = m - i0 < kBandRows ? m : i0 + kBandRows;
    const int jlo = i0 + 1 + dlo < 1 ? 1 : i0 + 1 + dlo;
    const int jhi = last + dhi > n ? n : last + dhi;
    *a = (jlo - 1) >> 5;
    *b = (jhi - 1) >> 5;
}

// B as the windows use it, or -1 when the shape has no band.
inline int effective_bound(int m, int n, int max_distance)
{
    if (m <= 0 || n <= 0 || max_distance < 0) return -1;
    const long long delta = static_cast<long long>(n) - m, sum = static_cast<long long>(m) + n;
    if ((delta < 0 ? -delta : delta) > max_distance) return -1;
    return max_distance < sum ? max_distance : static_cast<int>(sum < 0x7fffffff ? sum : 0x7fffffff);
}

inline void band_diagonals(int m, int n, int bound, int *dlo, int *dhi)
{
    const int delta = n - m;
    *dlo = -((bound - delta) / 2);
    *dhi = static_cast<int>((static_cast<long long>(delta) + bound) / 2);
}

int band_words_of(int m, int n, int max_distance)
{
    const int bound = effective_bound(m, n, max_distance);
    if (bound < 0 || static_cast<long long>(m) + n > 0x7fffffff) return 0;
    int dlo = 0, dhi = 0, widest = 0;
    band_diagonals(m, n, bound, &dlo, &dhi);
    const int wn = (n + 31) / 32;
    for (int i0 = 0; i0 < m && widest < wn; i0 += kBandRows) {
        int a = 0, b = 0;
        block_window(m, n, dlo, dhi, i0, &a, &b);
        if (b - a + 1 > widest) widest = b - a + 1;
        if (m - i0 <= kBandRows) break;
    }
    return widest;
}

size_t banded_hist_bytes(int m, int band_words) { return static_cast<size_t>(m) * 2 * band_words * kLanes * sizeof(uint32_t); }
size_t banded_state_bytes(int n) { return static_cast<size_t>(2) * ((n + 31) / 32) * kLanes * sizeof(uint32_t); }
size_t banded_wave_bytes(int m, int n, int band_words)
{
    const size_t ops = (static_cast<size_t>(m) + static_cast<size_t>(n)) * kLanes;
    return (banded_hist_bytes(m, band_words) + banded_state_bytes(n) + ops + 255) & ~static_cast<size_t>(255);
}

template <int WB>
__global__ __launch_bounds__(kLanes) void align_pairs_banded_forward_kernel(BandArgs g, int64_t first)
{
    const PairArgs &a = g.p;
    const int lane = threadIdx.x;
    const int64_t p = first + static_cast<int64_t>(blockIdx.x) * kLanes + lane;
    int q = 0;
    int64_t col = 0;
    if (!owned_pair(a, p, true, &q, &col)) return;
    const int wn = a.word_num, m = a.ref_len, n = a.read_len;

    // the subject's Peq planes: [group][class][word][lane], whatever word_num is
    const uint32_t *planes = a.peq + static_cast<size_t>(col >> 6) * kChars * wn * kLanes + (col & (kLanes - 1));
    unsigned char *slice = a.workspace + static_cast<size_t>(blockIdx.x) * a.wave_bytes;
    uint32_t *h = reinterpret_cast<uint32_t *>(slice) + lane;
    uint32_t *state = reinterpret_cast<uint32_t *>(slice + g.state_off) + lane;   // [pv | mv][word][lane]
    state_init(state, wn);

    const unsigned char *row = reinterpret_cast<const unsigned char *>(a.content) + static_cast<size_t>(q) * (m + 1);
    const size_t row_words = static_cast<size_t>(2) * g.band_words * kLanes;
    for (int i0 = 0; i0 < m; i0 += kBandRows) {
        int wa = 0, wlast = 0;
        block_window(m, n, g.dlo, g.dhi, i0, &wa, &wlast);
        const int wb = wlast - wa + 1;   // wave-uniform, 1 .. WB (the launcher dispatches on the widest one)

        // every load of the block at its head: a load waits for every older store of the wave
        uint32_t peq[kChars][WB], pv[WB], mv[WB];
#pragma unroll
        for (int w = 0; w < WB; w++) {
            if (w < wb) {
#pragma unroll
                for (int c = 0; c < kChars; c++) peq[c][w] = planes[(static_cast<size_t>(c) * wn + wa + w) * kLanes];
                pv[w] = state[static_cast<size_t>(wa + w) * kLanes];
                mv[w] = state[static_cast<size_t>(wn + wa + w) * kLanes];
            } else {
#pragma unroll
                for (int c = 0; c < kChars; c++) peq[c][w] = 0u;
                pv[w] = mv[w] = 0u;
            }
        }
        const int rows = m - i0 < kBandRows ? m - i0 : kBandRows;
        unsigned long long lo = 0, hi = 0;   // the block's characters, four bits each
#pragma unroll
        for (int r = 0; r < kBandRows; r++) {
            unsigned long long c = r < rows ? row[i0 + r] : 0u;
            if (c > 4) c = 0;   // as the packed streams: out-of-alphabet bytes behave as 'A'
            if (r < 16) lo |= c << (4 * r);
            else hi |= c << (4 * (r - 16));
        }

#pragma unroll 1
        for (int r = 0; r < rows; r++) {
            const ClassMasks k = class_masks<false>(next_class(lo, hi));
            uint32_t carry = 0, hp_in = 1, hn_in = 0;
#pragma unroll
            for (int w = 0; w < WB; w++) {
                if (w < wb) {   // a window narrower than WB runs its own words only
                    const uint32_t e = class_eq(peq, w, k);
                    const MyersWord s = myers_word(e, pv[w], mv[w], carry, hp_in, hn_in);
                    h[static_cast<size_t>(w) * kLanes] = e | ~s.d0;
                    h[static_cast<size_t>(g.band_words + w) * kLanes] = e | (s.d0 & s.hp);
                }
            }
            h += row_words;
        }

#pragma unroll
        for (int w = 0; w < WB; w++) {
            if (w < wb) {
                state[static_cast<size_t>(wa + w) * kLanes] = pv[w];
                state[static_cast<size_t>(wn + wa + w) * kLanes] = mv[w];
            }
        }
    }

    const int score = state_score(state, wn, n, m);
    const bool certified = score <= g.max_distance;
    a.distance[p] = certified ? score : BGSA_HIP_DISTANCE_BEYOND;
    if (!certified) a.n_ops[p] = 0;
}

__global__ __launch_bounds__(kLanes) void align_pairs_banded_traceback_kernel(BandArgs g, int64_t first)
{
    const PairArgs &a = g.p;
    const int lane = threadIdx.x;
    const int64_t p = first + static_cast<int64_t>(blockIdx.x) * kLanes + lane;
    int q = 0;
    int64_t col = 0;
    if (!owned_pair(a, p, false, &q, &col)) return;
    if (a.distance[p] < 0) return;   // beyond the bound: the forward kernel has said so
    unsigned char *slice = a.workspace + static_cast<size_t>(blockIdx.x) * a.wave_bytes;
    const uint32_t *hist = reinterpret_cast<const uint32_t *>(slice) + lane;
    unsigned char *ops = slice + g.ops_off + lane;   // [step][lane]
    const size_t row_words = static_cast<size_t>(2) * g.band_words * kLanes;

    int i = a.ref_len, j = a.read_len;
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
            int wa = 0, wlast = 0;
            block_window(a.ref_len, a.read_len, g.dlo, g.dhi, (i - 1) & ~(kBandRows - 1), &wa, &wlast);
            const int w = (j - 1) >> 5;
            if (w < wa || w > wlast) {   // cannot happen for a certified pair; a bug must not become an out-of-bounds load
                atomicOr(a.fault_word, static_cast<unsigned>(BGSA_HIP_FAULT_BAND));
                a.n_ops[p] = 0;
                return;
            }
            int jj = j - 32 * wa;   // the column inside the block's window
            op = history_step(hist, row_words, g.band_words, &i, &jj);
            j = jj + 32 * wa;
        }
        ops[steps * kLanes] = static_cast<unsigned char>(op);
        steps++;
    }

    a.n_ops[p] = encode_runs(ops, steps, a.cigar + static_cast<size_t>(p) * a.cigar_cap, a.cigar_cap);
}

// |n - m| > max_distance: every owned pair is beyond the bound, and no row has to run to know it.
__global__ __launch_bounds__(kLanes) void align_pairs_banded_beyond_kernel(PairArgs a, int64_t first)
{
    const int64_t p = first + static_cast<int64_t>(blockIdx.x) * kLanes + threadIdx.x;
    int q = 0;
    int64_t col = 0;
    if (!owned_pair(a, p, true, &q, &col)) return;
    a.distance[p] = BGSA_HIP_DISTANCE_BEYOND;
    a.n_ops[p] = 0;
}

// One chunk: no band at all, or the forward kernel of the widest window, then the traceback.
int launch_banded(const BandArgs &g, dim3 grid, int64_t first, hipStream_t stream)
{
    if (g.band_words == 0) {
        hipLaunchKernelGGL(align_pairs_banded_beyond_kernel, grid, dim3(kLanes), 0, stream, g.p, first);
        BGSA_HIP_TRY(hipGetLastError());
        return BGSA_HIP_OK;
    }
    const int rc = BandWidths::dispatch(g.band_words, "myers_align_pairs_banded", [&](auto width) {
        hipLaunchKernelGGL((align_pairs_banded_forward_kernel<decltype(width)::value>), grid, dim3(kLanes), 0, stream, g, first);
        BGSA_HIP_TRY(hipGetLastError());
        return BGSA_HIP_OK;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(align_pairs_banded_traceback_kernel, grid, dim3(kLanes), 0, stream, g, first);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

// The largest max_distance whose windows the kernels hold for this shape (band_words is monotone in it), or -1.
int largest_bound(int m, int n)
{
    const long long delta = static_cast<long long>(n) - m;
    int lo = static_cast<int>(delta < 0 ? -delta : delta), hi = effective_bound(m, n, 0x7fffffff);
    if (band_words_of(m, n, lo) > kBandTraceMaxWords) return -1;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (band_words_of(m, n, mid) <= kBandTraceMaxWords) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

}  // namespace

}  // namespace bgsa

using namespace bgsa;

extern "C" {

int bgsa_hip_align_pairs_band_words(int ref_len, int read_len, int max_distance)
{
    return band_words_of(ref_len, read_len, max_distance);
}

size_t bgsa_hip_align_pairs_banded_min_workspace_bytes(int ref_len, int read_len, int max_distance)
{
    if (ref_len <= 0 || read_len <= 0 || max_distance < 0) return 0;
    return banded_wave_bytes(ref_len, read_len, band_words_of(ref_len, read_len, max_distance));
}

size_t bgsa_hip_align_pairs_banded_workspace_bytes(int ref_len, int read_len, int max_distance, int64_t n_pairs)
{
    if (ref_len <= 0 || read_len <= 0 || max_distance < 0 || n_pairs < 0) return 0;
    return pair_workspace_for(banded_wave_bytes(ref_len, read_len, band_words_of(ref_len, read_len, max_distance)), n_pairs);
}

int bgsa_hip_myers_align_pairs_banded_dev(const char *d_content, const hip_read_t *d_peq, int ref_len, int read_len, int64_t read_count,
                                          int word_num, const int32_t *d_pair_query, const int64_t *d_pair_subject, int64_t n_pairs,
                                          int n_queries, int64_t subject_base, int max_distance, int32_t *d_distance, int32_t *d_n_ops,
                                          uint32_t *d_cigar, int cigar_cap, void *d_workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "myers_align_pairs_banded_dev";
    if (int rc = check_pair_call(who, !d_content || !d_peq || !d_pair_query || !d_pair_subject || !d_distance || !d_n_ops || !d_cigar,
                                 "a NULL pointer (only the workspace may be NULL)", n_pairs, ref_len, read_len, n_queries, cigar_cap, read_count))
        return rc;
    if (word_num != bgsa_hip_word_num(BGSA_ALGO_MYERS, ref_len, read_len, 0))
        return refuse(who, BGSA_HIP_EINVAL, "word_num is not bgsa_hip_word_num(BGSA_ALGO_MYERS, ...)");
    if (max_distance < 0) return refuse(who, BGSA_HIP_EINVAL, "max_distance is negative");
    if (static_cast<long long>(ref_len) + read_len > 0x7fffffff) return refuse(who, BGSA_HIP_EUNSUPPORTED, "ref_len + read_len beyond 2^31 - 1");
    const int band_words = band_words_of(ref_len, read_len, max_distance);
    if (band_words > kBandTraceMaxWords) {
        char why[200];
        const int most = largest_bound(ref_len, read_len);
        if (most >= 0)
            snprintf(why, sizeof why, "the band of max_distance %d is %d words wide, the kernels hold %d: %d x %d bp takes max_distance <= %d",
                     max_distance, band_words, kBandTraceMaxWords, ref_len, read_len, most);
        else
            snprintf(why, sizeof why, "the band of max_distance %d is %d words wide, the kernels hold %d: no bound fits %d x %d bp",
                     max_distance, band_words, kBandTraceMaxWords, ref_len, read_len);
        return refuse(who, BGSA_HIP_EUNSUPPORTED, why);
    }
    const size_t per = banded_wave_bytes(ref_len, read_len, band_words);
    if (d_workspace && workspace_bytes < per)
        return refuse(who, BGSA_HIP_EINVAL, "workspace smaller than bgsa_hip_align_pairs_banded_min_workspace_bytes()");
    if (n_pairs == 0) return BGSA_HIP_OK;

    BandArgs args{};
    const size_t hist = banded_hist_bytes(ref_len, band_words);
    args.p = PairArgs{d_content, d_peq, ref_len, read_len, read_count, word_num, d_pair_query, d_pair_subject, n_pairs, n_queries,
                      subject_base, d_distance, d_n_ops, d_cigar, cigar_cap, nullptr, per, hist, device_fault_word(), nullptr};
    if (!args.p.fault_word) return BGSA_HIP_EHIP;
    const int bound = effective_bound(ref_len, read_len, max_distance);
    args.max_distance = bound < 0 ? 0 : bound;
    if (band_words > 0) band_diagonals(ref_len, read_len, bound, &args.dlo, &args.dhi);
    args.band_words = band_words;
    args.state_off = hist;
    args.ops_off = hist + banded_state_bytes(read_len);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return run_pair_chunks(d_workspace, workspace_bytes, per, n_pairs, s, [&](unsigned char *workspace, dim3 grid, int64_t first) {
        args.p.workspace = workspace;
        return launch_banded(args, grid, first, s);
    });
}

}  // extern "C"
