// place_pairs_banded.hip — where a read lies inside its window and how it aligns, for reads of ANY length: Myers unit-cost
// SEMI-GLOBAL (the subject end to end inside the query), the history limited to the diagonal band of a caller-given
// max_distance (include/bgsa_hip.h "band-limited semi-global placement").
//
// trace_pairs.hip runs a scalar DP per lane over a 16-bit row in LDS and stops at 1,024 bp.  align_pairs_banded.hip showed how
// a distance bound turns the history of a long pair into a window of words per block of 32 rows; its band is fixed by (m, n).
// In semi-global mode the read's diagonal is not known before the row it ends at is, and that row differs from pair to pair.
// So a chunk of pairs runs THREE kernels, one pair per lane and one wave per workgroup each:
//
//   locate     the bit-parallel Myers semi-global row on ALL words of the subject (the row edge feeds hp_in = 0: the free
//              column 0), the query character per lane.  run = D[i][n] starts at n and moves by Hp - Hn at column n per row; the
//              smallest run is D*, the SMALLEST row that has it is e.  Exact whatever the bound.  Column blocks of
//              kLocateWords words with everything in registers; the three carries of a block's last word (Hp, Hn, the add's)
//              travel to the next column block as one bit per row in the slice's carry words, 32 rows to a word.
//   forward    for a pair with D* <= B = min(max_distance, n): every optimal path ends at (e, n) and costs <= B, so it lies on
//              the diagonals within B of that cell's.  In VIRTUAL rows i' = i - o, o = e - n - B per lane, the end cell is
//              (M', n), M' = n + B, for every lane: the block of 0-based virtual rows i0 .. last - 1, last = min(i0 + 32, M'),
//              has the WINDOW of words [a, b], a = (max(1, i0 + 1 - 2B) - 1) / 32, b = (min(n, last) - 1) / 32 — the diagonals
//              j - i' in [-2B, 0] — which depends on (n, B) only: wave-uniform, the schedule of align_pairs_banded.hip.  Every
//              row is the Myers row on exactly these words; the lowest window word takes hp_in = 0 when a == 0 and 1 otherwise;
//              words left of the window keep their last deltas, words right of it their initial state.  A virtual row whose
//              query row does not exist (i < 1: only when o < 0, only in blocks with a == 0 because -o <= 2B) runs with an
//              all-zero match mask and leaves the state at row 0's.  D' = (rows run with hp_in = 1) + sum over all words of
//              popc(pv & mask) - popc(mv & mask) is the cost of a real path to (e, n): D' >= D*, and for D* <= B it is D*.
//              D' != D* raises BGSA_HIP_FAULT_BAND: a bug, never an input.
//   traceback  the walk of trace_pairs.hip's Myers semi-global mode from (e, n) through the window words' history (A = Eq | ~D0,
//              B = Eq | (D0 & Hp)): diagonal, then up 'I', then left 'D'; it stops at the first cell with j = 0, whose row is
//              q_begin; on query row 0 what is left of the subject is 'D'.
//
// tests/place_reference.py restates all of it on Python integers.  The rows of locate and forward are written out here, not
// through myers_word (bgsa_common.h) and class_masks / state_score (pair_trace.h) as align_pairs_banded.hip's are: with the
// helpers these kernels grew by one to three instructions and two timed lines missed their rule (LABNOTES §31.5).
//
// One wave's slice: [history][state][carry][op bytes].
//   history  [virtual row][vector A|B][window word][lane] uint32, the word stride band_words = the widest window of (n, B)
//   state    [vector pv|mv][word][lane] uint32, all word_num words, then one word per lane: 1 = the forward kernel certified
//   carry    [block of 32 rows][Hp|Hn|add][lane] uint32: locate's carries between its column blocks
//   op bytes [step][lane]
#include "pair_trace.h"

namespace bgsa {

namespace {

constexpr int kPlaceRows = 32;            // virtual rows of a block: one window, one load of the query's characters
constexpr int kPlaceMaxWords = 32;        // widest window with a kernel
constexpr int kLocateWords = 16;          // words of a locate column block: 5 Peq planes + pv + mv in 112 registers

using PlaceWidths = Widths<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32>;

struct PlaceArgs {
    PairArgs p;                  // hist_bytes: the history at the slice's head
    int32_t *span;               // [pair][q_begin, q_end = e, 0, n]
    int bound;                   // B = min(max_distance, n)
    int band_words;              // the history's word stride
    size_t state_off, carry_off, ops_off;
};

// B as the windows use it: D* <= n always, so a larger bound changes nothing.
__host__ __device__ inline int place_bound(int n, int max_distance) { return max_distance < n ? max_distance : n; }

// The window [*a, *b] of the block of virtual rows i0 .. min(i0 + 32, n + B) - 1.  0 <= a <= b <= word_num - 1.
__host__ __device__ inline void place_window(int n, int bound, int i0, int *a, int *b)
{
    const int rows = n + bound;
    const int last = rows - i0 < kPlaceRows ? rows : i0 + kPlaceRows;
    const int jlo = i0 + 1 - 2 * bound < 1 ? 1 : i0 + 1 - 2 * bound;
    const int jhi = last > n ? n : last;
    *a = (jlo - 1) >> 5;
    *b = (jhi - 1) >> 5;
}

// Whether the virtual rows and the op bytes of the shape count in int.
inline bool place_counts_fit(int m, int n, int max_distance)
{
    const long long bound = place_bound(n, max_distance);
    return static_cast<long long>(m) + n + bound <= 0x7fffffff && 2ll * n + bound <= 0x7fffffff;
}

int place_band_words_of(int n, int max_distance)
{
    if (n <= 0 || max_distance < 0 || !place_counts_fit(0, n, max_distance)) return 0;
    const int bound = place_bound(n, max_distance), rows = n + bound, wn = (n + 31) / 32;
    const int full = 1 + (bound + 15) / 16;   // a window that neither edge of the subject clips
    const int most = full < wn ? full : wn;
    int widest = 0;
    for (int i0 = 0; i0 < rows && widest < most; i0 += kPlaceRows) {
        int a = 0, b = 0;
        place_window(n, bound, i0, &a, &b);
        if (b - a + 1 > widest) widest = b - a + 1;
        if (rows - i0 <= kPlaceRows) break;
    }
    return widest;
}

size_t place_rows_of(int n, int max_distance) { return static_cast<size_t>(n) + static_cast<size_t>(place_bound(n, max_distance)); }
size_t place_hist_bytes(int n, int max_distance, int band_words)
{
    return place_rows_of(n, max_distance) * 2 * band_words * kLanes * sizeof(uint32_t);
}
size_t place_state_bytes(int n) { return (static_cast<size_t>(2) * ((n + 31) / 32) + 1) * kLanes * sizeof(uint32_t); }
size_t place_carry_bytes(int m) { return static_cast<size_t>((m + 31) / 32) * 3 * kLanes * sizeof(uint32_t); }
size_t place_wave_bytes(int m, int n, int max_distance, int band_words)
{
    // a walk consumes a query row or a subject column per step, and never more rows than the virtual ones
    const size_t rows = place_rows_of(n, max_distance);
    const size_t ops = (static_cast<size_t>(n) + (rows < static_cast<size_t>(m) ? rows : static_cast<size_t>(m))) * kLanes;
    return (place_hist_bytes(n, max_distance, band_words) + place_state_bytes(n) + place_carry_bytes(m) + ops + 255) & ~static_cast<size_t>(255);
}

// The block's characters, four bits each, rows i0 .. i0 + 31 of `row` (0-based; may be negative or beyond m - 1: code 15, a
// row that matches nothing).  Out-of-alphabet bytes behave as 'A', as in the packed streams.
__device__ __forceinline__ void block_classes(const unsigned char *row, int m, int i0, int rows, unsigned long long *lo, unsigned long long *hi)
{
    unsigned long long l = 0, h = 0;
#pragma unroll
    for (int r = 0; r < kPlaceRows; r++) {
        const int i = i0 + r;
        unsigned long long c = 15u;
        if (r < rows && i >= 0 && i < m) {
            c = row[i];
            if (c > 4) c = 0;
        }
        if (r < 16) l |= c << (4 * r);
        else h |= c << (4 * (r - 16));
    }
    *lo = l;
    *hi = h;
}

__global__ __launch_bounds__(kLanes) void place_pairs_locate_kernel(PlaceArgs g, int64_t first)
{
    constexpr int W = kLocateWords;
    const PairArgs &a = g.p;
    const int lane = threadIdx.x;
    const int64_t p = first + static_cast<int64_t>(blockIdx.x) * kLanes + lane;
    int q = 0;
    int64_t col = 0;
    if (!owned_pair(a, p, true, &q, &col)) return;
    const int wn = a.word_num, m = a.ref_len, n = a.read_len;

    const uint32_t *planes = a.peq + static_cast<size_t>(col >> 6) * kChars * wn * kLanes + (col & (kLanes - 1));
    unsigned char *slice = a.workspace + static_cast<size_t>(blockIdx.x) * a.wave_bytes;
    uint32_t *carries = reinterpret_cast<uint32_t *>(slice + g.carry_off) + lane;   // [row block][Hp | Hn | add][lane]
    const unsigned char *row = reinterpret_cast<const unsigned char *>(a.content) + static_cast<size_t>(q) * (m + 1);
    const int top = (n - 1) & 31;   // column n inside the last word

    int run = n, best = n, e = 0;
    for (int w0 = 0; w0 < wn; w0 += W) {
        const int wb = wn - w0 < W ? wn - w0 : W;   // wave-uniform
        const bool leftmost = w0 == 0, rightmost = w0 + W >= wn;
        uint32_t peq[kChars][W], pv[W], mv[W];
#pragma unroll
        for (int w = 0; w < W; w++) {
#pragma unroll
            for (int c = 0; c < kChars; c++) peq[c][w] = w < wb ? planes[(static_cast<size_t>(c) * wn + w0 + w) * kLanes] : 0u;
            pv[w] = ~0u;
            mv[w] = 0u;
        }
        for (int i0 = 0; i0 < m; i0 += kPlaceRows) {
            const int rows = m - i0 < kPlaceRows ? m - i0 : kPlaceRows;
            uint32_t *cw = carries + static_cast<size_t>(i0 >> 5) * 3 * kLanes;
            // every load of the block at its head
            uint32_t in_hp = 0, in_hn = 0, in_add = 0;
            if (!leftmost) {
                in_hp = cw[0];
                in_hn = cw[kLanes];
                in_add = cw[2 * kLanes];
            }
            unsigned long long lo = 0, hi = 0;
            block_classes(row, m, i0, rows, &lo, &hi);
            uint32_t out_hp = 0, out_hn = 0, out_add = 0;
#pragma unroll 1
            for (int r = 0; r < rows; r++) {
                const uint32_t c = static_cast<uint32_t>(lo) & 15u;
                lo = (lo >> 4) | (hi << 60);
                hi >>= 4;
                const uint32_t k0 = 0u - (c == 0), k1 = 0u - (c == 1), k2 = 0u - (c == 2), k3 = 0u - (c == 3), k4 = 0u - (c == 4);
                uint32_t carry = (in_add >> r) & 1u, hp_in = (in_hp >> r) & 1u, hn_in = (in_hn >> r) & 1u;
                uint32_t top_hp = 0, top_hn = 0;
#pragma unroll
                for (int w = 0; w < W; w++) {
                    if (w < wb) {
                        const uint32_t eq = (peq[0][w] & k0) | (peq[1][w] & k1) | (peq[2][w] & k2) | (peq[3][w] & k3) | (peq[4][w] & k4);
                        const uint32_t x = pv[w];
                        const unsigned long long s = static_cast<unsigned long long>(x & eq) + x + carry;
                        carry = static_cast<uint32_t>(s >> 32);
                        const uint32_t d0 = (static_cast<uint32_t>(s) ^ x) | eq | mv[w];
                        const uint32_t hp = ~(d0 | x) | mv[w];
                        const uint32_t hn = d0 & x;
                        const uint32_t hps = (hp << 1) | hp_in;
                        const uint32_t hns = (hn << 1) | hn_in;
                        hp_in = hp >> 31;
                        hn_in = hn >> 31;
                        pv[w] = ~(d0 | hps) | hns;
                        mv[w] = d0 & hps;
                        top_hp = hp;
                        top_hn = hn;
                    }
                }
                out_hp |= hp_in << r;
                out_hn |= hn_in << r;
                out_add |= carry << r;
                if (rightmost) {
                    run += static_cast<int>((top_hp >> top) & 1u) - static_cast<int>((top_hn >> top) & 1u);
                    if (run < best) {   // strict: the smallest row among equals
                        best = run;
                        e = i0 + r + 1;
                    }
                }
            }
            if (!rightmost) {
                cw[0] = out_hp;
                cw[kLanes] = out_hn;
                cw[2 * kLanes] = out_add;
            }
        }
    }

    a.distance[p] = best;
    g.span[4 * p + 0] = -1;
    g.span[4 * p + 1] = e;
    g.span[4 * p + 2] = 0;
    g.span[4 * p + 3] = n;
    if (best > g.bound) a.n_ops[p] = 0;   // beyond the bound: the exact distance and the end row are all there is
}

template <int WB>
__global__ __launch_bounds__(kLanes) void place_pairs_forward_kernel(PlaceArgs g, int64_t first)
{
    const PairArgs &a = g.p;
    const int lane = threadIdx.x;
    const int64_t p = first + static_cast<int64_t>(blockIdx.x) * kLanes + lane;
    int q = 0;
    int64_t col = 0;
    if (!owned_pair(a, p, false, &q, &col)) return;
    const int dstar = a.distance[p];
    if (dstar > g.bound) return;
    const int wn = a.word_num, m = a.ref_len, n = a.read_len, bound = g.bound;
    const int vrows = n + bound;                      // M'
    const int o = g.span[4 * p + 1] - n - bound;      // query row = virtual row + o

    const uint32_t *planes = a.peq + static_cast<size_t>(col >> 6) * kChars * wn * kLanes + (col & (kLanes - 1));
    unsigned char *slice = a.workspace + static_cast<size_t>(blockIdx.x) * a.wave_bytes;
    uint32_t *h = reinterpret_cast<uint32_t *>(slice) + lane;
    uint32_t *state = reinterpret_cast<uint32_t *>(slice + g.state_off) + lane;   // [pv | mv][word][lane], then the flag
    for (int w = 0; w < wn; w++) {
        state[static_cast<size_t>(w) * kLanes] = ~0u;
        state[static_cast<size_t>(wn + w) * kLanes] = 0u;
    }

    const unsigned char *row = reinterpret_cast<const unsigned char *>(a.content) + static_cast<size_t>(q) * (m + 1);
    const size_t row_words = static_cast<size_t>(2) * g.band_words * kLanes;
    int edge_rows = 0;   // rows run with hp_in = 1
    for (int i0 = 0; i0 < vrows; i0 += kPlaceRows) {
        int wa = 0, wlast = 0;
        place_window(n, bound, i0, &wa, &wlast);
        const int wb = wlast - wa + 1;           // wave-uniform, 1 .. WB (the launcher dispatches on the widest one)
        const uint32_t edge = wa == 0 ? 0u : 1u;   // the free column 0 feeds 0

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
        const int rows = vrows - i0 < kPlaceRows ? vrows - i0 : kPlaceRows;
        unsigned long long lo = 0, hi = 0;
        block_classes(row, m, i0 + o, rows, &lo, &hi);   // virtual row i0 + r + 1 is query row i0 + r + 1 + o, 0-based one less
        edge_rows += edge ? rows : 0;

#pragma unroll 1
        for (int r = 0; r < rows; r++) {
            const uint32_t c = static_cast<uint32_t>(lo) & 15u;
            lo = (lo >> 4) | (hi << 60);
            hi >>= 4;
            const uint32_t k0 = 0u - (c == 0), k1 = 0u - (c == 1), k2 = 0u - (c == 2), k3 = 0u - (c == 3), k4 = 0u - (c == 4);
            uint32_t carry = 0, hp_in = edge, hn_in = 0;
#pragma unroll
            for (int w = 0; w < WB; w++) {
                if (w < wb) {   // a window narrower than WB runs its own words only
                    const uint32_t e = (peq[0][w] & k0) | (peq[1][w] & k1) | (peq[2][w] & k2) | (peq[3][w] & k3) | (peq[4][w] & k4);
                    const uint32_t x = pv[w];
                    const unsigned long long s = static_cast<unsigned long long>(x & e) + x + carry;
                    carry = static_cast<uint32_t>(s >> 32);
                    const uint32_t d0 = (static_cast<uint32_t>(s) ^ x) | e | mv[w];
                    const uint32_t hp = ~(d0 | x) | mv[w];
                    const uint32_t hn = d0 & x;
                    const uint32_t hps = (hp << 1) | hp_in;
                    const uint32_t hns = (hn << 1) | hn_in;
                    hp_in = hp >> 31;
                    hn_in = hn >> 31;
                    pv[w] = ~(d0 | hps) | hns;
                    mv[w] = d0 & hps;
                    h[static_cast<size_t>(w) * kLanes] = e | ~d0;
                    h[static_cast<size_t>(g.band_words + w) * kLanes] = e | (d0 & hp);
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

    int score = edge_rows;
    for (int w = 0; w < wn; w++) {
        const int rem = n - 32 * w;
        const uint32_t mask = rem >= 32 ? ~0u : ((1u << rem) - 1u);   // rem >= 1: w < word_num
        score += __popc(state[static_cast<size_t>(w) * kLanes] & mask) - __popc(state[static_cast<size_t>(wn + w) * kLanes] & mask);
    }
    const bool certified = score == dstar;
    state[static_cast<size_t>(2) * wn * kLanes] = certified ? 1u : 0u;
    if (!certified) {   // cannot happen for D* <= B
        atomicOr(a.fault_word, static_cast<unsigned>(BGSA_HIP_FAULT_BAND));
        a.n_ops[p] = 0;
    }
}

__global__ __launch_bounds__(kLanes) void place_pairs_traceback_kernel(PlaceArgs g, int64_t first)
{
    const PairArgs &a = g.p;
    const int lane = threadIdx.x;
    const int64_t p = first + static_cast<int64_t>(blockIdx.x) * kLanes + lane;
    int q = 0;
    int64_t col = 0;
    if (!owned_pair(a, p, false, &q, &col)) return;
    if (a.distance[p] > g.bound) return;   // beyond the bound: locate has said so
    unsigned char *slice = a.workspace + static_cast<size_t>(blockIdx.x) * a.wave_bytes;
    const uint32_t *hist = reinterpret_cast<const uint32_t *>(slice) + lane;
    const uint32_t *state = reinterpret_cast<const uint32_t *>(slice + g.state_off) + lane;
    if (!state[static_cast<size_t>(2) * a.word_num * kLanes]) return;   // not certified: the forward kernel has raised the fault
    unsigned char *ops = slice + g.ops_off + lane;   // [step][lane]
    const size_t row_words = static_cast<size_t>(2) * g.band_words * kLanes;

    const int n = a.read_len, bound = g.bound;
    const int o = g.span[4 * p + 1] - n - bound;
    int iv = n + bound, j = n;   // the virtual row of query row e
    size_t steps = 0;
    while (j > 0) {
        int op;
        if (iv + o == 0) {   // query row 0: what is left of the subject hangs off the query's start
            op = kOpD;
            j--;
        } else {
            int wa = 0, wlast = 0;
            const int w = (j - 1) >> 5;
            if (iv >= 1) place_window(n, bound, (iv - 1) & ~(kPlaceRows - 1), &wa, &wlast);
            if (iv < 1 || w < wa || w > wlast) {   // cannot happen for a certified pair; a bug must not become an out-of-bounds load
                atomicOr(a.fault_word, static_cast<unsigned>(BGSA_HIP_FAULT_BAND));
                a.n_ops[p] = 0;
                return;
            }
            int jj = j - 32 * wa;   // the column inside the block's window
            op = history_step(hist, row_words, g.band_words, &iv, &jj);
            j = jj + 32 * wa;
        }
        ops[steps * kLanes] = static_cast<unsigned char>(op);
        steps++;
    }
    g.span[4 * p + 0] = iv + o;   // q_begin: the row of the first cell with j = 0
    a.n_ops[p] = encode_runs(ops, steps, a.cigar + static_cast<size_t>(p) * a.cigar_cap, a.cigar_cap);
}

// One chunk: locate, the forward kernel of the widest window, the traceback.
int launch_place(const PlaceArgs &g, dim3 grid, int64_t first, hipStream_t stream)
{
    hipLaunchKernelGGL(place_pairs_locate_kernel, grid, dim3(kLanes), 0, stream, g, first);
    BGSA_HIP_TRY(hipGetLastError());
    const int rc = PlaceWidths::dispatch(g.band_words, "myers_place_pairs_banded", [&](auto width) {
        hipLaunchKernelGGL((place_pairs_forward_kernel<decltype(width)::value>), grid, dim3(kLanes), 0, stream, g, first);
        BGSA_HIP_TRY(hipGetLastError());
        return BGSA_HIP_OK;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(place_pairs_traceback_kernel, grid, dim3(kLanes), 0, stream, g, first);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

// The largest max_distance whose windows the kernels hold for a read of n bp (band_words is monotone in it).
int largest_place_bound(int n)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (place_band_words_of(n, mid) <= kPlaceMaxWords) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

}  // namespace

}  // namespace bgsa

using namespace bgsa;

extern "C" {

int bgsa_hip_place_pairs_band_words(int read_len, int max_distance) { return place_band_words_of(read_len, max_distance); }

size_t bgsa_hip_place_pairs_banded_min_workspace_bytes(int ref_len, int read_len, int max_distance)
{
    if (ref_len <= 0 || read_len <= 0 || max_distance < 0) return 0;
    return place_wave_bytes(ref_len, read_len, max_distance, place_band_words_of(read_len, max_distance));
}

size_t bgsa_hip_place_pairs_banded_workspace_bytes(int ref_len, int read_len, int max_distance, int64_t n_pairs)
{
    if (ref_len <= 0 || read_len <= 0 || max_distance < 0 || n_pairs < 0) return 0;
    return pair_workspace_for(place_wave_bytes(ref_len, read_len, max_distance, place_band_words_of(read_len, max_distance)), n_pairs);
}

int bgsa_hip_myers_place_pairs_banded_dev(const char *d_content, const hip_read_t *d_peq, int ref_len, int read_len, int64_t read_count,
                                          int word_num, const int32_t *d_pair_query, const int64_t *d_pair_subject, int64_t n_pairs,
                                          int n_queries, int64_t subject_base, int max_distance, int32_t *d_distance, int32_t *d_span,
                                          int32_t *d_n_ops, uint32_t *d_cigar, int cigar_cap, void *d_workspace, size_t workspace_bytes,
                                          void *stream)
{
    const char *who = "myers_place_pairs_banded_dev";
    if (int rc = check_pair_call(who, !d_content || !d_peq || !d_pair_query || !d_pair_subject || !d_distance || !d_span || !d_n_ops || !d_cigar,
                                 "a NULL pointer (only the workspace and the stream may be NULL)", n_pairs, ref_len, read_len, n_queries, cigar_cap,
                                 read_count))
        return rc;
    if (word_num != bgsa_hip_word_num(BGSA_ALGO_MYERS, ref_len, read_len, 0))
        return refuse(who, BGSA_HIP_EINVAL, "word_num is not bgsa_hip_word_num(BGSA_ALGO_MYERS, ...)");
    if (max_distance < 0) return refuse(who, BGSA_HIP_EINVAL, "max_distance is negative");
    if (!place_counts_fit(ref_len, read_len, max_distance))
        return refuse(who, BGSA_HIP_EUNSUPPORTED, "ref_len + read_len + min(max_distance, read_len) beyond 2^31 - 1");
    const int band_words = place_band_words_of(read_len, max_distance);
    if (band_words > kPlaceMaxWords) {
        char why[200];
        snprintf(why, sizeof why, "the windows of max_distance %d are %d words wide, the kernels hold %d: a %d bp read takes max_distance <= %d",
                 max_distance, band_words, kPlaceMaxWords, read_len, largest_place_bound(read_len));
        return refuse(who, BGSA_HIP_EUNSUPPORTED, why);
    }
    const size_t per = place_wave_bytes(ref_len, read_len, max_distance, band_words);
    if (d_workspace && workspace_bytes < per)
        return refuse(who, BGSA_HIP_EINVAL, "workspace smaller than bgsa_hip_place_pairs_banded_min_workspace_bytes()");
    if (n_pairs == 0) return BGSA_HIP_OK;

    PlaceArgs args{};
    const size_t hist = place_hist_bytes(read_len, max_distance, band_words);
    args.p = PairArgs{d_content, d_peq, ref_len, read_len, read_count, word_num, d_pair_query, d_pair_subject, n_pairs, n_queries,
                      subject_base, d_distance, d_n_ops, d_cigar, cigar_cap, nullptr, per, hist, device_fault_word(), nullptr};
    if (!args.p.fault_word) return BGSA_HIP_EHIP;
    args.span = d_span;
    args.bound = place_bound(read_len, max_distance);
    args.band_words = band_words;
    args.state_off = hist;
    args.carry_off = hist + place_state_bytes(read_len);
    args.ops_off = args.carry_off + place_carry_bytes(ref_len);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return run_pair_chunks(d_workspace, workspace_bytes, per, n_pairs, s, [&](unsigned char *workspace, dim3 grid, int64_t first) {
        args.p.workspace = workspace;
        return launch_place(args, grid, first, s);
    });
}

}  // extern "C"
