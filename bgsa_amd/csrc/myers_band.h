// myers_band.h — the certified diagonal band of the Myers global kernels.
//
// A path through cell (i, j) of the m x n matrix (query rows, subject columns) holds at least |d| + |d - (n - m)| indels,
// d = j - i.  If a pair's distance is <= B = 2h + 1, its optimal paths stay inside the band |d| + |d - (n - m)| <= B, and a
// row needs only the words that hold the band's columns: its WINDOW [a, b].  Words left of the window keep their last
// deltas (the lowest active word gets the row-edge carry-ins, a vertical step), words right of it keep their initial
// state (a horizontal path), so every column still holds the cost of a real path: the score D' >= D, and D' <= B
// certifies D' = D.  A wave with a lane above B runs the query again with full rows (myers_global_asm_kernel<NW, 1, *, true>).
//
// Band stream (one per query, 8-byte windows, `band_stream_stride` bytes): the plain stream's codes — 0..4 rows, 5 END,
// 6 REFILL — plus 7 = SETWIN followed by one byte, the slot group (band_window_index) of the rows that follow.  A SETWIN
// and its byte always share a window: where only byte 6 is left, a REFILL there ends the window early.  The packer pads
// with END up to the stride; the last window is all END.  rows_ir.py: myers_band_stream restates it.
#pragma once

#include <stdlib.h>

#include "bgsa_common.h"

namespace bgsa {

constexpr int kBandMaxWords = 8;                        // widths with windowed bodies (gen_rows_asm.py: MYERS_BAND_NW): 65..256 bp
constexpr int kBandMinWords = 3;
constexpr int kBandMaxSwitches = 2 * kBandMaxWords;     // a query's window changes at most 2 NW - 2 times after the first
constexpr int kCodeSetWin = 7;
constexpr int kBandBadCode = 0xff;                      // SETWIN with a window byte past the last group: the loop's fail exit

struct BandSchedule {
    int n = 0;                        // windows of the query (0: band off)
    int row[kBandMaxSwitches] = {};   // first query row (0-based) of each window
    int win[kBandMaxSwitches] = {};   // its slot group
};

__host__ __device__ inline int band_window_index(int nw, int a, int b) { return a * nw - a * (a - 1) / 2 + (b - a); }
// ... and back: the window [a, b] of slot group `win`.
inline void band_window_of(int nw, int win, int *a, int *b)
{
    *a = 0;
    while (*a + 1 < nw && band_window_index(nw, *a + 1, *a + 1) <= win) ++*a;
    *b = *a + win - band_window_index(nw, *a, *a);
}

// Default half-width for a length: the mean edit distance of random uniform ACGT pairs + 4.5 standard deviations
// (rows_ir.py: myers_band_half, LABNOTES §11): 150 bp -> h = 48, B = 97.
inline int band_default_half(int len) { return (9 * len + 192) / 32; }

// The half-width of a two-group launch that RESCUES (below, "rescue"): three less, 150 bp -> h = 45, B = 91.  There about one
// random pair in a thousand is not certified (LABNOTES §33), and those lanes are scored again one by one instead of their
// waves.  rows_ir.py: myers_band_rescue_half.
inline int band_rescue_half(int len) { return band_default_half(len) - 3; }

// The half-width of a launch: BGSA_MYERS_BAND=0 turns the band off, =N sets h = N (A/B knob); default by the
// longer of the two lengths.  rescue: the launch scores its uncertified lanes again one by one (band_rescue_half).
inline int band_half(int m, int n, bool rescue = false)
{
    static const int knob = [] {
        const char *e = getenv("BGSA_MYERS_BAND");
        return e ? atoi(e) : -1;
    }();
    if (knob >= 0) return knob;
    return rescue ? band_rescue_half(m > n ? m : n) : band_default_half(m > n ? m : n);
}

// The windows of every row of an m-row query against nw-word subjects of length n: false (s->n = 0) when the band is off
// for this shape — |n - m| > B, a width without windowed bodies, or windows that would not save a fifth of the word-rows.
// rows_ir.py: myers_band_windows.
inline bool band_schedule(int m, int n, int h, int nw, BandSchedule *s)
{
    s->n = 0;
    const int B = 2 * h + 1, delta = n - m;
    if (h <= 0 || m <= 0 || n <= 0 || abs(delta) > B || nw < kBandMinWords || nw > kBandMaxWords || (n + 31) / 32 != nw)
        return false;
    const int dlo = -((B - delta) / 2), dhi = (delta + B) / 2;   // ceil((delta - B) / 2), floor((delta + B) / 2): both numerators >= 0
    long long words = 0;
    int pa = -1, pb = -1;
    for (int i = 1; i <= m; i++) {
        const int jlo = i + dlo < 1 ? 1 : i + dlo, jhi = i + dhi > n ? n : i + dhi;
        const int a = (jlo - 1) / 32, b = (jhi - 1) / 32;
        words += b - a + 1;
        if (a != pa || b != pb) {
            if (s->n == kBandMaxSwitches) {
                s->n = 0;
                return false;
            }
            s->row[s->n] = i - 1;
            s->win[s->n] = band_window_index(nw, a, b);
            s->n++;
            pa = a;
            pb = b;
        }
    }
    if (5 * words > 4ll * m * nw) {
        s->n = 0;
        return false;
    }
    return true;
}

// ---- early leave (LABNOTES §37) --------------------------------------------------------------------------------
// The static rule keeps a low word in the window until its last column j_r = 32 (w + 1) lies more than h diagonals below the
// row: all it knows is D[i][j] >= i - j.  The state knows D'[r][j_r] itself.  D'[r][j] - j does not grow with j, so every
// in-window cell (r, j), j <= j_r, has D'[r][j] + (r - j) >= M = D'[r][j_r] + (r - j_r), and a path that enters the rows
// behind r in columns <= j_r costs at least M (n = m).  Word w may therefore leave behind ANY row r >= j_r: the banded score
// stays exact for every lane with D' <= min(B, M) — a limit per lane.  A lane above it is what a lane above B is: a pool entry
// (rescue, below).  A CUT {row, word}: behind `row` rows (1-based row r of the text) the window's low end is at least word + 1.
// Behind the cut no row touches words 0 .. w again, so they still hold D'[r][j_r] - r when the query ends: the kernel forms M
// there, beside the score, from the state it has — the cuts cost the row loop nothing, and the stream is the band stream of
// the schedule with the cuts applied (whole, or in the segments of prefix sharing): no segment and no code of its own.
constexpr int kBandMaxCuts = 2;
struct BandCuts {
    int n = 0;                      // cuts (0: the static schedule)
    int row[kBandMaxCuts] = {};     // ascending
    int word[kBandMaxCuts] = {};    // ascending
};
// The cut rows of the default rescue lengths (band_rescue_lengths, n = m, h = band_rescue_half): per leaving word the earliest
// row at which the cut adds at most 5e-5 of random uniform pairs to the rescue, the two words that save most; lengths whose
// cuts save under 2 % of the word-rows have none (scripts/band_early_cuts.py, profiles/r12_band_early_cuts.txt).
// 150 bp keeps the rows of the first CPU check, (106, 130): four and five rows behind the script's (102, 125), which costs
// word-rows and never a score — the script's pair there waits for an A/B on the GPU (LABNOTES §37).
struct BandEarlyEntry {
    int len, n, row[kBandMaxCuts], word[kBandMaxCuts];
};
constexpr BandEarlyEntry kBandEarlyCuts[] = {
    {68, 1, {51, 0}, {0, 0}},
    {96, 2, {60, 83}, {0, 1}},
    {100, 2, {62, 85}, {0, 1}},
    {107, 2, {64, 88}, {0, 1}},
    {111, 2, {65, 89}, {0, 1}},
    {114, 2, {66, 90}, {0, 1}},
    {118, 2, {67, 92}, {0, 1}},
    {121, 2, {68, 93}, {0, 1}},
    {125, 2, {69, 94}, {0, 1}},
    {128, 2, {70, 95}, {0, 1}},
    {132, 2, {71, 96}, {0, 1}},
    {139, 2, {99, 121}, {1, 2}},
    {143, 2, {100, 122}, {1, 2}},
    {146, 2, {101, 123}, {1, 2}},
    {150, 2, {106, 130}, {1, 2}},
    {153, 2, {104, 126}, {1, 2}},
    {157, 2, {105, 128}, {1, 2}},
    {160, 2, {106, 129}, {1, 2}},
};
// The cuts of an m x n launch at half-width h: none unless n = m, the length is in the table and h is the table's.
inline BandCuts band_early_cuts(int m, int n, int h)
{
    BandCuts c;
    if (m != n || h != band_rescue_half(n)) return c;
    for (const BandEarlyEntry &e : kBandEarlyCuts)
        if (e.len == n) {
            c.n = e.n;
            for (int j = 0; j < e.n; j++) c.row[j] = e.row[j], c.word[j] = e.word[j];
        }
    return c;
}
// What the kernel gets of the cuts, in the launch's band_limit above B: per cut 2 r - j_r (nine bits) and w (two).
constexpr int kBandEarlyLimitBits = 10, kBandEarlyCutBits = 11;
constexpr int kBandEarlyLimitMask = (1 << kBandEarlyLimitBits) - 1;
inline int band_early_word(int band_limit, const BandCuts &c)
{
    unsigned v = static_cast<unsigned>(band_limit) & kBandEarlyLimitMask;
    for (int j = 0; j < c.n; j++)
        v |= (static_cast<unsigned>(2 * c.row[j] - 32 * (c.word[j] + 1)) | static_cast<unsigned>(c.word[j]) << 9)
             << (kBandEarlyLimitBits + kBandEarlyCutBits * j);
    return static_cast<int>(v);
}
// band_schedule with the cuts applied: rows behind cut j run on windows whose low end is at least word[j] + 1.  False (s->n = 0,
// as band_schedule) also where a cut is out of order, lies above its word's last column (r < j_r: the bound needs r >= j_r),
// or would empty a window.  rows_ir.py: myers_band_windows(cuts = ...).
inline bool band_schedule_early(int m, int n, int h, int nw, const BandCuts &cuts, BandSchedule *s)
{
    if (cuts.n == 0) return band_schedule(m, n, h, nw, s);
    BandSchedule base;
    s->n = 0;
    if (m != n || cuts.n < 0 || cuts.n > kBandMaxCuts || !band_schedule(m, n, h, nw, &base)) return false;
    for (int j = 0; j < cuts.n; j++)
        if (cuts.word[j] < 0 || cuts.word[j] >= nw - 1 || cuts.row[j] < 32 * (cuts.word[j] + 1) || cuts.row[j] >= m ||
            (j && (cuts.row[j] <= cuts.row[j - 1] || cuts.word[j] <= cuts.word[j - 1])))
            return false;
    int pw = -1, sw = 0;
    for (int r = 0; r < m; r++) {   // 0-based row r is behind cut j when r >= cuts.row[j]
        while (sw + 1 < base.n && base.row[sw + 1] <= r) sw++;
        int a, b;
        band_window_of(nw, base.win[sw], &a, &b);
        for (int j = 0; j < cuts.n; j++)
            if (r >= cuts.row[j] && a < cuts.word[j] + 1) a = cuts.word[j] + 1;
        if (a > b || s->n == kBandMaxSwitches) {
            s->n = 0;
            return false;
        }
        const int win = band_window_index(nw, a, b);
        if (win != pw) {
            s->row[s->n] = r;
            s->win[s->n] = win;
            s->n++;
            pw = win;
        }
    }
    return true;
}
// Word-rows of a schedule (per subject group).
inline long long band_schedule_word_rows(int m, int nw, const BandSchedule &s)
{
    long long words = 0;
    for (int i = 0; i < s.n; i++) {
        int a, b;
        band_window_of(nw, s.win[i], &a, &b);
        words += static_cast<long long>((i + 1 < s.n ? s.row[i + 1] : m) - s.row[i]) * (b - a + 1);
    }
    return words;
}

// Bytes of one band stream, padded like the plain one: the codes, at most 3 bytes per window change (SETWIN, its byte, a
// byte 7 skipped by an early REFILL), END, the spare window.
inline size_t band_stream_stride(int ref_len) { return stream_stride(ref_len + 3 * kBandMaxSwitches); }

// Writes bytes [first, first + count) of the stream of rows r0 .. r1 - 1 of one query (row = its mapped characters) to
// dst[0 .. count) when dst != nullptr and returns the length in bytes — or, once the range is written, the position after
// it.  The stream begins with the SETWIN of row r0's window, ends with END padded to its 8-byte window and, if `spare`, the
// all-END window that the loops fetch ahead.  Where the SETWIN and REFILL bytes go depends on the schedule only, so the
// packers give every 8-byte window a thread of its own, which reads the (at most seven) characters of its window and no
// others.  Rows 0 .. len - 1 with the spare window are the band stream of a query (band_stream_layout); a query's stream in
// segments (prefix sharing, below) is one such stream per segment.
__host__ __device__ inline int band_rows_layout(const BandSchedule &s, int r0, int r1, bool spare, const char *row, unsigned char *dst,
                                                int first = 0, int count = 0x7fffffff)
{
    int pos = 0, sw = 0;
    auto in = [&]() { return dst && pos >= first && pos - first < count; };
    auto put = [&](int c) {
        if (in()) dst[pos - first] = static_cast<unsigned char>(c);
        pos++;
    };
    auto refill = [&]() {
        put(kCodeRefill);
        while (pos & 7) put(kCodeEnd);
    };
    while (sw + 1 < s.n && s.row[sw + 1] <= r0) sw++;   // the window row r0 runs on (s.row[0] = 0)
    for (int r = r0; r < r1; r++) {
        if (dst && pos - first >= count) return pos;
        if (sw < s.n && (s.row[sw] == r || r == r0)) {
            if ((pos & 7) >= 6) refill();
            put(kCodeSetWin);
            put(s.win[sw]);
            sw++;
        }
        if ((pos & 7) == 7) refill();
        if (in()) {
            const unsigned c = static_cast<unsigned char>(row[r]);
            dst[pos - first] = static_cast<unsigned char>(c > 4 ? 0u : c);   // as plain_stream_window: out-of-alphabet bytes behave as 'A'
        }
        pos++;
    }
    if ((pos & 7) == 7) refill();
    put(kCodeEnd);
    while (pos & 7) put(kCodeEnd);
    for (int j = 0; spare && j < 8; j++) put(kCodeEnd);
    return pos;
}

// ... of the whole query: the band stream (<= band_stream_stride bytes).  Shared by the packer kernel and bgsa_hip_myers_band_stream.
__host__ __device__ inline int band_stream_layout(int len, const BandSchedule &s, const char *row, unsigned char *dst,
                                                  int first = 0, int count = 0x7fffffff)
{
    return band_rows_layout(s, 0, len, true, row, dst, first, count);
}

// ---- prefix sharing ------------------------------------------------------------------------------------------
// The state after query row r depends on the subjects and on the query's first r characters only.  A wave walks a tile of
// queries over the same subjects, so with the tile's queries in sorted order a query that begins like its predecessor need
// not run the rows they share: the wave keeps the state after rows d_1 < d_2 < ... (the DEPTHS, launch constants) of the
// current query's prefix in LDS and a query resumes behind the deepest depth <= its common prefix with the predecessor.
// The packer writes each query's stream in segments — rows 1..d_1, d_1+1..d_2, ..., d_n+1..m, each a stream of its own
// (band_rows_layout) at an offset that depends on the schedule only.  Only where rows 1..d_n run on words 0..1: the snapshot
// is those two words of each group, the other words still hold their initial state.
constexpr int kPrefixMaxDepths = 5;
constexpr int kPrefixKeyChars = 10;                     // characters of the sort key, 3 bits each; also the deepest depth
struct PrefixPlan {
    int n = 0;                                // depths (0: no sharing — one segment, the band stream as ever)
    int depth[kPrefixMaxDepths] = {};         // ascending, 1 .. kPrefixKeyChars
    int off[kPrefixMaxDepths + 2] = {};       // byte offset of segment j in a query's stream, j = 0 .. n; off[n + 1] = the stride
};
// Bytes per query that n_depths more segments add at most: per cut the SETWIN and its byte, the END and its padding.
inline size_t band_segments_stride_bound(int ref_len) { return band_stream_stride(ref_len) + 16 * kPrefixMaxDepths; }

// Fills the segment offsets for depths p->depth[0 .. n); false (p->n = 0) where the shape does not qualify: a depth outside
// 1 .. min(kPrefixKeyChars, m - 1), depths not ascending, or a row up to the deepest depth whose window leaves words 0..1.
inline bool prefix_plan_layout(int m, int nw, const BandSchedule &s, PrefixPlan *p)
{
    const int n = p->n;
    p->n = 0;
    if (n < 1 || n > kPrefixMaxDepths || s.n < 1) return false;
    for (int j = 0; j < n; j++)
        if (p->depth[j] < 1 || p->depth[j] > kPrefixKeyChars || p->depth[j] >= m || (j && p->depth[j] <= p->depth[j - 1])) return false;
    for (int i = 0; i < s.n && s.row[i] < p->depth[n - 1]; i++)   // windows (0, 0) and (0, 1) are slot groups 0 and 1
        if (s.win[i] != band_window_index(nw, 0, 0) && s.win[i] != band_window_index(nw, 0, 1)) return false;
    int pos = 0;
    for (int j = 0; j <= n; j++) {
        p->off[j] = pos;
        pos += band_rows_layout(s, j ? p->depth[j - 1] : 0, j < n ? p->depth[j] : m, j == n, nullptr, nullptr);
    }
    p->off[n + 1] = pos;
    if (static_cast<size_t>(pos) > band_segments_stride_bound(m) || pos / 8 > 255) return false;   // (prefix_segments_word: a byte per offset)
    p->n = n;
    return true;
}

// One entry per query of a sharing launch, in sorted order, behind the streams and the task counter's kTaskCounterBytes:
// q = the query (relative to ref_start), lcp = its common prefix with the sorted predecessor, capped at the deepest depth and
// 0 for the first query of every tile, seg = the segment it may start at (the depths <= lcp).  The sort keys follow the entries
// (scratch of the launch).
struct PrefixEntry {
    int q;
    short lcp, seg;
};
inline size_t prefix_order_bytes(int n_queries) { return static_cast<size_t>(n_queries) * (sizeof(PrefixEntry) + sizeof(uint32_t)) + 256; }
__host__ __device__ inline PrefixEntry *prefix_entries(unsigned *task_counter)
{
    return reinterpret_cast<PrefixEntry *>(reinterpret_cast<unsigned char *>(task_counter) + kTaskCounterBytes);
}
// What the kernel gets of a plan, one word: byte j <= n = off[j] / 8, the top byte = n (0: no sharing).
inline unsigned long long prefix_segments_word(const PrefixPlan &p)
{
    unsigned long long w = static_cast<unsigned long long>(p.n) << 56;
    for (int j = 0; j <= p.n && p.n; j++) w |= static_cast<unsigned long long>(p.off[j] / 8) << (8 * j);
    return w;
}

// Sorts queries ref_start .. ref_end - 1 by their first kPrefixKeyChars class codes and writes the entries (q_tile: the
// launch's queries per task); then packs their streams in the segments of `p` and zeroes the task counter and the guard's
// pair, as launch_pack_band does.  All on `stream`, nothing read back.
int launch_prefix_order(const char *d_content, int ref_len, int ref_start, int ref_end, int q_tile, const PrefixPlan &p,
                        unsigned *d_words, hipStream_t stream);   // preprocess.hip
int launch_pack_band_segments(const char *d_content, int ref_len, const BandSchedule &s, const PrefixPlan &p, int ref_start,
                              int ref_end, void *d_streams, hipStream_t stream, unsigned *d_words,
                              unsigned rescue_entries = 0);   // preprocess.hip

// The guard's pair of one launch, {queries redone, queries banded} (myers_global_asm_kernel<NW, 1, *, true>): 64 bytes behind
// the task counter, inside the kTaskCounterBytes behind the streams; zeroed by the packer with the counter.
__host__ __device__ inline unsigned long long *band_launch_words(unsigned *task_counter)
{
    return reinterpret_cast<unsigned long long *>(task_counter + 16);
}

// Packs the band streams of queries ref_start .. ref_end - 1 and zeroes the task counter d_words[0], the guard's pair and the
// rescue's words (below; rescue_entries: the pool's capacity, 0 for a launch that does not rescue).
int launch_pack_band(const char *d_content, int ref_len, const BandSchedule &s, int ref_start, int ref_end, void *d_streams,
                     hipStream_t stream, unsigned *d_words, unsigned rescue_entries = 0);   // preprocess.hip

// Certificate statistics, per device: [0] = queries a wave ran again with full rows, [1] = queries a wave ran banded,
// [2] = lanes rescued, [3] = group-queries a rescuing wave sent through the full rows after all (below).
// They live behind the sticky fault word (bgsa_common.h: device_fault_word, a 64-byte allocation) and are read and
// cleared by bgsa_hip_myers_band_stats() and bgsa_hip_myers_band_rescue_stats().
__host__ __device__ inline unsigned long long *band_stats_words(unsigned *fault_word)
{
    return reinterpret_cast<unsigned long long *>(fault_word + 2);
}

// ---- rescue ----------------------------------------------------------------------------------------------------
// A two-group launch on a large bucket runs a narrower band (band_rescue_half) and does not send a wave through the full rows
// for a few uncertified lanes: a live group with 1 .. kRescueMaxLanes lanes above B writes {query, subject} of each into the
// launch's POOL, those lanes store no score, and myers_band_rescue_kernel scores the pool's pairs afterwards, one pair per
// lane with full rows.  A group with more such lanes, or a pool that is full, takes the wave through the full rows as ever.
// The pool lies in the workspace behind the prefix entries and their keys; band_launch_words [2], [3] are the launch's
// {lanes rescued (counted by the rescue kernel), group-queries redone because of the lane limit or a full pool}, [4] counts
// the entries claimed, and the word behind it holds the pool's capacity.  The packers zero the five and write the capacity.
constexpr int kRescueMaxLanes = 8;
constexpr int kRescueMinLen = 65, kRescueMaxLen = 160;   // the two-group band kernels: 3..5 words
struct RescueEntry {
    int q, subject;   // q relative to ref_start; {-1, -1}: claimed by a wave that found the pool full
};
__host__ __device__ inline unsigned long long *rescue_claimed(unsigned *task_counter) { return band_launch_words(task_counter) + 4; }
__host__ __device__ inline unsigned *rescue_capacity(unsigned *task_counter) { return task_counter + 26; }
// ... and the next one where the pool begins, in entries behind the prefix entries: behind them and their keys
// (rescue_pool_offset: the packers write it, so that the kernels need no query count for it).
__host__ __device__ inline unsigned *rescue_offset(unsigned *task_counter) { return task_counter + 27; }
__host__ __device__ inline unsigned rescue_pool_offset(int n_queries)
{
    return static_cast<unsigned>((static_cast<size_t>(n_queries) * (sizeof(PrefixEntry) + sizeof(uint32_t)) + 7) / 8);
}
__device__ __forceinline__ RescueEntry *rescue_pool(unsigned *task_counter)
{
    const unsigned at = __builtin_amdgcn_readfirstlane(*rescue_offset(task_counter));
    return reinterpret_cast<RescueEntry *>(reinterpret_cast<unsigned char *>(task_counter) + kTaskCounterBytes) + at;
}
// Where a launch may rescue by default: lengths at which no more than 2 in 1,000 random pairs lie above the rescue band's B,
// and nearly equal ones, which is where that rate was measured (LABNOTES §33).  band_default_half rounds down, and where it
// loses a quarter or more of a column the rate at h - 3 reaches or passes that — 66 and 80 bp: 4 in 1,000.
constexpr int kRescueMaxDelta = 3;
inline bool band_rescue_lengths(int m, int n)
{
    const int len = m > n ? m : n;
    return n >= kRescueMinLen && n <= kRescueMaxLen && abs(n - m) <= kRescueMaxDelta && (9 * len + 192) % 32 < 8;
}
// What plan_workspace_bytes adds for the pool: 4,096 entries per query, 512 MiB at the most; only where a launch may rescue.
inline size_t rescue_pool_bytes(int read_len, int n_queries)
{
    if (read_len < kRescueMinLen || read_len > kRescueMaxLen || n_queries <= 0) return 0;
    const size_t want = static_cast<size_t>(n_queries) << 15, most = static_cast<size_t>(512) << 20;
    return want < most ? want : most;
}
// Its entries.  The task counter in front is aligned up by as much as prefix_order_bytes' spare 256 bytes and the pool by 7
// more, so the last eight entries stay unused.
inline long long rescue_pool_entries(int read_len, int n_queries)
{
    const long long n = static_cast<long long>(rescue_pool_bytes(read_len, n_queries) / sizeof(RescueEntry));
    return n > 8 ? n - 8 : 0;
}

}  // namespace bgsa
