// seed_map.hip — seeded read mapping: an exact pigeonhole k-mer filter in front of the placement (include/bgsa_hip.h "seeded
// read mapping").  ReferenceMapper.map_reads scores every window of the reference against
// every read; these calls look only at the windows that CAN hold a read within the bound, and verify those exactly.
//
// Geometry (the header states it; bgsa_amd/reference.py: seed_plan and tests/seed_map_reference.py restate it).  The windows are those of
// reference_windows.hip: L mapped bytes, 1 <= S <= W <= L, n_windows = 1 + ceil((L - W) / S), start(w) = min(w * S, L - W).
//   index       forward reference only, q = seed_len in 1..13.  Position p is indexed when ref[p .. p + q) are all below 4; its
//               value is sum ref[p + i] * 4^(q - 1 - i).  offsets[4^q + 1], bucket c = positions[offsets[c] .. offsets[c + 1]),
//               any order inside a bucket.
//   pieces      a read of n bp within B = min(max_distance, n) edits: step = n / (B + 1), piece j = 0..B starts at o_j = j * step
//               and is q <= step long, so the pieces are disjoint and one of them is untouched by any B edits.  Forward strand:
//               the pieces of the read; reverse strand: the pieces of its reverse complement, looked up in the same index, a
//               window w found that way has id n_windows + w.
//   candidates  an occurrence at p of the piece at o makes window w a candidate when start(w) <= p, p + q <= start(w) + W,
//               start(w) <= p - o + B and p - o + n - B <= start(w) + W.
//   flags       a read with a class-4 character in any piece of the strands asked for is -1 (N matches N in the scorer, the index
//               has no N: the pigeonhole count does not hold); a read with more than max_candidates candidates is -2.
//   lengths     the *_lens_dev calls: read r is its row's first n_r = lens[r] characters, B_r = min(max_distance, n_r), step_r =
//               n_r / (B_r + 1); the rules above hold with n_r and B_r, and step_r < q (n_r == 0 among them) is flag -3.  The
//               verify kernel's Lens instances take a lane's score column from the lane's own word (LABNOTES §28).
//
// Five steps, each a launch on the caller's stream and nothing else:
//   index build  rolling codes counted with atomics into offsets[c + 1], an inclusive scan over the 4^q counts in three kernels
//                (block sums, their scan by one workgroup, the blocks again with their bases) that also leaves every bucket's
//                start in a cursor array of the workspace, and the same rolling walk filling positions through the cursors.
//   count, emit  one lane per read: the walk over its pieces' buckets, counting or writing (read, window id).
//   verify       the hot kernel: one pair per lane, the Myers semi-global row of place_pairs_locate_kernel (free column 0, the
//                window's character per lane, column blocks of kVerifyWords words whose three carries travel as one bit per row);
//                the window's characters are read straight from the mapped reference, forward for forward ids, complemented from
//                the window's end backwards for reverse ids, 32 rows at a time as nine aligned dwords (window_block).  No window
//                row exists anywhere.  A template instance per block width keeps a narrow read's registers low: the words are
//                all live for the whole row loop (36 / 64 / 142 / 228 VGPRs at 1 / 5 / 16 / 32 words, no scratch; LABNOTES §27.2).
//   select       one wave per read: k rounds, each the minimum (distance, id) key above the last one taken.
#include "pair_trace.h"           // the Myers word, the class masks, the chunk loop and the workspace rule
#include "reference_geometry.h"   // Geometry, window_start, make_geometry

namespace bgsa {

namespace {

constexpr int kSeedMaxLen = 13;            // 4^13 + 1 offsets are 268 MB; codes stay below 2^26
constexpr int kSeedChunk = 32;             // reference positions one thread rolls over
constexpr int kScanItems = 8;              // counts per thread of a scan workgroup
constexpr int kScanBlock = 256 * kScanItems;
constexpr int kVerifyRows = 32;            // window characters fetched per block of rows
constexpr int kVerifyWords = 16;           // words of a column block: 5 Peq planes + pv + mv in 112 registers
constexpr int kVerifyMaxWords = 32;
constexpr unsigned kMaxBlocks = 1u << 20;

// ---- index -------------------------------------------------------------------------------------------------------------------
// One thread rolls over kSeedChunk positions.  Fill == false: offsets[code + 1]++.  Fill == true: positions[cursor[code]++] = p.
template <bool Fill>
__global__ __launch_bounds__(256) void seed_index_walk_kernel(const unsigned char *__restrict__ reference, int64_t ref_len, int q,
                                                              int32_t *__restrict__ counters, int32_t *__restrict__ positions)
{
    const int64_t n_pos = ref_len - q + 1;     // >= 1: the launcher has checked
    const int64_t step = static_cast<int64_t>(gridDim.x) * blockDim.x * kSeedChunk;
    const uint32_t mask = (1u << (2 * q)) - 1u;   // q <= 13
    for (int64_t p0 = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) * kSeedChunk; p0 < n_pos; p0 += step) {
        const int64_t p1 = p0 + kSeedChunk < n_pos ? p0 + kSeedChunk : n_pos;
        uint32_t code = 0;
        int valid = 0;
        for (int64_t i = p0; i < p0 + q - 1; i++) {         // i <= p0 + q - 2 < ref_len
            const uint32_t c = reference[i];
            code = (code << 2) | (c & 3u);
            valid = c < 4u ? valid + 1 : 0;
        }
        for (int64_t p = p0; p < p1; p++) {                 // p + q - 1 <= ref_len - 1
            const uint32_t c = reference[p + q - 1];
            code = ((code << 2) | (c & 3u)) & mask;
            valid = c < 4u ? valid + 1 : 0;
            if (valid >= q) {
                if (Fill) positions[atomicAdd(&counters[code], 1)] = static_cast<int32_t>(p);
                else atomicAdd(&counters[code + 1], 1);
            }
        }
    }
}

// Inclusive scan of the 256 values of a workgroup, one per thread; returns this thread's inclusive value, *total = the sum.
__device__ __forceinline__ int block_scan(int v, int *lds, int *total)
{
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int add = t >= d ? lds[t - d] : 0;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    const int mine = lds[t];
    *total = lds[255];
    __syncthreads();
    return mine;
}

// counts = offsets + 1, n of them.  sums[b] = the sum of block b's kScanBlock counts.
__global__ __launch_bounds__(256) void seed_scan_sums_kernel(const int32_t *__restrict__ counts, int64_t n, int32_t *__restrict__ sums)
{
    __shared__ int lds[256];
    const int64_t at = static_cast<int64_t>(blockIdx.x) * kScanBlock + static_cast<int64_t>(threadIdx.x) * kScanItems;
    int v = 0;
#pragma unroll
    for (int i = 0; i < kScanItems; i++)
        if (at + i < n) v += counts[at + i];
    int total = 0;
    block_scan(v, lds, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// One workgroup: sums[b] becomes the sum of all blocks in front of b.
__global__ __launch_bounds__(256) void seed_scan_bases_kernel(int32_t *__restrict__ sums, int64_t n_blocks)
{
    __shared__ int lds[256];
    int running = 0;
    for (int64_t base = 0; base < n_blocks; base += 256) {
        const int64_t b = base + threadIdx.x;
        const int v = b < n_blocks ? sums[b] : 0;
        int total = 0;
        const int inclusive = block_scan(v, lds, &total);
        if (b < n_blocks) sums[b] = running + inclusive - v;
        running += total;
    }
}

// counts[i] becomes the inclusive sum (= offsets[i + 1]), cursor[i] the exclusive one (= offsets[i]: bucket i's start).
__global__ __launch_bounds__(256) void seed_scan_apply_kernel(int32_t *__restrict__ counts, int64_t n, const int32_t *__restrict__ sums,
                                                              int32_t *__restrict__ cursor)
{
    __shared__ int lds[256];
    const int64_t at = static_cast<int64_t>(blockIdx.x) * kScanBlock + static_cast<int64_t>(threadIdx.x) * kScanItems;
    int item[kScanItems];
    int v = 0;
#pragma unroll
    for (int i = 0; i < kScanItems; i++) {
        item[i] = at + i < n ? counts[at + i] : 0;
        v += item[i];
    }
    int total = 0;
    int run = sums[blockIdx.x] + block_scan(v, lds, &total) - v;
#pragma unroll
    for (int i = 0; i < kScanItems; i++) {
        if (at + i < n) {
            cursor[at + i] = run;
            run += item[i];
            counts[at + i] = run;
        }
    }
}

// ---- candidates ----------------------------------------------------------------------------------------------------------------
struct SeedArgs {
    Geometry g;
    const int32_t *offsets, *positions;
    int q;
    const unsigned char *reads;      // ASCII rows, stride n + 1
    int n;
    int64_t n_reads;
    int bound, step, strands;
    int64_t cap;
    const int32_t *lens;             // the *_lens calls: every read's own length (n is then the rows' width), else NULL
};

__device__ __forceinline__ uint32_t map_char(uint32_t ch)   // the subject preprocess's classes (preprocess.hip)
{
    return ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : ch == 'N' ? 4u : 0u;
}

// Class of character i of the read (strand 0) or of its reverse complement (strand 1).
__device__ __forceinline__ uint32_t strand_class(const unsigned char *row, int n, int strand, int i)
{
    const uint32_t c = map_char(strand ? row[n - 1 - i] : row[i]);
    return strand && c < 4u ? 3u - c : c;
}

// The windows w with lo <= start(w) <= hi, as a range [*w_lo, *w_hi] of the regular windows (start w * S, w <= n_windows - 2)
// and whether the anchored last one joins them.  Returns their number.
__device__ __forceinline__ int candidate_windows(const Geometry &g, int64_t lo, int64_t hi, int64_t *w_lo, int64_t *w_hi, bool *last)
{
    if (lo < 0) lo = 0;
    *last = lo <= g.last_start && g.last_start <= hi;
    *w_lo = (lo + g.stride - 1) / g.stride;
    *w_hi = hi < 0 ? -1 : hi / g.stride;
    if (*w_hi > g.n_windows - 2) *w_hi = g.n_windows - 2;
    const int64_t regular = *w_hi >= *w_lo ? *w_hi - *w_lo + 1 : 0;
    return static_cast<int>(regular) + (*last ? 1 : 0);
}

// Emit == false: counts[r] = the read's candidates, -1 (an N in a piece) or -2 (above the cap).  Emit == true: a read with a
// non-negative count writes its candidates from prefix[r] on.
// Lens == true: read r is its row's first n_r = lens[r] characters (clamped to [0, a.n]) with B_r = min(a.bound, n_r) and step_r =
// n_r / (B_r + 1); step_r < q (n_r == 0 among them) is flag -3 and nothing of the row is read.  Every piece ends at or before
// (B_r + 1) * step_r <= n_r, and the reverse strand counts back from n_r - 1: the pad behind a read's end is never looked at.
template <bool Emit, bool Lens>
__global__ __launch_bounds__(256) void seed_candidates_kernel(SeedArgs a, int32_t *__restrict__ counts, const int64_t *__restrict__ prefix,
                                                              int64_t read_base, int32_t *__restrict__ out_read,
                                                              int32_t *__restrict__ out_window)
{
    const int64_t r = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (r >= a.n_reads) return;
    const unsigned char *row = a.reads + r * (a.n + 1);
    int64_t at = 0;
    if (Emit && counts[r] < 0) return;
    int n = a.n, B = a.bound, step = a.step;
    if (Lens) {
        n = a.lens[r];
        n = n < 0 ? 0 : n > a.n ? a.n : n;
        B = a.bound < n ? a.bound : n;
        step = n / (B + 1);
        if (step < a.q) {                         // too short for this seed and bound (n == 0: step 0)
            if (!Emit) counts[r] = -3;
            return;
        }
    }
    if (Emit) {
        at = prefix[r];
    } else {
        for (int s = 0; s < a.strands; s++)
            for (int j = 0; j <= B; j++)
                for (int t = 0; t < a.q; t++)
                    if (strand_class(row, n, s, j * step + t) == 4u) {
                        counts[r] = -1;
                        return;
                    }
    }
    const int W = a.g.window_len, q = a.q;
    int64_t count = 0;
    for (int s = 0; s < a.strands; s++) {
        for (int j = 0; j <= B; j++) {
            const int o = j * step;
            uint32_t code = 0;
            for (int t = 0; t < q; t++) code = (code << 2) | (strand_class(row, n, s, o + t) & 3u);
            const int32_t end = a.offsets[code + 1];
            for (int32_t i = a.offsets[code]; i < end; i++) {
                const int64_t p = a.positions[i];
                const int64_t d = p - o;                                 // the diagonal: where the read's first base would lie
                const int64_t lo_a = p + q - W, lo_b = d + n - B - W;
                const int64_t hi_b = d + B;
                int64_t w_lo = 0, w_hi = -1;
                bool last = false;
                const int found = candidate_windows(a.g, lo_a > lo_b ? lo_a : lo_b, p < hi_b ? p : hi_b, &w_lo, &w_hi, &last);
                if (Emit) {
                    const int32_t id_base = static_cast<int32_t>(s * a.g.n_windows);
                    for (int64_t w = w_lo; w <= w_hi; w++) {
                        out_read[at] = static_cast<int32_t>(read_base + r);
                        out_window[at++] = id_base + static_cast<int32_t>(w);
                    }
                    if (last) {
                        out_read[at] = static_cast<int32_t>(read_base + r);
                        out_window[at++] = id_base + static_cast<int32_t>(a.g.n_windows - 1);
                    }
                } else {
                    count += found;
                    if (count > a.cap) {
                        counts[r] = -2;
                        return;
                    }
                }
            }
        }
    }
    if (!Emit) counts[r] = static_cast<int32_t>(count);
}

// ---- verify --------------------------------------------------------------------------------------------------------------------
struct VerifyArgs {
    const unsigned char *reference;
    Geometry g;
    const uint32_t *peq;
    int read_len;
    int64_t read_count;
    int word_num;
    const int32_t *pair_window;
    const int64_t *pair_subject;
    int64_t n_pairs, subject_base;
    const int32_t *read_lens;        // the *_lens call: one length per column of the bucket, else NULL
    int32_t *distance;
    unsigned char *workspace;        // [wave][block of 32 rows][Hp | Hn | add][lane] uint32: only for word_num > kVerifyWords
    size_t wave_bytes;
};

size_t verify_wave_bytes(int window_len, int word_num)
{
    if (word_num <= kVerifyWords) return 0;
    return static_cast<size_t>((window_len + kVerifyRows - 1) / kVerifyRows) * 3 * kLanes * sizeof(uint32_t);
}

// The characters of rows i0 .. i0 + rows - 1 (rows <= 32) of the window that starts at reference offset `at`, four bits each:
// row i0 + r in bits [4r, 4r + 4) of *lo (r < 16) or *hi.  The 32 bytes [span, span + 32) of the reference hold the block —
// forward row r at span + r, reverse row r at span + 31 - r, complemented — and are fetched as the nine ALIGNED dwords that
// cover them, funnel-shifted by the span's misalignment: a lane loads 9 dwords, not 32 bytes.  A dword is loaded only where it
// holds a byte some row needs, so a load never leaves the 4-byte line of a window byte (and with it never that byte's page);
// what the rows beyond `rows` would hold is never run.  Codes are 0..4 (a mapped reference); the low three bits are taken.
__device__ __forceinline__ void window_block(const unsigned char *reference, int64_t at, int m, bool reverse, int i0, int rows,
                                             unsigned long long *lo, unsigned long long *hi)
{
    const int64_t span = reverse ? at + m - kVerifyRows - i0 : at + i0;
    const int64_t need_lo = reverse ? span + kVerifyRows - rows : span, need_hi = reverse ? span + kVerifyRows - 1 : span + rows - 1;
    const uintptr_t address = reinterpret_cast<uintptr_t>(reference) + static_cast<uintptr_t>(span);
    const unsigned skew = static_cast<unsigned>(address & 3u);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(address - skew);
    uint32_t d[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const int64_t o = span - skew + 4 * k;          // dword k holds the reference offsets [o, o + 4)
        d[k] = o + 3 >= need_lo && o <= need_hi ? src[k] : 0u;
    }
    uint32_t nib[8];                                    // 4 characters each, in address order
#pragma unroll
    for (int k = 0; k < 8; k++) {
        uint32_t x = __builtin_amdgcn_alignbyte(d[k + 1], d[k], skew) & 0x07070707u;
        x = (x | (x >> 4)) & 0x00ff00ffu;
        nib[k] = (x | (x >> 8)) & 0xffffu;
    }
    unsigned long long l = nib[0] | (nib[1] << 16) | (static_cast<unsigned long long>(nib[2] | (nib[3] << 16)) << 32);
    unsigned long long h = nib[4] | (nib[5] << 16) | (static_cast<unsigned long long>(nib[6] | (nib[7] << 16)) << 32);
    if (reverse) {                                      // row r is character 31 - r: the nibbles in reverse order, complemented
        auto flip = [](unsigned long long v) {
            v = ((v >> 4) & 0x0f0f0f0f0f0f0f0full) | ((v & 0x0f0f0f0f0f0f0f0full) << 4);
            v = __builtin_bswap64(v);
            return v ^ (((~v >> 2) & 0x1111111111111111ull) * 3u);   // 3 - c below 4, 4 stays 4
        };
        const unsigned long long t = flip(h);
        h = flip(l);
        l = t;
    }
    *lo = l;
    *hi = h;
}

// WB words per column block; Blocks == false: the read is one block (word_num <= WB), no carries leave the registers.
// Lens == true: lane p verifies its column's first n = read_lens[col] characters (clamped to [0, read_len]).  The planes stay
// where the bucket's preprocess put them; the lane takes its score column from its OWN word (n - 1) >> 5 at bit (n - 1) & 31 —
// a compare (hoisted out of the row loop) and two selects per word and row.  Carries and shifts travel upward only, so the
// columns above n (the pad, and with column blocks every later block) are computed and never looked at; the block that holds
// the lane's word sees every row, so `run` and `best` are complete when that block ends.  n == 0: distance 0.
template <int WB, bool Blocks, bool Lens>
__global__ __launch_bounds__(kLanes) void reference_verify_pairs_kernel(VerifyArgs a, int64_t first)
{
    const int lane = threadIdx.x;
    const int64_t p = first + static_cast<int64_t>(blockIdx.x) * kLanes + lane;
    if (p >= a.n_pairs) return;
    const int64_t s = a.pair_subject[p];
    if (s < a.subject_base ||
        static_cast<unsigned long long>(s) - static_cast<unsigned long long>(a.subject_base) >= static_cast<unsigned long long>(a.read_count))
        return;                                   // another bucket's pair, or the unused slot -1
    const int64_t id = a.pair_window[p];
    if (id < 0 || id >= 2 * a.g.n_windows) return;   // no window: the id forms no address
    const int64_t col = s - a.subject_base;
    const int wn = a.word_num, m = a.g.window_len;
    int n = a.read_len;
    if (Lens) {
        n = a.read_lens[col];
        n = n < 0 ? 0 : n > a.read_len ? a.read_len : n;
        if (n == 0) {
            a.distance[p] = 0;
            return;
        }
    }
    const bool reverse = id >= a.g.n_windows;
    const int64_t at = window_start(a.g, reverse ? id - a.g.n_windows : id);

    const uint32_t *planes = a.peq + static_cast<size_t>(col >> 6) * kChars * wn * kLanes + (col & (kLanes - 1));
    uint32_t *carries = Blocks ? reinterpret_cast<uint32_t *>(a.workspace + static_cast<size_t>(blockIdx.x) * a.wave_bytes) + lane : nullptr;
    const int top = (n - 1) & 31;   // column n inside the last word (Lens: inside the lane's own word)
    const int own = Lens ? (n - 1) >> 5 : 0;

    int run = n, best = n;
    for (int w0 = 0; w0 < (Blocks ? wn : 1); w0 += WB) {
        const int wb = wn - w0 < WB ? wn - w0 : WB;   // wave-uniform
        const bool leftmost = w0 == 0, rightmost = !Blocks || w0 + WB >= wn;
        const int own_w = own - w0;                   // Lens: the lane's word inside this block, or outside [0, WB)
        uint32_t peq[kChars][WB], pv[WB], mv[WB];
#pragma unroll
        for (int w = 0; w < WB; w++) {
#pragma unroll
            for (int c = 0; c < kChars; c++) peq[c][w] = w < wb ? planes[(static_cast<size_t>(c) * wn + w0 + w) * kLanes] : 0u;
            pv[w] = ~0u;
            mv[w] = 0u;
        }
        for (int i0 = 0; i0 < m; i0 += kVerifyRows) {
            const int rows = m - i0 < kVerifyRows ? m - i0 : kVerifyRows;
            uint32_t in_hp = 0, in_hn = 0, in_add = 0;
            uint32_t *cw = nullptr;
            if (Blocks) {
                cw = carries + static_cast<size_t>(i0 >> 5) * 3 * kLanes;
                if (!leftmost) {
                    in_hp = cw[0];
                    in_hn = cw[kLanes];
                    in_add = cw[2 * kLanes];
                }
            }
            unsigned long long lo = 0, hi = 0;          // the block's characters, four bits each, every load at the block's head
            window_block(a.reference, at, m, reverse, i0, rows, &lo, &hi);
            uint32_t out_hp = 0, out_hn = 0, out_add = 0;
#pragma unroll 1
            for (int r = 0; r < rows; r++) {
                const ClassMasks k = class_masks<true>(next_class(lo, hi));
                uint32_t carry = (in_add >> r) & 1u, hp_in = (in_hp >> r) & 1u, hn_in = (in_hn >> r) & 1u;
                uint32_t top_hp = 0, top_hn = 0;
#pragma unroll
                for (int w = 0; w < WB; w++) {
                    if (w < wb) {
                        const MyersWord s = myers_word(class_eq(peq, w, k), pv[w], mv[w], carry, hp_in, hn_in);
                        if (Lens) {
                            top_hp = w == own_w ? s.hp : top_hp;
                            top_hn = w == own_w ? s.hn : top_hn;
                        } else {
                            top_hp = s.hp;
                            top_hn = s.hn;
                        }
                    }
                }
                if (Blocks) {
                    out_hp |= hp_in << r;
                    out_hn |= hn_in << r;
                    out_add |= carry << r;
                }
                if (Lens || rightmost) {             // Lens: a block without the lane's word adds 0
                    run += static_cast<int>((top_hp >> top) & 1u) - static_cast<int>((top_hn >> top) & 1u);
                    best = run < best ? run : best;
                }
            }
            if (Blocks && !rightmost) {
                cw[0] = out_hp;
                cw[kLanes] = out_hn;
                cw[2 * kLanes] = out_add;
            }
        }
    }
    a.distance[p] = best;
}

template <int WB, bool Blocks>
int launch_verify(const VerifyArgs &a, dim3 grid, int64_t first, hipStream_t stream)
{
    if (a.read_lens) hipLaunchKernelGGL((reference_verify_pairs_kernel<WB, Blocks, true>), grid, dim3(kLanes), 0, stream, a, first);
    else hipLaunchKernelGGL((reference_verify_pairs_kernel<WB, Blocks, false>), grid, dim3(kLanes), 0, stream, a, first);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

// ---- which instance verifies a read of wn words: decided here, once; dispatch_verify launches the answer,
// verify_kernel_name formats it ----
template <int WB, bool Blocks>
struct VerifyWidth {
    static constexpr int words = WB;
    static constexpr bool blocks = Blocks;
};

// The narrowest instance that holds the read in one block; column blocks of kVerifyWords beyond that.
template <typename F>
int verify_select(int wn, F &&f)
{
    if (wn > kVerifyWords) return f(VerifyWidth<kVerifyWords, true>{});
    if (wn <= 1) return f(VerifyWidth<1, false>{});
    if (wn <= 2) return f(VerifyWidth<2, false>{});
    if (wn <= 3) return f(VerifyWidth<3, false>{});
    if (wn <= 4) return f(VerifyWidth<4, false>{});
    if (wn <= 5) return f(VerifyWidth<5, false>{});
    if (wn <= 6) return f(VerifyWidth<6, false>{});
    if (wn <= 8) return f(VerifyWidth<8, false>{});
    if (wn <= 12) return f(VerifyWidth<12, false>{});
    return f(VerifyWidth<16, false>{});
}

int dispatch_verify(const VerifyArgs &a, dim3 grid, int64_t first, hipStream_t stream)
{
    return verify_select(a.word_num, [&](auto w) { return launch_verify<decltype(w)::words, decltype(w)::blocks>(a, grid, first, stream); });
}

const char *verify_kernel_name(int word_num, bool lens)
{
    static thread_local char name[64];
    verify_select(word_num, [&](auto w) {
        return snprintf(name, sizeof name, "reference_verify_pairs_kernel<%d, %s, %s>", decltype(w)::words,
                        decltype(w)::blocks ? "true" : "false", lens ? "true" : "false");
    });
    return name;
}

// ---- select --------------------------------------------------------------------------------------------------------------------
// One wave per read.  The read's candidates are cand[seg[r] .. seg[r + 1]), ids ascending and distinct; round t takes the
// smallest key (distance << 32 | id) above the one round t - 1 took, among the candidates within the bound.
__global__ __launch_bounds__(256) void seed_select_kernel(const int32_t *__restrict__ cand_window, const int32_t *__restrict__ cand_distance,
                                                          const int64_t *__restrict__ segments, int64_t n_reads, int bound, int k,
                                                          int32_t *__restrict__ hit_scores, int32_t *__restrict__ hit_windows)
{
    const int lane = threadIdx.x & (kLanes - 1);
    const int64_t read = static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (read >= n_reads) return;     // wave-uniform
    const int64_t lo = segments[read], hi = segments[read + 1];
    const unsigned long long none = ~0ull;
    unsigned long long last = 0;
    bool any = false, done = false;  // any: `last` is a key already taken
    for (int t = 0; t < k; t++) {    // k is wave-uniform
        unsigned long long mine = none;
        if (!done) {
            for (int64_t i = lo + lane; i < hi; i += kLanes) {
                const int d = cand_distance[i];
                if (d < 0 || d > bound) continue;
                const unsigned long long key = (static_cast<unsigned long long>(d) << 32) | static_cast<uint32_t>(cand_window[i]);
                if ((!any || key > last) && key < mine) mine = key;
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const unsigned long long other = __shfl_xor(mine, off);
                mine = other < mine ? other : mine;
            }
            if (mine == none) done = true;
        }
        if (lane == 0) {
            hit_scores[read * k + t] = mine == none ? INT32_MIN : -static_cast<int32_t>(mine >> 32);
            hit_windows[read * k + t] = mine == none ? -1 : static_cast<int32_t>(mine & 0xffffffffu);
        }
        last = mine;
        any = true;
    }
}

// ---- checks ----------------------------------------------------------------------------------------------------------------------
// The shape of reference_windows.hip's calls, with index positions and window ids in int32.  0, or the error with its text set.
int seed_geometry(const char *who, int64_t ref_len, int window_len, int stride, Geometry *out)
{
    if (ref_len > static_cast<int64_t>(INT32_MAX)) return refuse(who, BGSA_HIP_EINVAL, "ref_len beyond 2^31 - 1 (index positions are int32)");
    if (int rc = make_geometry(who, ref_len, window_len, stride, out)) return rc;
    if (2 * out->n_windows > static_cast<int64_t>(INT32_MAX))
        return refuse(who, BGSA_HIP_EINVAL, "the windows on two strands do not fit int32 window ids");
    return BGSA_HIP_OK;
}

bool seed_len_ok(int seed_len) { return seed_len >= 1 && seed_len <= kSeedMaxLen; }
int64_t seed_codes(int seed_len) { return static_cast<int64_t>(1) << (2 * seed_len); }
int64_t scan_blocks(int seed_len) { return (seed_codes(seed_len) + kScanBlock - 1) / kScanBlock; }

unsigned grid_of(int64_t threads)
{
    const int64_t blocks = (threads + 255) / 256;
    return static_cast<unsigned>(blocks < kMaxBlocks ? blocks : kMaxBlocks);
}

}  // namespace

}  // namespace bgsa

using namespace bgsa;

extern "C" {

int64_t bgsa_hip_seed_index_offsets(int seed_len)
{
    if (!seed_len_ok(seed_len)) {
        refuse("seed_index_offsets", BGSA_HIP_EINVAL, "seed_len must lie in 1..13");
        return -1;
    }
    return seed_codes(seed_len) + 1;
}

size_t bgsa_hip_seed_index_workspace_bytes(int64_t ref_len, int seed_len)
{
    if (!seed_len_ok(seed_len) || ref_len < 0 || ref_len > static_cast<int64_t>(INT32_MAX)) return 0;
    return static_cast<size_t>(seed_codes(seed_len) + scan_blocks(seed_len)) * sizeof(int32_t);   // the cursors, then the block sums
}

int bgsa_hip_seed_index_build_dev(const char *d_reference, int64_t ref_len, int seed_len, int32_t *d_offsets, int32_t *d_positions,
                                  void *d_workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "seed_index_build_dev";
    if (!d_reference || !d_offsets || !d_positions || !d_workspace)
        return refuse(who, BGSA_HIP_EINVAL, "a NULL pointer (only the stream may be NULL)");
    if (!seed_len_ok(seed_len)) return refuse(who, BGSA_HIP_EINVAL, "seed_len must lie in 1..13");
    if (ref_len < 0) return refuse(who, BGSA_HIP_EINVAL, "ref_len is negative");
    if (ref_len > static_cast<int64_t>(INT32_MAX)) return refuse(who, BGSA_HIP_EINVAL, "ref_len beyond 2^31 - 1 (index positions are int32)");
    if (workspace_bytes < bgsa_hip_seed_index_workspace_bytes(ref_len, seed_len))
        return refuse(who, BGSA_HIP_EINVAL, "workspace smaller than bgsa_hip_seed_index_workspace_bytes()");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t codes = seed_codes(seed_len), blocks = scan_blocks(seed_len);
    BGSA_HIP_TRY(hipMemsetAsync(d_offsets, 0, static_cast<size_t>(codes + 1) * sizeof(int32_t), s));
    if (ref_len < seed_len) return BGSA_HIP_OK;   // no k-mer: every bucket is empty
    int32_t *cursor = static_cast<int32_t *>(d_workspace), *sums = cursor + codes;
    const unsigned char *ref = reinterpret_cast<const unsigned char *>(d_reference);
    const unsigned walk = grid_of((ref_len - seed_len + 1 + kSeedChunk - 1) / kSeedChunk);
    hipLaunchKernelGGL(seed_index_walk_kernel<false>, dim3(walk), dim3(256), 0, s, ref, ref_len, seed_len, d_offsets, nullptr);
    BGSA_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(seed_scan_sums_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, d_offsets + 1, codes, sums);
    BGSA_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(seed_scan_bases_kernel, dim3(1), dim3(256), 0, s, sums, blocks);
    BGSA_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(seed_scan_apply_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, s, d_offsets + 1, codes, sums, cursor);
    BGSA_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(seed_index_walk_kernel<true>, dim3(walk), dim3(256), 0, s, ref, ref_len, seed_len, cursor, d_positions);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

// per_read: the *_lens calls — d_read_lens is required, and step < seed_len is every read's own flag -3, not a refusal.
static int seed_args(const char *who, int64_t ref_len, int window_len, int stride, const int32_t *d_offsets, const int32_t *d_positions,
                     int seed_len, const char *d_reads, int read_len, int64_t n_reads, int max_distance, int both_strands, SeedArgs *out,
                     bool per_read = false, const int32_t *d_read_lens = nullptr)
{
    if (!d_offsets || !d_positions || !d_reads || (per_read && !d_read_lens)) return refuse(who, BGSA_HIP_EINVAL, "a NULL pointer (only the stream may be NULL)");
    if (!seed_len_ok(seed_len)) return refuse(who, BGSA_HIP_EINVAL, "seed_len must lie in 1..13");
    Geometry g;
    if (int rc = seed_geometry(who, ref_len, window_len, stride, &g)) return rc;
    if (read_len < 1 || max_distance < 0) return refuse(who, BGSA_HIP_EINVAL, "read_len must be positive and max_distance not negative");
    if (n_reads < 0 || n_reads > static_cast<int64_t>(INT32_MAX)) return refuse(who, BGSA_HIP_EINVAL, "n_reads must lie in [0, 2^31 - 1]");
    const int bound = max_distance < read_len ? max_distance : read_len;
    const int step = read_len / (bound + 1);
    if (!per_read && step < seed_len) {
        char why[200];
        snprintf(why, sizeof why, "the %d pieces of a %d bp read within distance %d are %d bp apart, shorter than seed_len %d", bound + 1,
                 read_len, bound, step, seed_len);
        return refuse(who, BGSA_HIP_EINVAL, why);
    }
    *out = SeedArgs{g, d_offsets, d_positions, seed_len, reinterpret_cast<const unsigned char *>(d_reads), read_len, n_reads, bound, step,
                    both_strands ? 2 : 1, 0, per_read ? d_read_lens : nullptr};
    return BGSA_HIP_OK;
}

static int count_candidates(const char *who, int64_t ref_len, int window_len, int stride, const int32_t *d_offsets,
                            const int32_t *d_positions, int seed_len, const char *d_reads, const int32_t *d_read_lens, bool per_read,
                            int read_len, int64_t n_reads, int max_distance, int both_strands, int64_t max_candidates, int32_t *d_counts,
                            void *stream)
{
    SeedArgs a;
    if (!d_counts) return refuse(who, BGSA_HIP_EINVAL, "a NULL pointer (only the stream may be NULL)");
    if (int rc = seed_args(who, ref_len, window_len, stride, d_offsets, d_positions, seed_len, d_reads, read_len, n_reads, max_distance,
                           both_strands, &a, per_read, d_read_lens))
        return rc;
    if (max_candidates < 0) return refuse(who, BGSA_HIP_EINVAL, "max_candidates is negative");
    a.cap = max_candidates < (1ll << 30) ? max_candidates : (1ll << 30);   // a count stays an int32
    if (n_reads == 0) return BGSA_HIP_OK;
    const dim3 grid(static_cast<unsigned>((n_reads + 255) / 256));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (per_read) hipLaunchKernelGGL((seed_candidates_kernel<false, true>), grid, dim3(256), 0, s, a, d_counts, nullptr, 0, nullptr, nullptr);
    else hipLaunchKernelGGL((seed_candidates_kernel<false, false>), grid, dim3(256), 0, s, a, d_counts, nullptr, 0, nullptr, nullptr);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

static int emit_candidates(const char *who, int64_t ref_len, int window_len, int stride, const int32_t *d_offsets,
                           const int32_t *d_positions, int seed_len, const char *d_reads, const int32_t *d_read_lens, bool per_read,
                           int read_len, int64_t n_reads, int max_distance, int both_strands, const int32_t *d_counts,
                           const int64_t *d_prefix, int64_t read_base, int32_t *d_cand_read, int32_t *d_cand_window, void *stream)
{
    SeedArgs a;
    if (!d_counts || !d_prefix || !d_cand_read || !d_cand_window)
        return refuse(who, BGSA_HIP_EINVAL, "a NULL pointer (only the stream may be NULL)");
    if (int rc = seed_args(who, ref_len, window_len, stride, d_offsets, d_positions, seed_len, d_reads, read_len, n_reads, max_distance,
                           both_strands, &a, per_read, d_read_lens))
        return rc;
    if (read_base < 0 || read_base > static_cast<int64_t>(INT32_MAX) - n_reads)
        return refuse(who, BGSA_HIP_EINVAL, "read_base + n_reads must stay within int32");
    if (n_reads == 0) return BGSA_HIP_OK;
    const dim3 grid(static_cast<unsigned>((n_reads + 255) / 256));
    hipStream_t s = static_cast<hipStream_t>(stream);
    int32_t *counts = const_cast<int32_t *>(d_counts);
    if (per_read)
        hipLaunchKernelGGL((seed_candidates_kernel<true, true>), grid, dim3(256), 0, s, a, counts, d_prefix, read_base, d_cand_read, d_cand_window);
    else
        hipLaunchKernelGGL((seed_candidates_kernel<true, false>), grid, dim3(256), 0, s, a, counts, d_prefix, read_base, d_cand_read, d_cand_window);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

int bgsa_hip_seed_count_candidates_dev(int64_t ref_len, int window_len, int stride, const int32_t *d_offsets, const int32_t *d_positions,
                                       int seed_len, const char *d_reads, int read_len, int64_t n_reads, int max_distance,
                                       int both_strands, int64_t max_candidates, int32_t *d_counts, void *stream)
{
    return count_candidates("seed_count_candidates_dev", ref_len, window_len, stride, d_offsets, d_positions, seed_len, d_reads, nullptr, false,
                            read_len, n_reads, max_distance, both_strands, max_candidates, d_counts, stream);
}

int bgsa_hip_seed_count_candidates_lens_dev(int64_t ref_len, int window_len, int stride, const int32_t *d_offsets,
                                            const int32_t *d_positions, int seed_len, const char *d_reads, const int32_t *d_read_lens,
                                            int read_len, int64_t n_reads, int max_distance, int both_strands, int64_t max_candidates,
                                            int32_t *d_counts, void *stream)
{
    return count_candidates("seed_count_candidates_lens_dev", ref_len, window_len, stride, d_offsets, d_positions, seed_len, d_reads,
                            d_read_lens, true, read_len, n_reads, max_distance, both_strands, max_candidates, d_counts, stream);
}

int bgsa_hip_seed_emit_candidates_dev(int64_t ref_len, int window_len, int stride, const int32_t *d_offsets, const int32_t *d_positions,
                                      int seed_len, const char *d_reads, int read_len, int64_t n_reads, int max_distance,
                                      int both_strands, const int32_t *d_counts, const int64_t *d_prefix, int64_t read_base,
                                      int32_t *d_cand_read, int32_t *d_cand_window, void *stream)
{
    return emit_candidates("seed_emit_candidates_dev", ref_len, window_len, stride, d_offsets, d_positions, seed_len, d_reads, nullptr, false,
                           read_len, n_reads, max_distance, both_strands, d_counts, d_prefix, read_base, d_cand_read, d_cand_window, stream);
}

int bgsa_hip_seed_emit_candidates_lens_dev(int64_t ref_len, int window_len, int stride, const int32_t *d_offsets,
                                           const int32_t *d_positions, int seed_len, const char *d_reads, const int32_t *d_read_lens,
                                           int read_len, int64_t n_reads, int max_distance, int both_strands, const int32_t *d_counts,
                                           const int64_t *d_prefix, int64_t read_base, int32_t *d_cand_read, int32_t *d_cand_window,
                                           void *stream)
{
    return emit_candidates("seed_emit_candidates_lens_dev", ref_len, window_len, stride, d_offsets, d_positions, seed_len, d_reads,
                           d_read_lens, true, read_len, n_reads, max_distance, both_strands, d_counts, d_prefix, read_base, d_cand_read,
                           d_cand_window, stream);
}

size_t bgsa_hip_reference_verify_workspace_bytes(int window_len, int read_len, int64_t n_pairs)
{
    if (window_len < 1 || read_len < 1 || n_pairs < 0) return 0;
    const size_t per = verify_wave_bytes(window_len, (read_len + 31) / 32);
    return per ? pair_workspace_for(per, n_pairs) : 0;
}

const char *bgsa_hip_reference_verify_kernel_name(int word_num, int lens) { return verify_kernel_name(word_num, lens != 0); }

// per_lane: the *_lens call — d_read_lens is required and every lane verifies at its own length.
static int verify_pairs(const char *who, const char *d_reference, int64_t ref_len, int window_len, int stride, const hip_read_t *d_peq,
                        const int32_t *d_read_lens, bool per_lane, int read_len, int64_t read_count, int word_num,
                        const int32_t *d_pair_window, const int64_t *d_pair_subject, int64_t n_pairs, int64_t subject_base,
                        int32_t *d_distance, void *d_workspace, size_t workspace_bytes, void *stream)
{
    if (!d_reference || !d_peq || !d_pair_window || !d_pair_subject || !d_distance || (per_lane && !d_read_lens))
        return refuse(who, BGSA_HIP_EINVAL, "a NULL pointer (only the workspace of a read of <= 16 words and the stream may be NULL)");
    Geometry g;
    if (int rc = seed_geometry(who, ref_len, window_len, stride, &g)) return rc;
    if (n_pairs < 0) return refuse(who, BGSA_HIP_EINVAL, "n_pairs is negative");
    if (read_len < 1) return refuse(who, BGSA_HIP_EINVAL, "read_len is not positive");
    if (read_count <= 0 || read_count % HIP_V_NUM != 0) return refuse(who, BGSA_HIP_EINVAL, "read_count must be a positive multiple of 64");
    if (word_num < 1 || word_num != (read_len + 31) / 32)
        return refuse(who, BGSA_HIP_EINVAL, "word_num is not bgsa_hip_word_num(BGSA_ALGO_MYERS, ...) = ceil(read_len / 32)");
    if (word_num > kVerifyMaxWords) return refuse(who, BGSA_HIP_EUNSUPPORTED, "reads beyond 1,024 bp (word_num > 32) have no verify kernel");
    const size_t per = verify_wave_bytes(window_len, word_num);
    if (per && (!d_workspace || workspace_bytes < per))
        return refuse(who, BGSA_HIP_EINVAL, "a read beyond 16 words needs a workspace of bgsa_hip_reference_verify_workspace_bytes()");
    if (n_pairs == 0) return BGSA_HIP_OK;

    VerifyArgs a{reinterpret_cast<const unsigned char *>(d_reference), g, d_peq, read_len, read_count, word_num, d_pair_window,
                 d_pair_subject, n_pairs, subject_base, per_lane ? d_read_lens : nullptr, d_distance, static_cast<unsigned char *>(d_workspace), per};
    return for_each_chunk(n_pairs, per, workspace_bytes,
                          [&](dim3 grid, int64_t first) { return dispatch_verify(a, grid, first, static_cast<hipStream_t>(stream)); });
}

int bgsa_hip_reference_verify_pairs_dev(const char *d_reference, int64_t ref_len, int window_len, int stride, const hip_read_t *d_peq,
                                        int read_len, int64_t read_count, int word_num, const int32_t *d_pair_window,
                                        const int64_t *d_pair_subject, int64_t n_pairs, int64_t subject_base, int32_t *d_distance,
                                        void *d_workspace, size_t workspace_bytes, void *stream)
{
    return verify_pairs("reference_verify_pairs_dev", d_reference, ref_len, window_len, stride, d_peq, nullptr, false, read_len, read_count,
                        word_num, d_pair_window, d_pair_subject, n_pairs, subject_base, d_distance, d_workspace, workspace_bytes, stream);
}

int bgsa_hip_reference_verify_pairs_lens_dev(const char *d_reference, int64_t ref_len, int window_len, int stride, const hip_read_t *d_peq,
                                             const int32_t *d_read_lens, int read_len, int64_t read_count, int word_num,
                                             const int32_t *d_pair_window, const int64_t *d_pair_subject, int64_t n_pairs,
                                             int64_t subject_base, int32_t *d_distance, void *d_workspace, size_t workspace_bytes,
                                             void *stream)
{
    return verify_pairs("reference_verify_pairs_lens_dev", d_reference, ref_len, window_len, stride, d_peq, d_read_lens, true, read_len,
                        read_count, word_num, d_pair_window, d_pair_subject, n_pairs, subject_base, d_distance, d_workspace, workspace_bytes,
                        stream);
}

int bgsa_hip_seed_select_dev(const int32_t *d_cand_window, const int32_t *d_cand_distance, const int64_t *d_segments, int64_t n_reads,
                             int max_distance, int k, int32_t *d_hit_scores, int32_t *d_hit_windows, void *stream)
{
    const char *who = "seed_select_dev";
    if (!d_segments || !d_hit_scores || !d_hit_windows) return refuse(who, BGSA_HIP_EINVAL, "the segments or an output is NULL");
    if (k < 1 || k > HIP_V_NUM) return refuse(who, BGSA_HIP_EINVAL, "k must lie in 1..64");
    if (max_distance < 0) return refuse(who, BGSA_HIP_EINVAL, "max_distance is negative");
    if (n_reads < 0 || n_reads > static_cast<int64_t>(INT32_MAX) * kWavesPerBlock)
        return refuse(who, BGSA_HIP_EINVAL, "n_reads is negative or beyond one launch");
    if (n_reads == 0) return BGSA_HIP_OK;
    hipLaunchKernelGGL(seed_select_kernel, dim3(static_cast<unsigned>((n_reads + kWavesPerBlock - 1) / kWavesPerBlock)),
                       dim3(kWavesPerBlock * kLanes), 0, static_cast<hipStream_t>(stream), d_cand_window, d_cand_distance, d_segments, n_reads,
                       max_distance, k, d_hit_scores, d_hit_windows);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

}  // extern "C"
