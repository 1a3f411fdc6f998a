// myers_global.hip — Myers unit-cost global alignment, one subject per lane, gfx950.
//
// Replaces the reference's align_cpu / align_sse hot loop (original/BGSA_CPU/align_core.c:54-146,
// original/BGSA_SSE/align_core.c:55-150) and its OpenMP grid (cal_cpu.c:66-84).
//
// Mapping to the machine
//   * lane  = one subject; a wavefront = one "group" of HIP_V_NUM = 64 subjects, which is exactly
//     the reference's SIMD-lane layout [group][char][word][lane] widened from 4/8/16 to 64 lanes.
//   * The subject's match masks stay in VGPRs for the whole task; a task scores a tile of
//     queries against the group, so each Peq block is read from HBM once per tile.
//   * The query character is wave-uniform: it is fetched through the scalar cache and selects
//     one of five copies of the row body by a scalar jump, so `Eq = Peq[c][w]` costs no VALU
//     work (the reference pays a pointer add + a vector load per word, align_core.c:67,74).
//   * Words are full 32-bit (the reference keeps bit W-1 free as a software carry,
//     align_core.c:79-83,91-96): the addition and the 1-bit shift of HP are add-with-carry chains
//     through VCC; HN needs no shift — it is read off the addition's carries (rows_ir.py: myers_body).
//   * The score is not tracked per row (align_core.c:121-124); after the last row
//     D[m][n] = m + popcount(VP & mask) - popcount(VN & mask), two v_bcnt per word.
//
// The kernels, chosen by myers_select() (launch_myers switches on its answer, myers_kernel_name formats it):
//   myers_global_asm_kernel<NW,1>   1..1024 bp   generated asm row loop, Peq planes resident, 8 VALU per (row, word); 30 and 32 words
//                                                (897..1024 bp) with the two carry chains in turns over blocks of 9 words
//   myers_global_planes_kernel<NW>  (A/B)        generated asm row loop on 3-bit character-code planes, 9 VALU per (row, word):
//                                                897..1024 bp until round 5, now under BGSA_MYERS_PEQ_MAX_WORDS
//   myers_global_kernel<NW,1>       compiler-scheduled C++ of the same recurrence: the A/B
//                                   reference for the asm (BGSA_MYERS_IMPL=c), 124 vs 216 TCUPS
//   myers_blocked_kernel<NW>        > 1024 bp    column blocks of the planes body, carries between
//                                                blocks through per-wave carry words
//
// Integer/bitwise only; no MFMA, and no LDS but the band kernels' snapshots of a prefix-sharing launch.  The kernels are
// VALU-issue bound.
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "bgsa_common.h"
#include "myers_band.h"

namespace bgsa {

// One DP row: in-place update of the vertical delta vectors for query character class `eq`.
// SEMI (the generator's `-s` for Myers, MyersGenerator.java:56-223): the row boundary feeds 0 instead
// of +1 into word 0 (D[0][i] = 0: the subject may start anywhere in the query) and the horizontal delta
// leaving the last subject column (bit `last_bit` of the last word's HP / HN) is handed back, so the
// caller can follow D[n][i] row by row.
template <int NW, int G, bool SEMI = false>
__device__ __forceinline__ void myers_row(uint32_t (&vp)[G * NW], uint32_t (&vn)[G * NW],
                                          const uint32_t (&eq)[G * NW], int last_word = 0, int last_bit = 0,
                                          int *delta = nullptr)
{
#pragma unroll
  for (int gi = 0; gi < G; gi++) {
    uint32_t hp_prev = 0, hn_prev = 0;
    unsigned carry = 0;
#pragma unroll
    for (int ww = 0; ww < NW; ww++) {
        const int w = gi * NW + ww;
        const uint32_t pv = vp[w], mv = vn[w], e = eq[w];
        const uint32_t pm = e | mv;
        // (pv & pm) == (pv & e) because pv & mv == 0 is an invariant of the recurrence.
        unsigned cout;
        const uint32_t sum = __builtin_addc(pv & e, pv, carry, &cout);
        carry = cout;
        const uint32_t d0 = (sum ^ pv) | pm;
        const uint32_t hp = ~(d0 | pv) | mv;
        const uint32_t hn = d0 & pv;
        // Shift one column along the subject; row boundary D[i][0]-D[i-1][0] = +1 enters word 0.
        const uint32_t hps = (ww == 0) ? ((hp << 1) | (SEMI ? 0u : 1u)) : ((hp << 1) | (hp_prev >> 31));
        const uint32_t hns = (ww == 0) ? (hn << 1) : ((hn << 1) | (hn_prev >> 31));
        hp_prev = hp;
        hn_prev = hn;
        vp[w] = ~(d0 | hps) | hns;
        vn[w] = d0 & hps;
        if (SEMI && ww == last_word)
            delta[gi] = static_cast<int>((hp >> last_bit) & 1u) - static_cast<int>((hn >> last_bit) & 1u);
    }
  }
}

// grid.x = ceil(n_groups / (4*G)), grid.y = number of query tiles; block = 4 waves, each wave
// owns G consecutive groups (G subjects per lane): the scalar work of a row (character fetch,
// 5-way branch) is shared by G x NW word updates.
template <int NW, int G, bool SEMI = false>
__global__ __launch_bounds__(256) void myers_global_kernel(
    const char *__restrict__ content, const uint32_t *__restrict__ peq, int16_t *__restrict__ out,
    int ref_len, int read_len, long long ld, int n_groups, int word_num, int ref_start,
    int ref_end, int q_tile)
{
    const int lane = threadIdx.x & (kLanes - 1);
    const int group0 = __builtin_amdgcn_readfirstlane((blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)) * G);
    if (group0 >= n_groups) return;

    // Peq blocks of this wave's groups: [char][word][lane], coalesced 256-B rows.  A group past
    // the end of the bucket is computed on zero masks and not stored.
    uint32_t P[kChars][G * NW];
#pragma unroll
    for (int gi = 0; gi < G; gi++) {
        const bool live = group0 + gi < n_groups;
        const uint32_t *g = peq + static_cast<size_t>(group0 + gi) * kChars * word_num * kLanes + lane;
#pragma unroll
        for (int c = 0; c < kChars; c++)
#pragma unroll
            for (int w = 0; w < NW; w++)
                P[c][gi * NW + w] = (live && w < word_num) ? g[(c * word_num + w) * kLanes] : 0u;
    }

    const int q0 = ref_start + blockIdx.y * q_tile;
    const int q1 = (q0 + q_tile < ref_end) ? q0 + q_tile : ref_end;
    int16_t *dst = out + static_cast<size_t>(group0) * kLanes + lane;

    for (int q = q0; q < q1; q++) {
        uint32_t vp[G * NW], vn[G * NW];
#pragma unroll
        for (int w = 0; w < G * NW; w++) {
            vp[w] = ~0u;
            vn[w] = 0u;
        }
        UniformBytes qs(content + static_cast<size_t>(q) * (ref_len + 1));
        // semi-global: run[gi] = D[n][i], the subject against the query prefix ending at row i;
        // best = its minimum, starting from D[n][0] = n (genSemiGlobal: score = read_len, min_score = score)
        const int last_word = (read_len - 1) >> 5, last_bit = (read_len - 1) & 31;
        int run[G], best[G], delta[G];
#pragma unroll
        for (int gi = 0; gi < G; gi++) run[gi] = best[gi] = read_len;
        for (int r = 0; r < ref_len; r++) {
            if ((r & 3) == 0) qs.refill(r, ref_len - r);
            const uint32_t c = __builtin_amdgcn_readfirstlane(qs.next());
            switch (c) {
            case 0: myers_row<NW, G, SEMI>(vp, vn, P[0], last_word, last_bit, delta); break;
            case 1: myers_row<NW, G, SEMI>(vp, vn, P[1], last_word, last_bit, delta); break;
            case 2: myers_row<NW, G, SEMI>(vp, vn, P[2], last_word, last_bit, delta); break;
            case 3: myers_row<NW, G, SEMI>(vp, vn, P[3], last_word, last_bit, delta); break;
            default: myers_row<NW, G, SEMI>(vp, vn, P[4], last_word, last_bit, delta); break;
            }
            if (SEMI) {
#pragma unroll
                for (int gi = 0; gi < G; gi++) {
                    run[gi] += delta[gi];
                    best[gi] = run[gi] < best[gi] ? run[gi] : best[gi];
                }
            }
        }
        if (SEMI) {
#pragma unroll
            for (int gi = 0; gi < G; gi++)
                if (group0 + gi < n_groups)
                    dst[static_cast<size_t>(q - ref_start) * ld + gi * kLanes] = static_cast<int16_t>(-best[gi]);
            continue;
        }
        // D[m][n] = m + sum over the n subject columns of (VP - VN).
#pragma unroll
        for (int gi = 0; gi < G; gi++) {
            int score = ref_len;
#pragma unroll
            for (int w = 0; w < NW; w++) {
                const int rem = read_len - 32 * w;
                const uint32_t m = rem >= 32 ? ~0u : (rem <= 0 ? 0u : ((1u << rem) - 1u));
                score += __popc(vp[gi * NW + w] & m) - __popc(vn[gi * NW + w] & m);
            }
            if (group0 + gi < n_groups)
                dst[static_cast<size_t>(q - ref_start) * ld + gi * kLanes] = static_cast<int16_t>(-score);
        }
    }
}

// ---- generated row loop (gen_rows_asm.py) ----------------------------------------------------------
// default of myers_peq_max_words(): the widest subject with its five Peq planes resident.  28 until round 5; 30 and 32 words since then
// — their rows run the two carry chains in turns over blocks of nine words (rows_ir.myers_body(split = 9)), which holds 18 temporaries
// where the row-long phases hold 64: 255 VGPRs, eight instructions per word against nine on the code planes (config 5: 4,214 -> 3,980 ms,
// profiles/r05_balance_ab.txt, r05_split_k9.txt).  BGSA_MYERS_PEQ_MAX_WORDS=28 puts 29 .. 32 words back on the code planes (A/B).
constexpr int kPeqMaxWords = 32;
constexpr int kSemiPeqMaxWords = 32;  // widest semi-global kernel with resident Peq planes (myers_semi_rows_asm; 26..32 words: chains in turns, round 5)
constexpr int kPairMaxWords = 2;  // widths instantiated as myers_pair_rows_asm (gen_rows_asm.py: MYERS_PAIR_NW)
constexpr int kBandPairMaxWords = 5;  // widest band loop with two subject groups per wave (gen_rows_asm.py: MYERS_BAND_PAIR_NW = 3..5)
#include "myers_rows_gen.inc"
#include "_gen/myers_band_rows_gen.inc"   // the certified band's row loops (written by the Makefile: gen_rows_asm.py --band)

// Same task decomposition as above, but all rows of a query run inside one generated asm block:
// five in-place row bodies selected by a scalar jump per row, every VALU instruction full rate
// (the inter-word shifts are add-with-carry chains instead of v_alignbit_b32), query characters
// from the packed code stream.  This is the kernel the launcher picks whenever NW <= 8.
// BAND (3..8 words, myers_band.h): the rows run on the band stream, each on the words of its window; a wave whose lanes are not
// all certified (score <= band_limit) runs the query again with full rows.  The guard: every such fallback is added to the
// launch's pair band_launch = {queries redone, queries banded} (with the queries this wave banded since its last report), and
// once the pair holds at least 64 banded queries of which more than one in eight were redone, the wave stops banding for the
// rest of its tasks.  Pairs that are all far apart then cost about one fallback per wave over the full rows; where
// (nearly) every wave is certified the pair is touched once per wave, at its end, when the wave adds the rest of its banded
// queries.  band_stats_add_kernel then adds the launch's pair to the device's sticky counts (bgsa_hip_myers_band_stats).
// LENS (a bucket of mixed subject lengths, bgsa_hip_cal_align_score_lens_ex): the rows run as ever over the bucket's padded width;
// column j of a global DP depends on columns <= j only, so the lane's score is the epilogue's sum under the mask of the lane's OWN
// length read_lens[column] — per lane instead of wave-uniform, once per query.  What lies behind a subject's end never enters.
// A separate instantiation: the equal-length kernels keep their code and their register counts.  Never with BAND: the window
// schedule and the limit certify one (m, n), DESIGN §4.2.
// the band kernels' snapshots of a sharing launch (dynamic LDS: launch_asm sizes it by the launch's depths; none without sharing)
extern __shared__ uint4 prefix_slots[];
// The lane's number formed where it is asked for, two instructions the compiler neither hoists nor keeps: for the kernels at
// their register limit, where a lane number kept across a row loop for a rare use costs the loop a register or a spill.
__device__ __forceinline__ unsigned lane_now()
{
    unsigned l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}
// SHARE (prefix sharing, myers_band.h) is a separate instantiation of the band kernels: a launch that does not share runs a
// kernel without the segment loop, the entry load and the slots (within one VGPR and two SGPRs of what it was before; the
// loop cost such a launch about 0.4 % while every band kernel carried it, LABNOTES §24.4).
// Waves per SIMD the SHARING kernels are held to — those of the same kernel without sharing, as the resource report gives them
// (3..8 words: 8, 8, 8, 8 | 7, 7 | 6, 6 | 5, the counter kernels from 6 words on one fewer; two groups: 8, 7 | 6, 5).  The segment
// loop put the counter kernels of 3..5 words a few scalar registers above the 100 that eight waves leave each; asked for, the
// compiler parks those in vector-register lanes outside the row loop.  The figure is a MINIMUM the compiler is forced under:
// a later change that needs more registers will not show up as a lost wave but as scratch, so whoever changes these kernels
// runs -Rpass-analysis=kernel-resource-usage again and looks at ScratchSize (0 everywhere today) as well as at the waves.
// 1 (every other kernel) asks for nothing.
// RESCUE (myers_band.h; two groups only) is one more separate instantiation: it changes the certificate block behind the
// score popcounts and nothing else, and every launch that does not rescue runs the kernel it ran before.  The same figures
// hold for it (LABNOTES §33): forced where it shares, found by the compiler where it does not.
constexpr int band_kernel_waves(int nw, int g, bool dyn, bool share)
{
    if (!share) return 1;
    if (g == 2) return nw == 3 ? 8 : (nw == 4 ? (dyn ? 6 : 7) : 5);
    return nw <= 5 ? 8 : (nw == 6 ? (dyn ? 7 : 8) : (nw == 7 ? (dyn ? 6 : 7) : (dyn ? 5 : 6)));
}
template <int NW, int G, bool DYN = false, bool BAND = false, bool LENS = false, bool SHARE = false, bool RESCUE = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(band_kernel_waves(NW, G, DYN, SHARE)))) void myers_global_asm_kernel(
    const unsigned char *__restrict__ streams, const uint32_t *__restrict__ peq,
    int16_t *__restrict__ out, int ref_len, int read_len, long long ld, int n_groups, int word_num,
    int n_queries, int q_tile, int stream_stride_bytes, unsigned *__restrict__ fault_word,
    unsigned *__restrict__ task_counter, int band_limit = 0, unsigned long long *__restrict__ band_launch = nullptr,
    const int32_t *__restrict__ read_lens = nullptr, unsigned long long prefix_segments = 0,
    const PrefixEntry *__restrict__ order = nullptr)
{
    static_assert(!BAND || (NW >= kBandMinWords && NW <= kBandMaxWords && (G == 1 || (G == 2 && NW <= kBandPairMaxWords))),
                  "band: 3..8 words, one subject group per wave — or two up to 5 words");
    static_assert(!(LENS && BAND), "the certified band is derived from one (m, n): a length-aware launch runs full rows");
    static_assert(!SHARE || BAND, "prefix sharing: the band kernels only");
    static_assert(!RESCUE || (BAND && G == 2), "rescue: the two-group band kernels only");
    // EARLY LEAVE (myers_band.h) is part of the RESCUE instantiations, no flag of its own: it needs the pool, which only they
    // have, and it costs them a few instructions per query behind the row loop — two scalar compares where the launch has no
    // cuts.  Every other instantiation keeps its code.  band_limit carries the cuts' constants above B (band_early_word).
    constexpr bool kEarly = RESCUE;
    // LENS: the lane's length is loaded once per task and kept across the row loops, one VGPR per group — except beyond 8 words,
    // where the widths sit at their occupancy steps (20 words 238, 28 and 32 words 255 VGPRs): there the epilogue loads it again
    // per query, one dword per lane against >= 10 words x ref_len rows.
    constexpr bool kLenPerQuery = LENS && NW > 8;
    const int lane = threadIdx.x & (kLanes - 1);
    // Static mapping (DYN = false): workgroup (x, y) = (four wave-groups, query tile).  Dynamic (bgsa_common.h "dynamic task
    // handout"; a separate instantiation, so that the static kernels keep their register counts: the loop costs 5-8 VGPRs,
    // which the widest widths do not have): a persistent grid whose waves take (wave-group, tile) tasks, tile-major like the
    // static order.
    const unsigned wave_groups = (static_cast<unsigned>(n_groups) + G - 1) / G;
    const unsigned n_tasks = wave_groups * ((static_cast<unsigned>(n_queries) + q_tile - 1) / q_tile);   // < 2^32: the launcher checked
    unsigned task = 0, task_issued = 0;
    if constexpr (DYN) {
        task = first_wave_task();
        if (task >= n_tasks) return;
    }
    int band_on = 1, unreported = 0;   // wave-uniform (BAND): the guard, and the banded queries not yet added to band_launch[1]
    // the lane that reports for the wave.  RESCUE: its number is formed where it is asked for — the kernels that share sit at their
    // register limit, and `lane` kept for the rare reports costs them a spill
    [[maybe_unused]] auto reporting_lane = [&]() {
        if constexpr (RESCUE) {
            return lane_now() == 0;
        } else
            return lane == 0;
    };
    do {
        int group0, tile;
        if constexpr (DYN) {
            group0 = static_cast<int>((task % wave_groups) * G);
            tile = static_cast<int>(task / wave_groups);
        } else {
            group0 = __builtin_amdgcn_readfirstlane((blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)) * G);
            tile = blockIdx.y;
            if (group0 >= n_groups) return;
        }

        uint32_t P[kChars][G * NW];
#pragma unroll
        for (int gi = 0; gi < G; gi++) {
            const bool live = group0 + gi < n_groups;
            const uint32_t *g = peq + static_cast<size_t>(group0 + gi) * kChars * word_num * kLanes + lane;
#pragma unroll
            for (int c = 0; c < kChars; c++)
#pragma unroll
                for (int w = 0; w < NW; w++)
                    P[c][gi * NW + w] = (live && w < word_num) ? g[(c * word_num + w) * kLanes] : 0u;
        }

        [[maybe_unused]] int own_len[G];   // LENS: this lane's subject length per group (a group past the end of the bucket is not stored)
        if constexpr (LENS && !kLenPerQuery) {
#pragma unroll
            for (int gi = 0; gi < G; gi++)
                own_len[gi] = group0 + gi < n_groups ? lane_read_len(read_lens, static_cast<size_t>(group0 + gi) * kLanes + lane, read_len) : 0;
        }

        const int q0 = tile * q_tile;
        const int q1 = (q0 + q_tile < n_queries) ? q0 + q_tile : n_queries;
        int16_t *dst = out + static_cast<size_t>(group0) * kLanes + lane;

        for (int k = q0; k < q1; k++) {
            if constexpr (DYN) {   // the next task, asked for under this one's last query: late enough that the tail of a
                if (k == q1 - 1) task_issued = issue_wave_task(task_counter);   // launch is handed out as waves free up, early enough that the round trip is hidden
            }
            // SHARE: the tile is walked in sorted order, k is a sorted position, and its entry names the query and the segment it may
            // start at (a pointer of its own, read-only: a scalar load)
            int q = k, seg = 0;
            if constexpr (SHARE) {
                const int2 e = *reinterpret_cast<const int2 *>(order + k);   // {q, lcp | seg << 16}
                q = __builtin_amdgcn_readfirstlane(e.x);
                seg = __builtin_amdgcn_readfirstlane(e.y >> 16);
            }
            uint32_t st[2 * G * NW];  // {VP, VN} per word
#pragma unroll
            for (int w = 0; w < G * NW; w++) {
                st[2 * w] = ~0u;
                st[2 * w + 1] = 0u;
            }
            const unsigned long long s =
                reinterpret_cast<unsigned long long>(streams) + static_cast<unsigned long long>(q) * stream_stride_bytes;
            if constexpr (BAND) {
                // one asm block for both passes: band = 0 runs the same stream with full rows.  G = 2: the wave carries two subject
                // groups through every row; score and certificate are per group, the statistics stay in units of (64-subject group,
                // query), and a second group past the end of the bucket (odd group count: zero masks) is neither stored, nor tested,
                // nor counted.  One live group with a lane above B sends the WAVE — both groups — through the full rows.
                const int n_live = G == 1 ? 1 : (group0 + 1 < n_groups ? 2 : 1);
                const int tried = band_on * n_live;
                int band = band_on, score[G];
                // Prefix sharing: the stream is n_depths + 1 segments, and behind segment j < n_depths the banded pass leaves words
                // 0..1 of each group in this wave's slot j.  A slot then holds the state of the CURRENT query's first depth[j] rows:
                // either this query ran them and wrote the slot, or it resumed at or behind that depth — it shares those rows with
                // whoever wrote it.  The full-row pass starts at row 0 and stores nothing (a banded snapshot is no full-row state);
                // a wave whose guard is off shares nothing.  Without SHARE: one segment, the band stream as ever.
                const int n_depths = SHARE ? static_cast<int>(prefix_segments >> 56) : 0;   // wave-uniform: a kernel argument
                // kEarly: a lane is certified by score <= limit, its own (formed behind the rows, below; B wherever there are no
                // cuts).  over[gi] = the group's lanes above theirs, as a mask: a limit kept per lane beside the score up to the
                // store is a vector register per group, and these kernels have none to give
                [[maybe_unused]] unsigned long long over[G];
                [[maybe_unused]] auto is_over = [&](int gi) { return ((over[gi] >> lane_now()) & 1ull) != 0; };
                const bool sharing = SHARE && band_on;
                // [depth][wave][group][lane].  RESCUE: formed again at either use, like reporting_lane() and for its reason
                [[maybe_unused]] auto wave_slots = [&]() {
                    if constexpr (RESCUE) {
                        return prefix_slots + __builtin_amdgcn_readfirstlane((threadIdx.x >> 6) * G) * kLanes + lane_now();
                    } else
                        return prefix_slots + ((threadIdx.x >> 6) * G) * kLanes + lane;
                };
                if (!sharing) seg = 0;
                if (SHARE && seg) {
                    const uint4 *const slots = wave_slots();
#pragma unroll
                    for (int gi = 0; gi < G; gi++) {
                        const uint4 v = slots[((seg - 1) * kWavesPerBlock * G + gi) * kLanes];
                        st[2 * gi * NW] = v.x;
                        st[2 * gi * NW + 1] = v.y;
                        st[2 * gi * NW + 2] = v.z;
                        st[2 * gi * NW + 3] = v.w;
                    }
                }
                for (;;) {
                    for (; seg <= n_depths; seg++) {
                        const int at = SHARE ? static_cast<int>((prefix_segments >> (8 * seg)) & 0xffu) * 8 : 0;   // the segment's offset in the stream
                        const int left = myers_band_rows_asm<NW, G>(st, P, uniform_u64(s + static_cast<unsigned>(at)),
                                                                    __builtin_amdgcn_readfirstlane((stream_stride_bytes - at) / 8 - 2),
                                                                    __builtin_amdgcn_readfirstlane(band));
                        note_stream_fault(fault_word, left);
                        if (SHARE && sharing && band && seg < n_depths) {
                            uint4 *const slots = wave_slots();
#pragma unroll
                            for (int gi = 0; gi < G; gi++)
                                slots[(seg * kWavesPerBlock * G + gi) * kLanes] =
                                    make_uint4(st[2 * gi * NW], st[2 * gi * NW + 1], st[2 * gi * NW + 2], st[2 * gi * NW + 3]);
                        }
                    }
                    // kEarly: behind cut (r, w) no row touched words 0 .. w, so they hold D'[r][j_r] - r, j_r = 32 (w + 1): the sum
                    // that is the score behind word w, and the lane's limit is the least of B and the cuts' M = D'[r][j_r] + (r - j_r)
                    // (myers_band.h).  The cuts are wave-uniform, a kernel argument; the full-row pass forms a limit nobody reads.
                    if constexpr (kEarly) {
                        // (decoded here, query by query: kept across the row loop the five fields are five scalar registers more,
                        // which the counter kernels, at their limit, park in vector lanes)
                        unsigned packed = static_cast<unsigned>(band_limit);
                        asm volatile("" : "+s"(packed));
                        int cut_word[kBandMaxCuts], cut_add[kBandMaxCuts];
#pragma unroll
                        for (int j = 0; j < kBandMaxCuts; j++) {
                            const unsigned cut = (packed >> (kBandEarlyLimitBits + kBandEarlyCutBits * j)) & ((1u << kBandEarlyCutBits) - 1u);
                            cut_word[j] = cut ? static_cast<int>(cut >> 9) : -1;       // w
                            cut_add[j] = static_cast<int>(cut & 0x1ffu) - ref_len;     // 2 r - j_r, less the score's first term
                        }
#pragma unroll
                        for (int gi = 0; gi < G; gi++) {
                            score[gi] = ref_len;
                            int limit = static_cast<int>(packed & kBandEarlyLimitMask);
#pragma unroll
                            for (int w = 0; w < NW; w++) {
                                const int rem = read_len - 32 * w;
                                const uint32_t m = rem >= 32 ? ~0u : (rem <= 0 ? 0u : ((1u << rem) - 1u));
                                score[gi] += __popc(st[2 * (gi * NW + w)] & m) - __popc(st[2 * (gi * NW + w) + 1] & m);
#pragma unroll
                                for (int j = 0; j < kBandMaxCuts; j++)   // (a band launch has (read_len + 31) / 32 = NW: words below the last are whole)
                                    if (w < NW - 1 && w == cut_word[j]) limit = score[gi] + cut_add[j] < limit ? score[gi] + cut_add[j] : limit;
                            }
                            over[gi] = __builtin_amdgcn_ballot_w64(score[gi] > limit);
                        }
                    } else {
#pragma unroll
                        for (int gi = 0; gi < G; gi++) {
                            score[gi] = ref_len;
#pragma unroll
                            for (int w = 0; w < NW; w++) {
                                const int rem = read_len - 32 * w;
                                const uint32_t m = rem >= 32 ? ~0u : (rem <= 0 ? 0u : ((1u << rem) - 1u));
                                score[gi] += __popc(st[2 * (gi * NW + w)] & m) - __popc(st[2 * (gi * NW + w) + 1] & m);
                            }
                        }
                    }
                    if (!band) break;
                    int n_over = 0;   // live groups with a lane above the limit (B; early leave: the lane's own)
#pragma unroll
                    for (int gi = 0; gi < G; gi++)
                        if (gi < n_live && (kEarly ? over[gi] : __builtin_amdgcn_ballot_w64(score[gi] > band_limit)) != 0) n_over++;
                    if (n_over == 0) break;
                    if constexpr (G == 1) n_over = 1;   // (what it is: said so that the one-group kernels keep their code)
                    if constexpr (RESCUE) {
                        // No group with more than kRescueMaxLanes lanes above B: the wave claims a pool entry per such lane — one
                        // atomic —, each of them writes its pair at base + its rank under the ballots, and the loop ends with the
                        // banded scores: the store below leaves those lanes out.  A claim that does not fit the pool marks what it
                        // holds of it as void, so that every entry below the capacity is written, and the wave goes on as it does
                        // for a group over the limit: the redo, the guard's pair, and the count of either in band_launch[3].
                        const unsigned c0 = __popcll(over[0]), c1 = n_live > 1 ? __popcll(over[1]) : 0u;
                        unsigned forced = (c0 > kRescueMaxLanes ? 1u : 0u) + (c1 > kRescueMaxLanes ? 1u : 0u);
                        if (forced == 0) {
                            unsigned *const words = reinterpret_cast<unsigned *>(band_launch) - 16;   // band_launch_words() of them
                            unsigned long long claim = 0;
                            if (reporting_lane()) claim = atomicAdd(rescue_claimed(words), static_cast<unsigned long long>(c0 + c1));
                            // (32-bit scalars from here on: there is no scalar 64-bit "less than", and a vector one makes the branches below divergent)
                            const unsigned base = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(claim)),
                                           base_hi = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(claim >> 32));
                            const unsigned capacity = __builtin_amdgcn_readfirstlane(*rescue_capacity(words));
                            const unsigned room = (base_hi == 0 && base < capacity) ? capacity - base : 0u;   // entries of the claim below the capacity
                            const bool fits = c0 + c1 <= room;
                            RescueEntry *const mine = rescue_pool(words) + base;   // (dereferenced where room > 0)
                            // (the lane number formed here: kept across the row loop it would cost the loop a register)
                            const unsigned column = lane_now() + static_cast<unsigned>(group0) * kLanes;
#pragma unroll
                            for (int gi = 0; gi < G; gi++) {
                                const bool up = gi < n_live && is_over(gi);
                                const unsigned long long over = __builtin_amdgcn_ballot_w64(up);
                                const unsigned at = (gi ? c0 : 0u) + __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(over >> 32),
                                                                                              __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(over), 0u));
                                if (up && at < room)
                                    mine[at] = fits ? RescueEntry{q, static_cast<int>(column + gi * kLanes)} : RescueEntry{-1, -1};
                            }
                            if (fits) break;
                            forced = static_cast<unsigned>(n_over);
                        }
                        if (reporting_lane()) atomicAdd(&band_launch[3], static_cast<unsigned long long>(forced));
                    }
                    band = 0;   // a lane is not certified: the whole wave runs the query again with full rows
                    seg = 0;    // ... from row 0
                    unsigned long long r = static_cast<unsigned long long>(n_over),
                                       b = static_cast<unsigned long long>(unreported) + n_live;
                    if (reporting_lane()) {
                        r += atomicAdd(&band_launch[0], r);
                        b += atomicAdd(&band_launch[1], b);
                    }
                    r = uniform_u64(r);   // lane 0's values: the first active lane, as every lane is
                    b = uniform_u64(b);
                    unreported = -n_live;   // this query is reported; banded += n_live below brings it to 0
                    if (b >= 64 && 8 * r > b) band_on = 0;
#pragma unroll
                    for (int w = 0; w < G * NW; w++) {
                        st[2 * w] = ~0u;
                        st[2 * w + 1] = 0u;
                    }
                }
                unreported += tried;
#pragma unroll
                for (int gi = 0; gi < G; gi++)
                    if (gi < n_live && !(RESCUE && band && is_over(gi)))   // (band still set: those lanes are in the pool)
                        dst[static_cast<size_t>(q) * ld + gi * kLanes] = static_cast<int16_t>(-score[gi]);
            } else {
                int left;
                if constexpr (NW <= kPairMaxWords)  // short rows: two per stream token (launch_asm packs it so)
                    left = myers_pair_rows_asm<NW, G>(st, P, uniform_u64(s), __builtin_amdgcn_readfirstlane(stream_stride_bytes / 8 - 2));
                else
                    left = myers_rows_asm<NW, G>(st, P, uniform_u64(s), __builtin_amdgcn_readfirstlane(stream_stride_bytes / 8 - 2));
                note_stream_fault(fault_word, left);
#pragma unroll
                for (int gi = 0; gi < G; gi++) {
                    int score = ref_len;  // D[m][n] = m + sum over the n subject columns of (VP - VN)
                    int n_cols = read_len;   // LENS: the lane's own n
                    if constexpr (kLenPerQuery) {
                        // (the lane number formed here: an address kept per lane across the row loop is two VGPRs these widths lack —
                        // 28 words: 255 -> 326, 32 words: 255 -> 258, one wave per SIMD instead of two)
                        const unsigned lane_e = lane_now();
                        n_cols = group0 + gi < n_groups ? lane_read_len(read_lens, static_cast<size_t>(group0 + gi) * kLanes + lane_e, read_len) : 0;
                    }
                    else if constexpr (LENS)
                        n_cols = own_len[gi];
                    // (the NW masks depend on the task only: laundered, or the compiler forms them once per task and keeps NW more
                    // VGPRs across the row loop — 28 words: 255 -> 423)
                    if constexpr (LENS) asm volatile("" : "+v"(n_cols));
#pragma unroll
                    for (int w = 0; w < NW; w++) {
                        const int rem = n_cols - 32 * w;
                        const uint32_t m = rem >= 32 ? ~0u : (rem <= 0 ? 0u : ((1u << rem) - 1u));
                        score += __popc(st[2 * (gi * NW + w)] & m) - __popc(st[2 * (gi * NW + w) + 1] & m);
                    }
                    if (group0 + gi < n_groups)
                        dst[static_cast<size_t>(q) * ld + gi * kLanes] = static_cast<int16_t>(-score);
                }
            }
        }
        if constexpr (DYN) task = resolve_wave_task(task_issued);
    } while (DYN && task < n_tasks);
    if constexpr (BAND) {
        if (reporting_lane() && unreported) atomicAdd(&band_launch[1], static_cast<unsigned long long>(unreported));
    }
}

// ---- semi-global (the generator's -m 0 -s, MyersGenerator.java:56-223) -------------------------------------
// The subject end to end inside the query: D[i][0] = 0 for every query row, result = -min over rows of D[i][n].
// What the semi-global kernels do to a subject once per task (rows_ir.py: semi_align): its n columns are moved
// to the top of the `total_words` words they occupy, so that column n is bit 31 of the last word and the
// HP / HN shift chains drop D[i][n] - D[i-1][n] out as their final carries; the s = 32 * total_words - n unused
// low columns match every character and start at VP = 0, which keeps them at D = 0 — the row edge of the mode,
// delivered to the first real column.
// Source word `i` of class plane `row` (words row[0 .. word_num), stride kLanes), zero outside the subject.
// Unconditional load, index clamped and result masked: a guarded load becomes a branch per word and the
// loads of a block then complete one after the other instead of together.
__device__ __forceinline__ uint32_t semi_source_word(const uint32_t *row, int word_num, int i)
{
    const int ic = i < 0 ? 0 : (i >= word_num ? word_num - 1 : i);
    return row[ic * kLanes] & ((i >= 0 && i < word_num) ? ~0u : 0u);
}
// Aligned word from its two source words, s = 32 q + r: hi = source word aw - q, lo = source word aw - q - 1.
__device__ __forceinline__ uint32_t semi_funnel(uint32_t hi, uint32_t lo, int r)
{
    return r ? __builtin_amdgcn_alignbit(hi, lo, 32 - r) : hi;
}
// the unused low columns of aligned word aw (wave-uniform)
__device__ __forceinline__ uint32_t semi_dummy_mask(int aw, int s)
{
    const int d = s - 32 * aw;
    return d >= 32 ? ~0u : (d <= 0 ? 0u : ((1u << d) - 1u));
}

// Subjects up to 1024 bp (resident Peq planes at every width; 26..32 words with the two carry chains in turns): generated asm row loop of
// myers_semi_body, 8 VALU per word + 3 per row.
// LENS (a bucket of mixed read lengths, bgsa_hip_myers_place_score_lens_dev): nothing in the row loop depends on the length — the subject
// is right-aligned once per task, and from then on the carries that leave the top word are D[i][n] - D[i-1][n] whatever n is.  So every
// lane right-aligns by its OWN n = read_lens[column]: shift, source word indices (per-lane addresses; the loads stay unconditional),
// dummy mask and start score are per lane instead of wave-uniform, and the generated rows run unchanged.  Column n of every lane is
// bit 31 of the last word; what lies behind a read's end is shifted out of the top word and never enters.  n = 0 (a clamped length):
// all columns dummy, VP = 0, score 0.  A separate instantiation: the equal-length kernels keep their code and their register counts.
// The lane keeps n across the row loop (one VGPR) except where the width sits at the register limit (semi_len_per_query): there the
// per-query set-up loads it again, one dword per lane against NW x ref_len rows.
constexpr bool semi_len_per_query(int nw) { return nw >= 32; }
template <int NW, bool LENS = false>
__global__ __launch_bounds__(256) void myers_semi_asm_kernel(
    const unsigned char *__restrict__ streams, const uint32_t *__restrict__ peq,
    int16_t *__restrict__ out, int ref_len, int read_len, long long ld, int n_groups, int word_num,
    int n_queries, int q_tile, int stream_stride_bytes, unsigned *__restrict__ fault_word,
    const int32_t *__restrict__ read_lens = nullptr)
{
    constexpr bool kLenPerQuery = LENS && semi_len_per_query(NW);
    const int lane = threadIdx.x & (kLanes - 1);
    const int group = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (group >= n_groups) return;
    int own_len = read_len;   // LENS: per lane; else wave-uniform, and everything derived from it stays scalar
    if constexpr (LENS) own_len = lane_read_len(read_lens, static_cast<size_t>(group) * kLanes + lane, read_len);
    const int s_cols = 32 * NW - own_len, sq = s_cols >> 5, sr = s_cols & 31;

    uint32_t P[kChars][NW];
    const uint32_t *g = peq + static_cast<size_t>(group) * kChars * word_num * kLanes + lane;
#pragma unroll
    for (int c = 0; c < kChars; c++) {
        const uint32_t *row = g + static_cast<size_t>(c) * word_num * kLanes;
        uint32_t src[NW + 1];
#pragma unroll
        for (int w = 0; w <= NW; w++) src[w] = semi_source_word(row, word_num, w - sq - 1);
#pragma unroll
        for (int w = 0; w < NW; w++) P[c][w] = semi_funnel(src[w + 1], src[w], sr) | semi_dummy_mask(w, s_cols);
    }

    const int q0 = blockIdx.y * q_tile;
    const int q1 = (q0 + q_tile < n_queries) ? q0 + q_tile : n_queries;
    int16_t *dst = out + static_cast<size_t>(group) * kLanes + lane;

    for (int q = q0; q < q1; q++) {
        uint32_t st[2 * NW + 2];
        int n_cols = own_len;
        if constexpr (kLenPerQuery) {
            // (the lane number formed here: an address kept per lane across the row loop is two VGPRs this width lacks)
            const unsigned lane_e = lane_now();
            n_cols = lane_read_len(read_lens, static_cast<size_t>(group) * kLanes + lane_e, read_len);
        }
        // (LENS: the NW masks depend on the task only: laundered, or the compiler forms them once per task and keeps NW more VGPRs
        // across the row loop)
        if constexpr (LENS) asm volatile("" : "+v"(n_cols));
        const int dummy_cols = 32 * NW - n_cols;
#pragma unroll
        for (int w = 0; w < NW; w++) {
            st[2 * w] = ~semi_dummy_mask(w, dummy_cols);
            st[2 * w + 1] = 0u;
        }
        st[2 * NW] = st[2 * NW + 1] = static_cast<uint32_t>(n_cols);   // D[0][n] = n (genSemiGlobal: min_score = score = read_len), LENS: the lane's own
        const unsigned long long s =
            reinterpret_cast<unsigned long long>(streams) + static_cast<unsigned long long>(q) * stream_stride_bytes;
        note_stream_fault(fault_word, myers_semi_rows_asm<NW>(st, P, uniform_u64(s),
                                                              __builtin_amdgcn_readfirstlane(stream_stride_bytes / 8 - 2)));
        dst[static_cast<size_t>(q) * ld] = static_cast<int16_t>(-static_cast<int>(st[2 * NW + 1]));
    }
}

// Long subjects (769..1024 bp; 257..1024 before the Peq-resident kernels were widened): the wave turns its five Peq planes into the subject's 3-bit
// character-code planes once per task (B0 = C|T, B1 = G|T, B2 = N) and the row body rebuilds the
// match mask of its class with one v_bitop3 per word (rows_ir.py:myers_planes_body): 9 VALU per
// word, 7*NW+1 registers, two waves per SIMD at NW = 32.
#ifdef BGSA_PLANES_WAVES_PER_EU   // measurement builds (scripts/build_variant.sh ... EXTRA=-DBGSA_PLANES_WAVES_PER_EU=3): ask for an occupancy
#define BGSA_PLANES_OCCUPANCY __attribute__((amdgpu_waves_per_eu(BGSA_PLANES_WAVES_PER_EU, BGSA_PLANES_WAVES_PER_EU)))
#else
#define BGSA_PLANES_OCCUPANCY
#endif
template <int NW, bool DYN = false>
__global__ __launch_bounds__(256) BGSA_PLANES_OCCUPANCY void myers_global_planes_kernel(
    const unsigned char *__restrict__ streams, const uint32_t *__restrict__ peq,
    int16_t *__restrict__ out, int ref_len, int read_len, long long ld, int n_groups, int word_num,
    int n_queries, int q_tile, int stream_stride_bytes, unsigned *__restrict__ fault_word,
    unsigned *__restrict__ task_counter)
{
    const int lane = threadIdx.x & (kLanes - 1);
    // DYN: the waves of a persistent grid take (group, tile) tasks from a counter (bgsa_common.h "dynamic task handout")
    const unsigned n_tasks = static_cast<unsigned>(n_groups) * ((static_cast<unsigned>(n_queries) + q_tile - 1) / q_tile);   // < 2^32: the launcher checked
    unsigned task = 0, task_issued = 0;
    if constexpr (DYN) {
        task = first_wave_task();
        if (task >= n_tasks) return;
    }
    do {
        int group, tile;
        if constexpr (DYN) {
            group = static_cast<int>(task % static_cast<unsigned>(n_groups));
            tile = static_cast<int>(task / static_cast<unsigned>(n_groups));
        } else {
            group = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
            tile = blockIdx.y;
            if (group >= n_groups) return;
        }

        uint32_t Bp[3 * NW];
        const uint32_t *g = peq + static_cast<size_t>(group) * kChars * word_num * kLanes + lane;
#pragma unroll
        for (int w = 0; w < NW; w++) {
            uint32_t p[kChars];
#pragma unroll
            for (int c = 0; c < kChars; c++) p[c] = (w < word_num) ? g[(c * word_num + w) * kLanes] : 0u;
            Bp[3 * w + 0] = p[1] | p[3];
            Bp[3 * w + 1] = p[2] | p[3];
            Bp[3 * w + 2] = p[4];
        }

        const int q0 = tile * q_tile;
        const int q1 = (q0 + q_tile < n_queries) ? q0 + q_tile : n_queries;
        int16_t *dst = out + static_cast<size_t>(group) * kLanes + lane;

        for (int q = q0; q < q1; q++) {
            if constexpr (DYN) {   // the next task, asked for under this one's last query: late enough that the tail of a
                if (q == q1 - 1) task_issued = issue_wave_task(task_counter);   // launch is handed out as waves free up, early enough that the round trip is hidden
            }
            uint32_t st[2 * NW];
#pragma unroll
            for (int w = 0; w < NW; w++) {
                st[2 * w] = ~0u;
                st[2 * w + 1] = 0u;
            }
            const unsigned long long s =
                reinterpret_cast<unsigned long long>(streams) + static_cast<unsigned long long>(q) * stream_stride_bytes;
            note_stream_fault(fault_word, myers_planes_rows_asm<NW>(st, Bp, uniform_u64(s),
                                                                    __builtin_amdgcn_readfirstlane(stream_stride_bytes / 8 - 2)));
            int score = ref_len;
#pragma unroll
            for (int w = 0; w < NW; w++) {
                const int rem = read_len - 32 * w;
                const uint32_t m = rem >= 32 ? ~0u : (rem <= 0 ? 0u : ((1u << rem) - 1u));
                score += __popc(st[2 * w] & m) - __popc(st[2 * w + 1] & m);
            }
            dst[static_cast<size_t>(q) * ld] = static_cast<int16_t>(-score);
        }
        if constexpr (DYN) task = resolve_wave_task(task_issued);
    } while (DYN && task < n_tasks);
}

// Semi-global on the code planes (801..1024 bp until round 5; since then those widths run myers_semi_asm_kernel with the chains in turns and
// this kernel is what BGSA_MYERS_PEQ_MAX_WORDS selects): the code planes right-aligned like the Peq planes of myers_semi_asm_kernel;
// the unused low columns get code 7 (all three planes set), which MATCH3's truth tables treat as "matches every
// class" (rows_ir.py: myers_semi_planes_body) — 9 VALU per word + 3 per row, two waves per SIMD at NW = 32.
template <int NW>
__global__ __launch_bounds__(256) void myers_semi_planes_kernel(
    const unsigned char *__restrict__ streams, const uint32_t *__restrict__ peq,
    int16_t *__restrict__ out, int ref_len, int read_len, long long ld, int n_groups, int word_num,
    int n_queries, int q_tile, int stream_stride_bytes, unsigned *__restrict__ fault_word)
{
    const int lane = threadIdx.x & (kLanes - 1);
    const int group = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    if (group >= n_groups) return;
    const int s_cols = 32 * NW - read_len, sq = s_cols >> 5, sr = s_cols & 31;

    uint32_t Bp[3 * NW];
    const uint32_t *g = peq + static_cast<size_t>(group) * kChars * word_num * kLanes + lane;
    {
        const uint32_t *rc = g + static_cast<size_t>(1) * word_num * kLanes, *rg = g + static_cast<size_t>(2) * word_num * kLanes;
        const uint32_t *rt = g + static_cast<size_t>(3) * word_num * kLanes, *rn = g + static_cast<size_t>(4) * word_num * kLanes;
        uint32_t lo[3];   // source word (w - sq - 1) of the three code planes
        {
            const uint32_t t = semi_source_word(rt, word_num, -sq - 1);
            lo[0] = semi_source_word(rc, word_num, -sq - 1) | t;
            lo[1] = semi_source_word(rg, word_num, -sq - 1) | t;
            lo[2] = semi_source_word(rn, word_num, -sq - 1);
        }
#pragma unroll
        for (int w = 0; w < NW; w++) {
            const uint32_t t = semi_source_word(rt, word_num, w - sq);
            const uint32_t hi[3] = {semi_source_word(rc, word_num, w - sq) | t, semi_source_word(rg, word_num, w - sq) | t,
                                    semi_source_word(rn, word_num, w - sq)};
            const uint32_t dummy = semi_dummy_mask(w, s_cols);
#pragma unroll
            for (int i = 0; i < 3; i++) {
                Bp[3 * w + i] = semi_funnel(hi[i], lo[i], sr) | dummy;
                lo[i] = hi[i];
            }
        }
    }

    const int q0 = blockIdx.y * q_tile;
    const int q1 = (q0 + q_tile < n_queries) ? q0 + q_tile : n_queries;
    int16_t *dst = out + static_cast<size_t>(group) * kLanes + lane;

    for (int q = q0; q < q1; q++) {
        uint32_t st[2 * NW + 2];
#pragma unroll
        for (int w = 0; w < NW; w++) {
            st[2 * w] = ~semi_dummy_mask(w, s_cols);
            st[2 * w + 1] = 0u;
        }
        st[2 * NW] = st[2 * NW + 1] = static_cast<uint32_t>(read_len);
        const unsigned long long s =
            reinterpret_cast<unsigned long long>(streams) + static_cast<unsigned long long>(q) * stream_stride_bytes;
        note_stream_fault(fault_word, myers_semi_planes_rows_asm<NW>(st, Bp, uniform_u64(s),
                                                                     __builtin_amdgcn_readfirstlane(stream_stride_bytes / 8 - 2)));
        dst[static_cast<size_t>(q) * ld] = static_cast<int16_t>(-static_cast<int>(st[2 * NW + 1]));
    }
}

// Subjects longer than 1024 bp: column blocks of NW words.  For each query the wave runs the
// generated row loop once per block; the three carry chains of row r cross the block boundary
// through its carry buffer ([32-row chunk][add, HP, HN][lane] words in the workspace, first row in
// bit 31 — rows_ir.py: myers_block_body).  A fixed number of workgroups loops over the tasks so
// that the buffer count does not grow with the problem.
// SEMI (PEQ blocks only): the subject right-aligned over the n_blocks x NW words (semi_aligned_word above),
// HP carry-in 0, and D[i][n] followed through the last block's HP / HN carry-out words after the row loop.
template <int NW, bool PEQ = false, bool SEMI = false>
__global__ __launch_bounds__(256) void myers_blocked_kernel(
    const unsigned char *__restrict__ streams, const uint32_t *__restrict__ peq, int16_t *__restrict__ out,
    uint32_t *__restrict__ carry_all, int ref_len, int read_len, long long ld, int n_groups, int word_num,
    int n_queries, int q_tile, int stream_stride_bytes, int n_blocks, unsigned long long *task_counter,
    unsigned *__restrict__ fault_word)
{
    const int lane = threadIdx.x & (kLanes - 1);
    const int wave = threadIdx.x >> 6;
    const int n_chunks = (ref_len + 31) / 32;
    uint32_t *carry = carry_all + (static_cast<size_t>(blockIdx.x) * kWavesPerBlock + wave) * n_chunks * 3 * kLanes;
    const unsigned long long carry_base = uniform_u64(reinterpret_cast<unsigned long long>(carry));
    const int q_tiles = (n_queries + q_tile - 1) / q_tile;
    const long long n_tasks = static_cast<long long>((n_groups + kWavesPerBlock - 1) / kWavesPerBlock) * q_tiles;
    const int tail_rows = ref_len & 31;
    static_assert(!SEMI || PEQ, "semi-global column blocks use the Peq-resident body");
    const int s_cols = 32 * NW * n_blocks - read_len, sq = s_cols >> 5, sr = s_cols & 31;   // SEMI: unused low columns
    dephase_persistent_workgroup();

    for (long long task = next_blocked_task(task_counter); task < n_tasks; task = next_blocked_task(task_counter)) {
        const int group = __builtin_amdgcn_readfirstlane(static_cast<int>(task / q_tiles) * kWavesPerBlock + wave);
        const int tile = static_cast<int>(task % q_tiles);
        if (group >= n_groups) continue;  // wave-uniform; the wave still meets the others at the next task fetch
        const uint32_t *g = peq + static_cast<size_t>(group) * kChars * word_num * kLanes + lane;
        const int q0 = tile * q_tile;
        const int q1 = (q0 + q_tile < n_queries) ? q0 + q_tile : n_queries;
        for (int q = q0; q < q1; q++) {
            // carry-in of block 0: addition 0, HP 1 (the row edge D[i][0] - D[i-1][0] = +1; semi-global: 0), HN 0
            for (int c = 0; c < n_chunks; c++) {
                carry[(c * 3 + 0) * kLanes + lane] = 0u;
                carry[(c * 3 + 1) * kLanes + lane] = SEMI ? 0u : ~0u;
                carry[(c * 3 + 2) * kLanes + lane] = 0u;
            }
            const unsigned long long s =
                reinterpret_cast<unsigned long long>(streams) + static_cast<unsigned long long>(q) * stream_stride_bytes;
            int score = ref_len;
            for (int blk = 0; blk < n_blocks; blk++) {
                uint32_t Bp[PEQ ? 1 : 3 * NW];       // 3-bit character-code planes of the block, or
                uint32_t Pq[kChars][PEQ ? NW : 1];   // its five Peq planes (PEQ: 8 VALU per word, narrower blocks)
                if constexpr (SEMI) {
#pragma unroll
                    for (int c = 0; c < kChars; c++) {
                        const uint32_t *row = g + static_cast<size_t>(c) * word_num * kLanes;
                        uint32_t src[NW + 1];
#pragma unroll
                        for (int w = 0; w <= NW; w++) src[w] = semi_source_word(row, word_num, blk * NW + w - sq - 1);
#pragma unroll
                        for (int w = 0; w < NW; w++)
                            Pq[c][w] = semi_funnel(src[w + 1], src[w], sr) | semi_dummy_mask(blk * NW + w, s_cols);
                    }
                } else {
#pragma unroll
                    for (int w = 0; w < NW; w++) {
                        const int gw = blk * NW + w;
                        uint32_t p[kChars];
                        // unconditional loads (index clamped, result masked): a guarded load becomes a branch per
                        // word, and this runs per query and block, not once per task as in the plain kernels
                        const int gwc = gw < word_num ? gw : word_num - 1;
                        const uint32_t keep = gw < word_num ? ~0u : 0u;
#pragma unroll
                        for (int c = 0; c < kChars; c++) p[c] = g[(c * word_num + gwc) * kLanes] & keep;
                        if constexpr (PEQ) {
#pragma unroll
                            for (int c = 0; c < kChars; c++) Pq[c][w] = p[c];
                        } else {
                            Bp[3 * w + 0] = p[1] | p[3];
                            Bp[3 * w + 1] = p[2] | p[3];
                            Bp[3 * w + 2] = p[4];
                        }
                    }
                }
                uint32_t st[2 * NW + 6];
#pragma unroll
                for (int w = 0; w < NW; w++) {
                    st[2 * w] = SEMI ? ~semi_dummy_mask(blk * NW + w, s_cols) : ~0u;
                    st[2 * w + 1] = 0u;
                }
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    st[2 * NW + i] = carry[i * kLanes + lane];  // chunk 0
                    st[2 * NW + 3 + i] = 0u;
                }
                uint32_t voff = static_cast<uint32_t>(lane * 4);
                int left;
                if constexpr (PEQ)
                    left = myers_peq_block_rows_asm<NW>(st, Pq, voff, carry_base, uniform_u64(s),
                                                        __builtin_amdgcn_readfirstlane(stream_stride_bytes / 8 - 2));
                else
                    left = myers_block_rows_asm<NW>(st, Bp, voff, carry_base, uniform_u64(s),
                                                    __builtin_amdgcn_readfirstlane(stream_stride_bytes / 8 - 2));
                note_stream_fault(fault_word, left);
                // carry-out words of the last (possibly partial) chunk, first row left-aligned
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    const uint32_t word = tail_rows ? (st[2 * NW + 3 + i] << (32 - tail_rows)) : st[2 * NW + 3 + i];
                    carry[((n_chunks - 1) * 3 + i) * kLanes + lane] = word;
                }
#pragma unroll
                for (int w = 0; w < NW; w++) {
                    const int rem = read_len - 32 * (blk * NW + w);
                    const uint32_t m = rem >= 32 ? ~0u : (rem <= 0 ? 0u : ((1u << rem) - 1u));
                    score += __popc(st[2 * w] & m) - __popc(st[2 * w + 1] & m);
                }
            }
            if constexpr (SEMI) {
                // The carry buffer now holds what left the LAST block: per 32-row chunk the HP and HN bits of
                // column n, first row in bit 31 — D[i][n] - D[i-1][n] row by row.  D[0][n] = n.
                int run = read_len, best = read_len;
                for (int c = 0; c < n_chunks; c++) {
                    const uint32_t hpw = carry[(c * 3 + 1) * kLanes + lane], hnw = carry[(c * 3 + kMyersBlockHnPair) * kLanes + lane];
                    const int rows = ref_len - 32 * c < 32 ? ref_len - 32 * c : 32;
                    for (int b2 = 0; b2 < rows; b2++) {
                        run += static_cast<int>((hpw >> (31 - b2)) & 1u) - static_cast<int>((hnw >> (31 - b2)) & 1u);
                        best = run < best ? run : best;
                    }
                }
                score = best;
            }
            out[static_cast<size_t>(q) * ld + static_cast<size_t>(group) * kLanes + lane] = static_cast<int16_t>(-score);
        }
    }
}

namespace {

// ---- the kernel widths: each list is what its family's selection picks from AND what its launcher dispatches on ----
// Resident Peq planes (myers_global_asm_kernel, myers_semi_asm_kernel).  A subject uses the smallest width that holds it
// (extra words are all-zero Peq and masked out of the score).
using PeqWidths = Widths<1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 18, 20, 22, 24, 25, 26, 28, 30, 32>;
using PairWidths = Widths<1, 2>;   // two rows per token and two subject groups per wave (kPairMaxWords)
using BandPairWidths = Widths<3, 4, 5>;   // the certified band with two subject groups per wave (kBandPairMaxWords)
// Code planes (myers_global_planes_kernel).  Below 29 words only BGSA_MYERS_PEQ_MAX_WORDS gets there (resident Peq planes
// measured faster): those widths ship in the A/B flavour.
using PlanesAbWidths = Widths<10, 12, 14, 16, 18, 20, 22, 24, 26, 28>;
using PlanesWidths = Widths<30, 32>;
using SemiPlanesWidths = Widths<26, 28, 30, 32>;   // myers_semi_planes_kernel
// Column blocks with resident Peq planes: 20 words = 238 VGPRs, two waves per SIMD (22 words would need 256).
using PeqBlockWidths = Widths<12, 14, 16, 18, 20>;
// ... on the code planes (BGSA_MYERS_BLOCK_FORM=planes, A/B flavour): 28 words is the widest block that keeps two waves
// per SIMD (32 needs 256 VGPRs: measured 93 vs 168 TCUPS).
using PlaneBlockWidths = Widths<12, 14, 16, 18, 20, 22, 24, 26, 28>;
// The compiler-scheduled kernel (BGSA_MYERS_IMPL=c, A/B flavour).
using CompilerWidths = Widths<1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32>;
static_assert(kPairMaxWords == 2 && kBandPairMaxWords == 5 && kPeqMaxWords == 32 && kSemiPeqMaxWords == 32, "the width lists above restate these");

// Queries per task.  Small enough that the grid has >> 256 CUs x 8 waves of tasks even for a
// few thousand subjects, large enough that the 5*NW Peq loads are noise next to
// q_tile * ref_len * 10 * NW VALU ops.
int pick_q_tile(int nq, int64_t n_wave_tasks, int ref_len, int words)
{
    return pick_query_tile(nq, n_wave_tasks, static_cast<long long>(ref_len) * words, 32);
}

// 0 = generated-asm row loop (default), 1 = compiler-scheduled C++ kernel (A/B and NW > 8).
int myers_impl()
{
    static const int impl = [] {
        const char *e = getenv("BGSA_MYERS_IMPL");
        return (e && e[0] == 'c') ? 1 : 0;
    }();
    return impl;
}

// Subject groups per wave of the two-rows-per-token kernels (<= 64 bp): 2 by default, BGSA_MYERS_PAIR_GROUPS=1 for the A/B.
static int pair_groups()
{
    static const int g = [] {
        const char *e = getenv("BGSA_MYERS_PAIR_GROUPS");
        return (e && e[0] == '1') ? 1 : 2;
    }();
    return g;
}

// Subject groups per wave of the certified band's kernels, 65..160 bp (3..5 words).  Two groups share every dispatch, REFILL,
// SETWIN, stream load and task — the scalar work that the windowed rows spread over 16..32 VALU instructions instead of 40 —
// at five waves per SIMD instead of eight (LABNOTES §19).  BGSA_MYERS_BAND_GROUPS=1|2 forces the choice for every
// banded bucket of at least two groups (A/B; read once); without it the bucket's size decides (kBandPairMinReads).
static int band_groups_knob()
{
    static const int g = [] {
        const char *e = getenv("BGSA_MYERS_BAND_GROUPS");
        return (e && (e[0] == '1' || e[0] == '2') && e[1] == 0) ? e[0] - '0' : 0;
    }();
    return g;
}
// The smallest bucket (subjects) whose banded launch carries two groups per wave by default.  Measured, 2,000 queries x 150 bp,
// kernel ms with one / two groups, two runs each (profiles/r09_band_groups_sweep.txt): 125k subjects 15.34, 15.38 / 15.10, 15.14
// (-1.5 %); 250k 30.43, 30.48 / 29.88, 29.99 (-1.7 %); 500k 60.63, 60.64 / 59.65, 59.33 (-1.9 %); 1M 121.19, 121.01 / 117.76,
// 117.52 (-2.9 %).  No crossover down to 125k: the gain shrinks with the bucket but stays ten times the run-to-run spread.
// Smaller buckets were not measured and keep one group per wave.
constexpr int64_t kBandPairMinReads = 125000;

// Measurement knob: bytes of unused dynamic LDS per workgroup of the counter kernels — caps the waves per SIMD (160 KB of LDS
// per CU: 40960 -> four workgroups = four waves per SIMD).  Round 4 asked whether the 150 bp kernel, which issues at 98 % of
// the sustained clock with eight waves per SIMD, holds a higher clock with fewer (LABNOTES 9.5).
static unsigned myers_lds_pad()
{
    static const unsigned v = [] { const char *e = getenv("BGSA_MYERS_LDS_PAD"); return e ? static_cast<unsigned>(atoi(e)) : 0u; }();
    return v;
}

// Most queries per task of the 30- and 32-word kernels.  A task loads the group's 160 Peq words once and walks its queries, so the
// tile is what the launch's HBM traffic hangs on: 8 (the code-plane kernels' choice: their tasks are long) re-read the 660 B per
// subject 125 times per 1,000 queries — 83 GB per config-5 pass, 9.7 x SURVEY's algorithmic bytes —, 32 a quarter of that.  Neither costs
// time at < 1 % of HBM peak; BGSA_MYERS_LONG_TILE (8 | 16 | 32) is the measurement knob.
static int long_query_tile()
{
    static const int v = [] {
        const char *e = getenv("BGSA_MYERS_LONG_TILE");
        const int t = e ? atoi(e) : 32;
        return (t == 8 || t == 16 || t == 32) ? t : 32;
    }();
    return v;
}

// Column blocks with resident Peq planes: 12..20 words (BGSA_MYERS_BLOCK_FORM=planes selects the
// code-plane blocks of up to 28 words instead, the A/B reference).
bool peq_blocks()
{
    static const bool on = [] {
        const char *e = getenv("BGSA_MYERS_BLOCK_FORM");
        return !(e && strcmp(e, "planes") == 0);
    }();
    return on;
}

// ---- prefix sharing of the band kernels (myers_band.h) ----
// BGSA_MYERS_PREFIX_SHARE (read once): 0 = off; 1 = the default depths under the default rule; a list a,b,c of one to
// kPrefixMaxDepths depths (a single number from 2 up is a list of one) = these depths for every banded launch whose shape
// and tile qualify, whatever its query count (tests, A/B); unset = kPrefixShareDefault.  A list that is too long, not
// ascending, outside 1 .. kPrefixKeyChars or reaching rows that leave words 0..1 turns sharing OFF for the launch — it is
// never cut to fit —, and bgsa_hip_myers_prefix_depths then answers 0.
constexpr bool kPrefixShareDefault = true;
// The fewest queries of a launch that shares by default.  The order costs three small kernels and the segments a few hundred
// cycles per (query, wave); a block of 100 queries shares about two rows.
constexpr int kPrefixMinQueries = 2000;
constexpr int kPrefixMinTile = 16;      // a tile's first query shares nothing
struct PrefixKnob {
    int mode;   // 0 off, 1 default depths, 2 the listed depths
    int n, depth[kPrefixMaxDepths];
};
static const PrefixKnob &prefix_knob()
{
    static const PrefixKnob k = [] {
        PrefixKnob v = {kPrefixShareDefault ? 1 : 0, 0, {}};
        const char *e = getenv("BGSA_MYERS_PREFIX_SHARE");
        if (!e || !*e) return v;
        if (!strchr(e, ',')) {
            const int d = atoi(e);
            if (d <= 0) v.mode = 0;
            else if (d == 1) v.mode = 1;
            else v = {2, 1, {d}};
            return v;
        }
        v = {2, 0, {}};
        for (const char *c = e; c; c = strchr(c, ',') ? strchr(c, ',') + 1 : nullptr) {
            if (v.n == kPrefixMaxDepths) return PrefixKnob{0, 0, {}};   // more depths than slots: off, not cut
            v.depth[v.n++] = atoi(c);
        }
        return v;
    }();
    return k;
}

// The depths of a banded launch of nq queries in tiles of q_tile against read_count subjects (s: its schedule), and its
// segment offsets: p->n = 0 where the launch does not share.  Default depths: d0 - 1, d0, d0 + 1 around d0 = floor(log4 nq), the
// prefix that consecutive queries of a sorted uniform set share, clipped to 1 .. kPrefixKeyChars and to the shape.
void prefix_select(int ref_len, int nw, const BandSchedule &s, int nq, int q_tile, int64_t read_count, PrefixPlan *p)
{
    *p = PrefixPlan{};
    const PrefixKnob &knob = prefix_knob();
    // the order is n^2 comparisons: not where the queries outnumber the subjects many times
    if (knob.mode == 0 || q_tile < kPrefixMinTile || nq < kPrefixMinTile || nq > 8 * read_count) return;
    PrefixPlan want;
    if (knob.mode == 2) {
        want.n = knob.n;
        for (int j = 0; j < knob.n; j++) want.depth[j] = knob.depth[j];
    } else {
        if (nq < kPrefixMinQueries) return;
        int d0 = 0;
        for (long long v = nq; v >= 4; v /= 4) d0++;
        for (int d = d0 - 1; d <= d0 + 1; d++)
            if (d >= 1 && d <= kPrefixKeyChars && d < ref_len) want.depth[want.n++] = d;
        // clipped to the rows on words 0..1: drop the depths behind the first window that leaves them
        while (want.n > 0) {
            PrefixPlan probe = want;
            if (prefix_plan_layout(ref_len, nw, s, &probe)) break;
            want.n--;
        }
    }
    if (prefix_plan_layout(ref_len, nw, s, &want)) *p = want;
}
// LDS of a sharing launch: per workgroup its waves' slots of two words {VP, VN} per group and lane
size_t prefix_lds_bytes(const PrefixPlan &p, int groups) { return static_cast<size_t>(p.n) * kWavesPerBlock * groups * kLanes * sizeof(uint4); }

// The certificate statistics of one band launch into the device's sticky counts (myers_band.h: band_stats_words).
__global__ void band_stats_add_kernel(const unsigned long long *__restrict__ launch, unsigned long long *__restrict__ stats)
{
    atomicAdd(&stats[0], launch[0]);   // launches on other streams may add at the same time
    atomicAdd(&stats[1], launch[1]);
    atomicAdd(&stats[2], launch[2]);   // the rescue's pair (myers_band.h): zero behind a launch that does not rescue
    atomicAdd(&stats[3], launch[3]);
}

// ---- rescue (myers_band.h) ----
// BGSA_MYERS_BAND_RESCUE=0|1 (read once) forces it off or on for every banded launch with two groups per wave (tests, A/B);
// BGSA_MYERS_BAND_RESCUE_POOL=N caps the pool's entries (tests).
constexpr bool kRescueDefault = true;
// The fewest queries of a launch that rescues by default.  The rescue kernel's time has a floor — one lane's full rows, some
// tenths of a millisecond however few the entries — against a gain of about 2 % of the row kernel's 0.057 ms per query and
// million subjects: 100-query launches (the reference's blocks) come out level or behind, LABNOTES §33.5.
constexpr int kRescueMinQueries = 1000;
static int rescue_knob()
{
    static const int v = [] {
        const char *e = getenv("BGSA_MYERS_BAND_RESCUE");
        return (e && (e[0] == '0' || e[0] == '1') && e[1] == 0) ? e[0] - '0' : -1;
    }();
    return v;
}
static long long rescue_pool_knob()
{
    static const long long v = [] {
        const char *e = getenv("BGSA_MYERS_BAND_RESCUE_POOL");
        return e ? atoll(e) : -1ll;
    }();
    return v;
}
// The pool's capacity for a two-group banded launch of nq queries against read_count subjects, 0 where it does not rescue.
// By default: a bucket that carries two groups by its size, at least kRescueMinQueries queries, lengths at which at most 2 in
// 1,000 random pairs are not certified (band_rescue_lengths), and a pool twice what that rate fills.
long long rescue_entries_for(int ref_len, int read_len, int nq, int64_t read_count)
{
    if (read_len < kRescueMinLen || read_len > kRescueMaxLen || nq <= 0 || read_count < 2 * kLanes || read_count > 0x7fffffffll) return 0;
    const long long pool = static_cast<long long>(rescue_pool_bytes(read_len, nq) / sizeof(RescueEntry));
    long long entries = rescue_pool_entries(read_len, nq);
    if (rescue_pool_knob() >= 0 && rescue_pool_knob() < entries) entries = rescue_pool_knob();
    if (rescue_knob() >= 0) return rescue_knob() ? entries : 0;
    if (!kRescueDefault || nq < kRescueMinQueries || read_count < kBandPairMinReads || !band_rescue_lengths(ref_len, read_len)) return 0;
    return 2e-3 * nq * static_cast<double>(read_count) <= static_cast<double>(pool / 2) ? entries : 0;
}
// The half-width and the schedule of a banded launch with `groups` subject groups per wave; *entries = the pool's capacity
// where it rescues (then h is the rescue half-width, or BGSA_MYERS_BAND's), else 0.  A shape whose rescue band has no
// schedule (|n - m| above its B) keeps the default band and does not rescue.
int band_half_for(int ref_len, int read_len, int nw, int groups, int nq, int64_t read_count, BandSchedule *sched, long long *entries)
{
    *entries = groups == 2 && nw <= kBandPairMaxWords ? rescue_entries_for(ref_len, read_len, nq, read_count) : 0;
    if (*entries > 0) {
        const int h = band_half(ref_len, read_len, true);
        if (band_schedule(ref_len, read_len, h, nw, sched)) return h;
        *entries = 0;
    }
    const int h = band_half(ref_len, read_len);
    band_schedule(ref_len, read_len, h, nw, sched);
    return h;
}

// ---- early leave (myers_band.h) ----
// On exactly where the launch rescues by the DEFAULT rule (no BGSA_MYERS_BAND_RESCUE: the tests that force rescue count the
// lanes of the plain rescue band), n = m, and the length has cuts at the launch's half-width.  BGSA_MYERS_BAND_EARLY=0|1 (read
// once) forces it off, or on for every rescuing launch with a table entry.
constexpr bool kEarlyDefault = true;
static int early_knob()
{
    static const int v = [] {
        const char *e = getenv("BGSA_MYERS_BAND_EARLY");
        return (e && (e[0] == '0' || e[0] == '1') && e[1] == 0) ? e[0] - '0' : -1;
    }();
    return v;
}
// The cuts of a two-group launch that rescues (`rescue` entries, half-width h): where it leaves early, *sched becomes the
// schedule with the cuts applied.  Whether the launch shares prefixes makes no difference: the cuts lie behind every depth.
BandCuts early_select(int ref_len, int read_len, int nw, int h, long long rescue, BandSchedule *sched)
{
    if (rescue <= 0 || early_knob() == 0) return BandCuts{};
    if (early_knob() < 0 && (!kEarlyDefault || rescue_knob() >= 0)) return BandCuts{};
    const BandCuts cuts = band_early_cuts(ref_len, read_len, h);
    BandSchedule early;
    if (cuts.n == 0 || !band_schedule_early(ref_len, read_len, h, nw, cuts, &early)) return BandCuts{};
    *sched = early;
    return cuts;
}

// The pool's pairs, one per lane, with full rows: exact by themselves, so no band, no certificate and no stream.  Persistent
// waves read the number of entries on the device and take chunks of 64.  A lane behind the last entry, or on an entry that is
// void or names no pair of the launch, runs pair (0, 0) and stores nothing.
template <int NW>
__global__ __launch_bounds__(256) void myers_band_rescue_kernel(unsigned *__restrict__ words, const char *__restrict__ content,
                                                                const uint32_t *__restrict__ peq, int16_t *__restrict__ out,
                                                                int ref_len, int read_len, long long ld, int word_num, int ref_start,
                                                                int n_queries)
{
    const unsigned long long claimed = *rescue_claimed(words), capacity = *rescue_capacity(words);
    const unsigned long long count = claimed < capacity ? claimed : capacity;
    const RescueEntry *pool = rescue_pool(words);
    const unsigned lane = threadIdx.x & (kLanes - 1);
    const unsigned long long n_waves = static_cast<unsigned long long>(gridDim.x) * kWavesPerBlock;
    unsigned rescued = 0;
    for (unsigned long long chunk = static_cast<unsigned long long>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6);
         chunk * kLanes < count; chunk += n_waves) {
        const unsigned long long at = chunk * kLanes + lane;
        RescueEntry e = pool[at < count ? at : count - 1];
        const bool live = at < count && e.q >= 0 && e.q < n_queries && e.subject >= 0 && e.subject < ld;
        if (!live) e = RescueEntry{0, 0};
        const uint32_t *g = peq + (static_cast<size_t>(e.subject / kLanes) * kChars * word_num) * kLanes + e.subject % kLanes;
        uint32_t P[kChars][NW], pv[NW], mv[NW];
#pragma unroll
        for (int c = 0; c < kChars; c++)
#pragma unroll
            for (int w = 0; w < NW; w++) P[c][w] = w < word_num ? g[(c * word_num + w) * kLanes] : 0u;
#pragma unroll
        for (int w = 0; w < NW; w++) {
            pv[w] = ~0u;
            mv[w] = 0u;
        }
        const unsigned char *row = reinterpret_cast<const unsigned char *>(content) + static_cast<size_t>(ref_start + e.q) * (ref_len + 1);
        for (int r = 0; r < ref_len; r++) {
            unsigned c = row[r];
            if (c > 4) c = 0;   // as the streams: out-of-alphabet bytes behave as 'A'
            uint32_t carry = 0, hp_in = 1, hn_in = 0;   // the row edge of the global mode
#pragma unroll
            for (int w = 0; w < NW; w++) {
                const uint32_t eq = c == 0 ? P[0][w] : c == 1 ? P[1][w] : c == 2 ? P[2][w] : c == 3 ? P[3][w] : P[4][w];
                myers_word(eq, pv[w], mv[w], carry, hp_in, hn_in);
            }
        }
        int score = ref_len;
#pragma unroll
        for (int w = 0; w < NW; w++) {
            const int rem = read_len - 32 * w;
            const uint32_t m = rem >= 32 ? ~0u : (rem <= 0 ? 0u : ((1u << rem) - 1u));
            score += __popc(pv[w] & m) - __popc(mv[w] & m);
        }
        if (live) out[static_cast<size_t>(e.q) * ld + e.subject] = static_cast<int16_t>(-score);
        rescued += __popcll(__builtin_amdgcn_ballot_w64(live));
    }
    if (lane == 0 && rescued) atomicAdd(&band_launch_words(words)[2], static_cast<unsigned long long>(rescued));
}

// Every instantiation of myers_global_asm_kernel through one pointer type (a function pointer has no default arguments: the
// plain kernels get their two band parameters passed as 0 / nullptr).
using AsmKernel = void (*)(const unsigned char *, const uint32_t *, int16_t *, int, int, long long, int, int, int, int, int,
                           unsigned *, unsigned *, int, unsigned long long *, const int32_t *, unsigned long long, const PrefixEntry *);

template <int NW, int G>
int launch_asm(const ScoreArgs &a)
{
    const int nq = a.nq();
    // the widths with registers to spare have a counter instantiation, and so have the split-chain widths (30, 32 words: two
    // waves per SIMD with or without the task loop's registers)
    constexpr bool kCounter = NW <= 8 || NW >= 30;
    constexpr bool kPairs = NW <= kPairMaxWords;
    // two subject groups per wave of the band loop (myers_select: large buckets of 65..160 bp): these widths have no two-group
    // kernel on full-row streams, so the launch is banded or refused
    constexpr bool kBandPair = G == 2 && !kPairs;
    static_assert(!kBandPair || NW <= kBandPairMaxWords, "two groups per wave: the pair kernels, or the band up to 5 words");
    // A mixed-length bucket runs the LENS instantiation, of which a width has ONE: on the counter where the width has a counter
    // kernel (the default selection's choice for every launch long enough to matter; a short launch pays the counter's fixed
    // cost, and BGSA_DYNAMIC_TASKS=0 does not reach it), on the static grid elsewhere.  Full rows always: no band.
    const bool lens = a.d_read_lens != nullptr;
    const int64_t n_waves = (a.n_groups() + G - 1) / G;
    const TaskPlan plan = plan_tasks(nq, n_waves, static_cast<long long>(a.ref_len) * NW * G, NW >= 30 ? 8 : 32, kCounter,
                                     NW >= 30 ? long_query_tile() : query_tile_max(), lens);
    if (lens && kCounter && !plan.dynamic) {
        set_error_text("myers: too many tasks for one length-aware launch (split the query window)");
        return BGSA_HIP_EUNSUPPORTED;
    }
    note_query_tile(plan.q_tile);
    AsmKernel on_grid = nullptr, on_counter = nullptr;
    if constexpr (!kBandPair) {
        on_grid = myers_global_asm_kernel<NW, G, false>;
        if constexpr (kCounter) on_counter = myers_global_asm_kernel<NW, G, true>;
        if (lens) {
            if constexpr (kCounter) on_grid = nullptr, on_counter = myers_global_asm_kernel<NW, G, true, false, true>;
            else on_grid = myers_global_asm_kernel<NW, G, false, false, true>;
        }
    }
    BandSchedule sched;
    PrefixPlan prefix;   // n = 0: the launch packs and runs as ever, on the kernel it ran on before
    int h = 0;
    bool band = false;
    long long rescue = 0;   // the pool's capacity of a launch that rescues (myers_band.h)
    BandCuts cuts;          // ... and where its low words leave early
    if constexpr ((G == 1 || kBandPair) && NW >= kBandMinWords && NW <= kBandMaxWords) {   // the certified band (myers_band.h)
        if (!lens) h = band_half_for(a.ref_len, a.read_len, NW, G, nq, a.read_count, &sched, &rescue);
        band = !lens && sched.n > 0;
        if (band) {
            on_grid = myers_global_asm_kernel<NW, G, false, true>;
            on_counter = myers_global_asm_kernel<NW, G, true, true>;
            if constexpr (kBandPair) cuts = early_select(a.ref_len, a.read_len, NW, h, rescue, &sched);
            prefix_select(a.ref_len, NW, sched, nq, plan.q_tile, a.read_count, &prefix);
            if (prefix.n) {
                on_grid = myers_global_asm_kernel<NW, G, false, true, false, true>;
                on_counter = myers_global_asm_kernel<NW, G, true, true, false, true>;
            }
            if constexpr (kBandPair) {
                if (rescue > 0) {
                    on_grid = prefix.n ? myers_global_asm_kernel<NW, G, false, true, false, true, true>
                                       : myers_global_asm_kernel<NW, G, false, true, false, false, true>;
                    on_counter = prefix.n ? myers_global_asm_kernel<NW, G, true, true, false, true, true>
                                          : myers_global_asm_kernel<NW, G, true, true, false, false, true>;
                }
            }
        }
    }
    if (band && 2 * h + 1 > kBandEarlyLimitMask) {   // (no schedule has such a band: band_early_word keeps ten bits of it)
        set_error_text("myers band: half-width out of range");
        return BGSA_HIP_EINVAL;
    }
    if (kBandPair && !band) {   // myers_band_groups answers 2 for banded launches only
        set_error_text("myers: two subject groups per wave selected for a launch without the certified band");
        return BGSA_HIP_EUNSUPPORTED;
    }
    const unsigned lds = (plan.dynamic ? myers_lds_pad() : 0u) + static_cast<unsigned>(prefix_lds_bytes(prefix, G));
    const int stride = static_cast<int>(prefix.n  ? static_cast<size_t>(prefix.off[prefix.n + 1])
                                        : band    ? band_stream_stride(a.ref_len)
                                        : kPairs  ? pair_stream_stride(a.ref_len)
                                                  : stream_stride(a.ref_len));
    // the task counter sits behind the streams, and the band's guard pair 64 bytes further (both inside the kTaskCounterBytes
    // the workspace reserves); the packer zeroes them
    unsigned *words = task_counter_in(a.d_workspace, static_cast<size_t>(stride) * nq);
    LaunchGrid lg;
    if (int rc = plan_grid(plan, n_waves, nq, words,
                           [&] { return on_counter ? persistent_blocks_for(on_counter, lds) : persistent_blocks(); }, "myers", &lg))
        return rc;
    if (prefix.n)
        if (int rc = launch_prefix_order(a.d_content, a.ref_len, a.ref_start, a.ref_end, plan.q_tile, prefix, words, a.stream))
            return rc;
    if (int rc = prefix.n ? launch_pack_band_segments(a.d_content, a.ref_len, sched, prefix, a.ref_start, a.ref_end, a.d_workspace, a.stream, words,
                                                       static_cast<unsigned>(rescue))
                 : band   ? launch_pack_band(a.d_content, a.ref_len, sched, a.ref_start, a.ref_end, a.d_workspace, a.stream, words,
                                             static_cast<unsigned>(rescue))
                 : kPairs ? launch_pack_query_pairs(a.d_content, a.ref_len, a.ref_start, a.ref_end, a.d_workspace, a.stream, lg.counter)
                          : launch_pack_queries(a.d_content, a.ref_len, a.ref_start, a.ref_end, a.d_workspace, a.stream, lg.counter))
        return rc;
    unsigned *fault = nullptr;
    if (int rc = stream_guard(a.d_workspace, stride, kPairs ? kPairRefill : kCodeRefill, band ? kBandBadCode : kPairs ? -1 : 7, a.stream, &fault))
        return rc;
    unsigned long long *guard = band ? band_launch_words(words) : nullptr;
    const AsmKernel kernel = lg.counter ? on_counter : on_grid;
    hipLaunchKernelGGL(kernel, lg.grid, dim3(256), lds, a.stream,
                       static_cast<const unsigned char *>(a.d_workspace), a.d_peq, a.results<int16_t>(), a.ref_len, a.read_len,
                       static_cast<long long>(a.read_count), static_cast<int>(a.n_groups()), a.word_num, nq, plan.q_tile, stride,
                       fault, lg.counter, band ? band_early_word(2 * h + 1, cuts) : 0, guard, a.d_read_lens, prefix_segments_word(prefix),
                       static_cast<const PrefixEntry *>(prefix_entries(words)));
    BGSA_HIP_TRY(hipGetLastError());
    if constexpr (kBandPair) {
        if (rescue > 0) {   // unconditionally: how many entries there are is read on the device
            hipLaunchKernelGGL(myers_band_rescue_kernel<NW>, dim3(persistent_blocks()), dim3(256), 0, a.stream, words, a.d_content, a.d_peq,
                               a.results<int16_t>(), a.ref_len, a.read_len, static_cast<long long>(a.read_count), a.word_num,
                               a.ref_start, nq);
            BGSA_HIP_TRY(hipGetLastError());
        }
    }
    if (band) {
        hipLaunchKernelGGL(band_stats_add_kernel, dim3(1), dim3(1), 0, a.stream, static_cast<const unsigned long long *>(guard),
                           band_stats_words(fault));
        BGSA_HIP_TRY(hipGetLastError());
    }
    return BGSA_HIP_OK;
}

// LENS: the bucket's per-column lengths go to the kernel (launch_myers_place_lens); tile and grid are planned as without them.
template <int NW, bool LENS = false>
int launch_semi_asm(const ScoreArgs &a)
{
    const int nq = a.nq(), stride = static_cast<int>(stream_stride(a.ref_len));
    const int q_tile = pick_q_tile(nq, a.n_groups(), a.ref_len, NW);
    note_query_tile(q_tile);
    LaunchGrid lg;
    if (int rc = plan_grid({q_tile, false}, a.n_groups(), nq, nullptr, no_counter_kernel, "myers", &lg)) return rc;
    if (int rc = launch_pack_queries(a.d_content, a.ref_len, a.ref_start, a.ref_end, a.d_workspace, a.stream)) return rc;
    unsigned *fault = nullptr;
    if (int rc = stream_guard(a.d_workspace, stride, kCodeRefill, 7, a.stream, &fault)) return rc;
    hipLaunchKernelGGL((myers_semi_asm_kernel<NW, LENS>), lg.grid, dim3(256), 0, a.stream,
                       static_cast<const unsigned char *>(a.d_workspace), a.d_peq, a.results<int16_t>(), a.ref_len,
                       a.read_len, static_cast<long long>(a.read_count), static_cast<int>(a.n_groups()), a.word_num,
                       nq, q_tile, stride, fault, LENS ? a.d_read_lens : nullptr);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

template <int NW, bool SEMI = false>
int launch_planes(const ScoreArgs &a)
{
    const int nq = a.nq(), stride = static_cast<int>(stream_stride(a.ref_len));
    // a task is already long: 8 queries x ref_len rows x 11*NW instructions.  Counter: two waves per SIMD with or without the
    // loop's registers from 26 words up; narrower A/B widths keep theirs
    const TaskPlan plan = plan_tasks(nq, a.n_groups(), static_cast<long long>(a.ref_len) * NW, 8, !SEMI && NW >= 26);
    note_query_tile(plan.q_tile);
    LaunchGrid lg;
    if (int rc = plan_grid(plan, a.n_groups(), nq, task_counter_in(a.d_workspace, static_cast<size_t>(stride) * nq),
                           [] { if constexpr (SEMI) return 0; else return persistent_blocks_for(myers_global_planes_kernel<NW, true>); },
                           "myers", &lg))
        return rc;
    if (int rc = launch_pack_queries(a.d_content, a.ref_len, a.ref_start, a.ref_end, a.d_workspace, a.stream, lg.counter)) return rc;
    unsigned *fault = nullptr;
    if (int rc = stream_guard(a.d_workspace, stride, kCodeRefill, 7, a.stream, &fault)) return rc;
    if constexpr (SEMI)
        hipLaunchKernelGGL((myers_semi_planes_kernel<NW>), lg.grid, dim3(256), 0, a.stream,
                           static_cast<const unsigned char *>(a.d_workspace), a.d_peq, a.results<int16_t>(), a.ref_len,
                           a.read_len, static_cast<long long>(a.read_count), static_cast<int>(a.n_groups()), a.word_num,
                           nq, plan.q_tile, stride, fault);
    else {
        auto kernel = lg.counter ? myers_global_planes_kernel<NW, true> : myers_global_planes_kernel<NW, false>;
        hipLaunchKernelGGL(kernel, lg.grid, dim3(256), 0, a.stream, static_cast<const unsigned char *>(a.d_workspace), a.d_peq,
                           a.results<int16_t>(), a.ref_len, a.read_len, static_cast<long long>(a.read_count),
                           static_cast<int>(a.n_groups()), a.word_num, nq, plan.q_tile, stride, fault, lg.counter);
    }
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

template <int NW, bool PEQ = false, bool SEMI = false>
int launch_blocked(const ScoreArgs &a, int n_blocks)
{
    const int nq = a.nq();
    const int stride = blocked_stream_layout(a.ref_len, nullptr, nullptr);
    const size_t stream_bytes = (static_cast<size_t>(stride) * nq + 255) & ~static_cast<size_t>(255);
    if (int rc = launch_pack_blocked(a.d_content, a.ref_len, a.ref_start, a.ref_end, a.d_workspace, a.stream)) return rc;
    uint32_t *carry = reinterpret_cast<uint32_t *>(static_cast<unsigned char *>(a.d_workspace) + stream_bytes);
    unsigned long long *counter = reinterpret_cast<unsigned long long *>(
        reinterpret_cast<unsigned char *>(carry) + blocked_carry_bytes(a.ref_len, 3));
    BGSA_HIP_TRY(hipMemsetAsync(counter, 0, sizeof(unsigned long long), a.stream));
    unsigned *fault = nullptr;
    if (int rc = stream_guard(a.d_workspace, stride, kCodeRefill, -1, a.stream, &fault)) return rc;
    const int q_tile = blocked_q_tile(nq, a.n_groups());
    note_query_tile(q_tile);
    hipLaunchKernelGGL((myers_blocked_kernel<NW, PEQ, SEMI>), dim3(blocked_workgroups()), dim3(256), 0, a.stream,
                       static_cast<const unsigned char *>(a.d_workspace), a.d_peq, a.results<int16_t>(), carry, a.ref_len,
                       a.read_len, static_cast<long long>(a.read_count), static_cast<int>(a.n_groups()), a.word_num, nq,
                       q_tile, stride, n_blocks, counter, fault);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

#if BGSA_AB_KERNELS
template <int NW, int G, bool SEMI = false>
int launch_nw(const ScoreArgs &a)
{
    const int64_t n_waves = (a.n_groups() + G - 1) / G;
    const int q_tile = pick_q_tile(a.nq(), n_waves, a.ref_len, NW * G);
    note_query_tile(q_tile);
    LaunchGrid lg;
    if (int rc = plan_grid({q_tile, false}, n_waves, a.nq(), nullptr, no_counter_kernel, "myers", &lg)) return rc;
    hipLaunchKernelGGL((myers_global_kernel<NW, G, SEMI>), lg.grid, dim3(256), 0, a.stream, a.d_content, a.d_peq,
                       a.results<int16_t>(), a.ref_len, a.read_len, static_cast<long long>(a.read_count),
                       static_cast<int>(a.n_groups()), a.word_num, a.ref_start, a.ref_end, q_tile);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}
#endif

}  // namespace

int myers_max_plain_words()
{
    static const int limit = [] {
        const char *e = getenv("BGSA_MYERS_MAX_PLAIN_WORDS");   // measurement knob
        const int v = e ? atoi(e) : kMaxWords;
        return (v >= 8 && v <= kMaxWords) ? v : kMaxWords;
    }();
    return limit;
}

// Widest subject (words) that keeps its five Peq planes in registers (8 VALU per word); wider ones use
// the 3-bit code planes (9 per word, fewer registers).  BGSA_MYERS_PEQ_MAX_WORDS overrides (measurement).
int myers_peq_max_words()
{
    static const int limit = [] {
        const char *e = getenv("BGSA_MYERS_PEQ_MAX_WORDS");
        const int v = e ? atoi(e) : kPeqMaxWords;
        return (v >= 8 && v <= 32) ? v : kPeqMaxWords;
    }();
    return limit;
}

// Semi-global: widest subject (words) scored without column blocks — resident Peq planes (myers_semi_asm_kernel) up
// to myers_peq_max_words(), the code planes (myers_semi_planes_kernel) up to 32 words; wider ones run as column blocks.
int myers_semi_max_plain_words() { return 32; }

namespace {

// ---- which kernel scores a launch: decided here, once; launch_myers switches on the answer, myers_kernel_name formats it ----
enum class MyersFamily {
    kAsm,            // myers_global_asm_kernel<nw, 1>: resident Peq planes (the certified band where it applies)
    kAsmPairs,       // myers_global_asm_kernel<nw, 2>: <= 64 bp, two rows per token, two subject groups per wave
    kAsmBandPairs,   // myers_global_asm_kernel<nw, 2>: 65..160 bp, the certified band with two subject groups per wave (large buckets)
    kSemiAsm,        // myers_semi_asm_kernel<nw>
    kPlanes,         // myers_global_planes_kernel<nw>
    kSemiPlanes,     // myers_semi_planes_kernel<nw>
    kBlockedPeq,     // myers_blocked_kernel<nw, true> / <nw, true, true>: n_blocks column blocks, resident Peq planes
    kBlockedPlanes,  // myers_blocked_kernel<nw>: ... on the code planes
    kCompiler,       // myers_global_kernel<nw, 1> / <nw, 1, true>: compiler-scheduled (BGSA_MYERS_IMPL=c)
    kStateInMemory,  // myers_long_kernel (long_kernels.hip): BGSA_MYERS_IMPL=c beyond the register-resident limit
};
struct MyersChoice {
    MyersFamily family;
    int nw, G, n_blocks;
    bool semi;
    const char *refused;   // not nullptr: this flavour of the library does not carry that kernel — the knob, as ab_knob_refused names it
};

// Groups per wave of a launch on resident Peq planes of width nw (global mode): 2 where the certified band applies to these
// lengths, the width has a two-group band loop and the bucket is large enough (or BGSA_MYERS_BAND_GROUPS says so); else 1.
// Lengths 0 (bgsa_hip_kernel_name: no launch in sight) answer 1, and so does its bucket of 128 reads: the name is the
// small-bucket kernel's.
int band_groups_for(int nw, int64_t read_count, int ref_len, int read_len, bool mixed_lengths)
{
    if (nw < kBandMinWords || nw > kBandPairMaxWords || mixed_lengths || read_count < 2 * kLanes || ref_len <= 0 || read_len <= 0) return 1;
    BandSchedule sched;
    if (!band_schedule(ref_len, read_len, band_half(ref_len, read_len), nw, &sched)) return 1;
    if (band_groups_knob()) return band_groups_knob();
    return read_count >= kBandPairMinReads ? 2 : 1;
}

// Precedence: BGSA_MYERS_IMPL=c first; then the alignment mode; global subjects beyond BGSA_MYERS_MAX_PLAIN_WORDS run as
// column blocks in the form BGSA_MYERS_BLOCK_FORM names; the others on resident Peq planes up to BGSA_MYERS_PEQ_MAX_WORDS
// (<= 64 bp: two groups per wave unless BGSA_MYERS_PAIR_GROUPS=1 or the bucket has one group only; 65..160 bp: band_groups_for) and on
// the code planes beyond.
MyersChoice myers_select(int word_num, int semi, int64_t read_count, int ref_len = 0, int read_len = 0, bool mixed_lengths = false)
{
    auto ab_only = [](const char *knob) -> const char * { return BGSA_AB_KERNELS ? nullptr : knob; };   // kernels of the A/B flavour
    MyersChoice c = {MyersFamily::kAsm, -1, 1, 0, semi != 0, nullptr};
    const bool c_impl = myers_impl() == 1;
    const int peq_max = semi ? std::min(myers_peq_max_words(), kSemiPeqMaxWords) : myers_peq_max_words();
    if (!semi && word_num > myers_max_plain_words()) {
        c.family = peq_blocks() ? MyersFamily::kBlockedPeq : MyersFamily::kBlockedPlanes;
        c.nw = peq_blocks() ? PeqBlockWidths::pick_blocks(word_num, &c.n_blocks) : PlaneBlockWidths::pick_blocks(word_num, &c.n_blocks);
        if (!peq_blocks()) c.refused = ab_only("BGSA_MYERS_BLOCK_FORM=planes");
        if (c_impl) {   // keeps nw: bgsa_hip_kernel_name has always answered with the column-block kernel it stands in for
            c.family = MyersFamily::kStateInMemory;
            c.refused = ab_only("BGSA_MYERS_IMPL=c");
        }
    } else if (c_impl) {
        c.family = MyersFamily::kCompiler;
        c.nw = CompilerWidths::pick(word_num);   // -1 beyond 1024 bp (semi-global only: global subjects went above)
        c.refused = ab_only("BGSA_MYERS_IMPL=c");
    } else if (word_num <= peq_max) {
        c.nw = PeqWidths::pick(word_num);
        if (semi)
            c.family = MyersFamily::kSemiAsm;
        else if (word_num <= kPairMaxWords && pair_groups() == 2 && read_count >= 2 * kLanes) {
            c.family = MyersFamily::kAsmPairs;
            c.G = 2;
        } else if (band_groups_for(c.nw, read_count, ref_len, read_len, mixed_lengths) == 2) {
            c.family = MyersFamily::kAsmBandPairs;
            c.G = 2;
        }
    } else if (semi && word_num > myers_semi_max_plain_words()) {
        c.family = MyersFamily::kBlockedPeq;
        c.nw = PeqBlockWidths::pick_blocks(word_num, &c.n_blocks);
    } else if (semi) {
        c.family = MyersFamily::kSemiPlanes;
        c.nw = SemiPlanesWidths::pick(word_num);
    } else {
        c.family = MyersFamily::kPlanes;
        c.nw = Join<PlanesAbWidths, PlanesWidths>::pick(word_num);
        if (!PlanesWidths::has(c.nw)) c.refused = ab_only("BGSA_MYERS_PEQ_MAX_WORDS");
    }
    return c;
}

}  // namespace

int myers_band_groups(int word_num, int64_t read_count, int ref_len, int read_len, int mixed_lengths)
{
    if (word_num < 1 || word_num > kMaxWords) return 1;
    const MyersChoice c = myers_select(word_num, 0, read_count, ref_len, read_len, mixed_lengths != 0);
    return c.family == MyersFamily::kAsmBandPairs ? 2 : 1;
}

int myers_prefix_depths(int word_num, int64_t read_count, int ref_len, int read_len, int n_queries, int mixed_lengths, int *depths)
{
    if (word_num < 1 || word_num > kMaxWords || n_queries < 1) return 0;
    const MyersChoice c = myers_select(word_num, 0, read_count, ref_len, read_len, mixed_lengths != 0);
    if ((c.family != MyersFamily::kAsm && c.family != MyersFamily::kAsmBandPairs) || mixed_lengths) return 0;
    BandSchedule sched;
    long long rescue = 0;
    band_half_for(ref_len, read_len, c.nw, c.G, n_queries, read_count, &sched, &rescue);
    if (sched.n == 0) return 0;
    // the tile launch_asm picks for the band widths (3..8 words: a counter kernel, tiles up to query_tile_max())
    const int64_t n_waves = (read_count / kLanes + c.G - 1) / c.G;
    const TaskPlan plan = plan_tasks(n_queries, n_waves, static_cast<long long>(ref_len) * c.nw * c.G, 32, true, query_tile_max());
    PrefixPlan p;
    prefix_select(ref_len, c.nw, sched, n_queries, plan.q_tile, read_count, &p);
    for (int j = 0; j < p.n; j++) depths[j] = p.depth[j];
    return p.n;
}

int myers_band_early(int ref_len, int read_len, int n_queries, int64_t read_count, int *rows, int *words)
{
    if (ref_len <= 0 || read_len <= 0 || n_queries < 1 || read_count < 1) return 0;
    const int word_num = (read_len + 31) / 32;
    if (word_num > kMaxWords) return 0;
    const MyersChoice c = myers_select(word_num, 0, read_count, ref_len, read_len, false);
    if (c.family != MyersFamily::kAsmBandPairs) return 0;
    BandSchedule sched;
    long long rescue = 0;
    const int h = band_half_for(ref_len, read_len, c.nw, c.G, n_queries, read_count, &sched, &rescue);
    if (sched.n == 0) return 0;
    const BandCuts cuts = early_select(ref_len, read_len, c.nw, h, rescue, &sched);
    for (int j = 0; j < cuts.n; j++) {
        if (rows) rows[j] = cuts.row[j];
        if (words) words[j] = cuts.word[j];
    }
    return cuts.n;
}

int myers_band_rescue(int ref_len, int read_len, int n_queries, int64_t read_count)
{
    if (ref_len <= 0 || read_len <= 0 || n_queries < 1 || read_count < 1) return 0;
    const int word_num = (read_len + 31) / 32;
    if (word_num > kMaxWords) return 0;
    const MyersChoice c = myers_select(word_num, 0, read_count, ref_len, read_len, false);
    if (c.family != MyersFamily::kAsmBandPairs) return 0;
    BandSchedule sched;
    long long rescue = 0;
    const int h = band_half_for(ref_len, read_len, c.nw, c.G, n_queries, read_count, &sched, &rescue);
    return rescue > 0 ? h : 0;
}

const char *myers_kernel_name(int word_num, int semi_global)
{
    static thread_local char name[64];
    const MyersChoice c = myers_select(word_num, semi_global, 2 * kLanes);   // "at least two groups": see bgsa_common.h
    switch (c.family) {
    case MyersFamily::kAsm:
    case MyersFamily::kAsmBandPairs:
    case MyersFamily::kAsmPairs: snprintf(name, sizeof name, "myers_global_asm_kernel<%d, %d>", c.nw, c.G); break;
    case MyersFamily::kSemiAsm: snprintf(name, sizeof name, "myers_semi_asm_kernel<%d>", c.nw); break;
    case MyersFamily::kPlanes: snprintf(name, sizeof name, "myers_global_planes_kernel<%d>", c.nw); break;
    case MyersFamily::kSemiPlanes: snprintf(name, sizeof name, "myers_semi_planes_kernel<%d>", c.nw); break;
    case MyersFamily::kStateInMemory:   // named after the column blocks of the selected form (myers_select)
        snprintf(name, sizeof name, peq_blocks() ? "myers_blocked_kernel<%d, true>" : "myers_blocked_kernel<%d>", c.nw);
        break;
    case MyersFamily::kBlockedPeq: snprintf(name, sizeof name, c.semi ? "myers_blocked_kernel<%d, true, true>" : "myers_blocked_kernel<%d, true>", c.nw); break;
    case MyersFamily::kBlockedPlanes: snprintf(name, sizeof name, "myers_blocked_kernel<%d>", c.nw); break;
    case MyersFamily::kCompiler: snprintf(name, sizeof name, c.semi ? "myers_global_kernel<%d, 1, true>" : "myers_global_kernel<%d, 1>", c.nw); break;
    }
    return name;
}

int launch_myers(const ScoreArgs &a, int semi_global)
{
    if (a.ref_end <= a.ref_start || a.read_count == 0) return BGSA_HIP_OK;
    const MyersChoice c = myers_select(a.word_num, semi_global, a.read_count, a.ref_len, a.read_len, a.d_read_lens != nullptr);
    if (c.refused) return ab_knob_refused(c.refused);
    if (a.d_read_lens && c.family != MyersFamily::kAsm && c.family != MyersFamily::kAsmPairs) {   // (never kAsmBandPairs: no band on mixed lengths)
        set_error_text("myers: per-subject lengths are scored by myers_global_asm_kernel only (global mode, word_num <= 32, no "
                       "BGSA_MYERS_IMPL / BGSA_MYERS_PEQ_MAX_WORDS / BGSA_MYERS_MAX_PLAIN_WORDS alternative)");
        return BGSA_HIP_EUNSUPPORTED;
    }
    switch (c.family) {
    case MyersFamily::kAsm:
        return PeqWidths::dispatch(c.nw, "myers_global_asm_kernel", [&](auto nw) { return launch_asm<decltype(nw)::value, 1>(a); });
    case MyersFamily::kAsmPairs:
        return PairWidths::dispatch(c.nw, "myers_global_asm_kernel (pairs)", [&](auto nw) { return launch_asm<decltype(nw)::value, 2>(a); });
    case MyersFamily::kAsmBandPairs:
        return BandPairWidths::dispatch(c.nw, "myers_global_asm_kernel (band, two groups)", [&](auto nw) { return launch_asm<decltype(nw)::value, 2>(a); });
    case MyersFamily::kSemiAsm:
        return PeqWidths::dispatch(c.nw, "myers_semi_asm_kernel", [&](auto nw) { return launch_semi_asm<decltype(nw)::value>(a); });
    case MyersFamily::kPlanes:
        return Join<AbOnly<PlanesAbWidths>, PlanesWidths>::dispatch(c.nw, "myers_global_planes_kernel",
                                                                   [&](auto nw) { return launch_planes<decltype(nw)::value>(a); });
    case MyersFamily::kSemiPlanes:
        return SemiPlanesWidths::dispatch(c.nw, "myers_semi_planes_kernel", [&](auto nw) { return launch_planes<decltype(nw)::value, true>(a); });
    case MyersFamily::kBlockedPeq:
        return PeqBlockWidths::dispatch(c.nw, "myers_blocked_kernel (Peq planes)", [&](auto nw) {
            return c.semi ? launch_blocked<decltype(nw)::value, true, true>(a, c.n_blocks) : launch_blocked<decltype(nw)::value, true>(a, c.n_blocks);
        });
    case MyersFamily::kBlockedPlanes:
        return AbOnly<PlaneBlockWidths>::dispatch(c.nw, "myers_blocked_kernel (code planes)",
                                                  [&](auto nw) { return launch_blocked<decltype(nw)::value>(a, c.n_blocks); });
#if BGSA_AB_KERNELS   // (the default flavour was refused above)
    case MyersFamily::kCompiler:
        if (c.nw < 0) {
            set_error_text("myers: the compiler-scheduled semi-global kernel (BGSA_MYERS_IMPL=c) covers subjects up to 1024 bp");
            return BGSA_HIP_EUNSUPPORTED;
        }
        return CompilerWidths::dispatch(c.nw, "myers_global_kernel", [&](auto nw) {
            return c.semi ? launch_nw<decltype(nw)::value, 1, true>(a) : launch_nw<decltype(nw)::value, 1>(a);
        });
    case MyersFamily::kStateInMemory: return launch_long(BGSA_ALGO_MYERS, a);
#endif
    default: break;
    }
    set_error_text("myers: no kernel for this word count");
    return BGSA_HIP_EUNSUPPORTED;
}

int launch_myers_place_lens(const ScoreArgs &a)
{
    if (a.ref_end <= a.ref_start || a.read_count == 0) return BGSA_HIP_OK;
    const MyersChoice c = myers_select(a.word_num, 1, a.read_count, a.ref_len, a.read_len, true);
    if (!a.d_read_lens || c.family != MyersFamily::kSemiAsm) {
        set_error_text("myers: per-read lengths in semi-global mode are scored by myers_semi_asm_kernel only (word_num <= 32, no "
                       "BGSA_MYERS_IMPL / BGSA_MYERS_PEQ_MAX_WORDS alternative)");
        return BGSA_HIP_EUNSUPPORTED;
    }
    return PeqWidths::dispatch(c.nw, "myers_semi_asm_kernel (per-lane lengths)",
                               [&](auto nw) { return launch_semi_asm<decltype(nw)::value, true>(a); });
}

}  // namespace bgsa
