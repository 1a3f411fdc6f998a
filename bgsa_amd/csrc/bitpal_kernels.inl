// bitpal_kernels.inl — the BitPAl kernels and launchers of ONE score set.  Included by a generated
// translation unit (_gen/bitpal_set_<tag>.hip, gen_bitpal_sets.py) inside `namespace bgsa::<set>`,
// right after that set's generated row loops (bitpal_rows_gen.inc for the default 2/-3/-5, or
// _gen/bitpal_rows_<tag>.inc), which define kBitpalPlanes, kBitpalChains, kBitpalGap, kBitpalWeights,
// the width lists and bitpal_rows_asm<NW> / bitpal_block_rows_asm<NW>.
//
// Replaces the reference's align_avx hot loop (original/BGSA_AVX2/align_core.c:164-482 for the
// committed 2/-3/-5 instance; generator/.../BitPAlGenerator.java:151-534 for any other scores).
// Same decomposition as myers_global.hip: lane = subject, wave = group of 64, the wave keeps its
// Peq block in VGPRs and walks a tile of queries; the row loop is generated threaded-code asm
// (rows_ir.py: bitpal_body), every inter-word carry a VCC add-with-carry chain on full 32-bit words.
//
// Final score (align_core.c:433-471 generalised): gap*(qlen + slen) + sum over subject columns of
// u = dH - gap, i.e. one masked popcount per plane and word, weighted 2^plane (kBitpalWeights).

template <int NW>
__device__ __forceinline__ int bitpal_column_sum(const uint32_t *st, int first_word, int read_len)
{
    int sum = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
        const int rem = read_len - 32 * (first_word + w);
        const uint32_t m = rem >= 32 ? ~0u : (rem <= 0 ? 0u : ((1u << rem) - 1u));
#pragma unroll
        for (int i = 0; i < kBitpalPlanes; i++) sum += kBitpalWeights[i] * __popc(st[w * kBitpalPlanes + i] & m);
    }
    return sum;
}

// Semi-global (generator option -s, BitPAlGenerator.java:78-116): walk the last DP row one subject
// column at a time, run = S[m][j], best = the maximum so far.  Once per (query, subject) pair — about
// 3 % of the row loop's work at 150 bp.
template <int NW>
__device__ __forceinline__ void bitpal_last_row_max(const uint32_t *st, int first_word, int read_len, int &run, int &best)
{
#pragma unroll
    for (int w = 0; w < NW; w++) {
        int cols = read_len - 32 * (first_word + w);
        cols = cols > 32 ? 32 : cols;
        for (int j = 0; j < cols; j++) {   // cols is wave-uniform
            int u = 0;
#pragma unroll
            for (int i = 0; i < kBitpalPlanes; i++) u += kBitpalWeights[i] * static_cast<int>((st[w * kBitpalPlanes + i] >> j) & 1u);
            run += u + kBitpalGap;
            best = run > best ? run : best;
        }
    }
}

// Row 0 of the DP: dH = gap everywhere (global: u = 0) or dH = 0 (semi-global: u = -gap,
// writeBitInitStr, BitPAlGenerator.java:2201-2218).  The planes hold u itself, unsigned.
__device__ __forceinline__ uint32_t bitpal_init_plane(int plane, int semi)
{
    constexpr uint32_t stored = static_cast<uint32_t>(-kBitpalGap);
    return (semi && ((stored >> plane) & 1u)) ? ~0u : 0u;
}

// LENS (global mode, a bucket of mixed subject lengths): the rows run over the padded width as ever; the lane's score is the
// column sum under the mask of its OWN length read_lens[column], and the constant term uses that length (column j of a global
// DP depends on columns <= j only).  A separate instantiation, so that the equal-length kernels keep their register counts.
template <int NW, bool SEMI, bool DYN = false, bool LENS = false>
__global__ __launch_bounds__(256) void bitpal_asm_kernel(
    const unsigned char *__restrict__ streams, const uint32_t *__restrict__ peq,
    int16_t *__restrict__ out, int ref_len, int read_len, long long ld, int n_groups, int word_num,
    int n_queries, int q_tile, int stream_stride_bytes, unsigned *__restrict__ fault_word,
    unsigned *__restrict__ task_counter, const int32_t *__restrict__ read_lens = nullptr)
{
    static_assert(!(LENS && SEMI), "semi-global walks the last row over a wave-uniform column count");
    constexpr int semi = SEMI;
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

        uint32_t P[kChars][NW];
        // In the task loop of the DYN instantiation everything that does not depend on the task is loop-invariant, and the
        // compiler keeps it in VGPRs across the row loop: five "word exists" flags and the two per-lane base pointers — ten
        // registers, 103 instead of 93 at five words, the 150 bp kernel's fifth wave per SIMD.  Values laundered through an
        // empty asm are redefined per task as far as the compiler can tell, so they are recomputed (a handful of scalar
        // instructions per task) instead of kept.
        int wn = word_num;
        const uint32_t *peq_t = peq;
        int16_t *out_t = out;
        unsigned lane_t = static_cast<unsigned>(lane);
        if constexpr (DYN) asm volatile("" : "+s"(wn), "+s"(peq_t), "+s"(out_t), "+v"(lane_t));
        const uint32_t *g = peq_t + static_cast<size_t>(group) * kChars * wn * kLanes + lane_t;
#pragma unroll
        for (int c = 0; c < kChars; c++)
#pragma unroll
            for (int w = 0; w < NW; w++)
                P[c][w] = (w < wn) ? g[(c * wn + w) * kLanes] : 0u;
        int n_cols = read_len;   // LENS: the lane's own length, loaded once per task
        if constexpr (LENS) n_cols = lane_read_len(read_lens, static_cast<size_t>(group) * kLanes + lane_t, read_len);

        const int q0 = tile * q_tile;
        const int q1 = (q0 + q_tile < n_queries) ? q0 + q_tile : n_queries;
        // (the store address is formed at the store from this wave-uniform base and the lane: a per-lane 64-bit pointer kept
        // across the row loop is two more registers)
        int16_t *dst = out_t + static_cast<size_t>(group) * kLanes;

        for (int q = q0; q < q1; q++) {
            if constexpr (DYN) {   // the next task, asked for under this one's last query: late enough that the tail of a
                if (q == q1 - 1) task_issued = issue_wave_task(task_counter);   // launch is handed out as waves free up, early enough that the round trip is hidden
            }
            uint32_t st[kBitpalPlanes * NW];
#pragma unroll
            for (int i = 0; i < kBitpalPlanes * NW; i++) st[i] = bitpal_init_plane(i % kBitpalPlanes, semi);  // (:167-171)
            const unsigned long long s =
                reinterpret_cast<unsigned long long>(streams) + static_cast<unsigned long long>(q) * stream_stride_bytes;
            note_stream_fault(fault_word, bitpal_rows_asm<NW>(st, P, uniform_u64(s),
                                                              __builtin_amdgcn_readfirstlane(stream_stride_bytes / 8 - 2)));
            int score;
            if (semi) {
                int run = kBitpalGap * ref_len;
                score = run;
                bitpal_last_row_max<NW>(st, 0, read_len, run, score);
            } else {
                int n_own = n_cols;   // (laundered: the per-word masks are otherwise formed once per task and kept, NW more VGPRs)
                if constexpr (LENS) asm volatile("" : "+v"(n_own));
                score = kBitpalGap * (ref_len + n_own) + bitpal_column_sum<NW>(st, 0, n_own);
            }
            unsigned lane_s = static_cast<unsigned>(lane);
            if constexpr (DYN) asm volatile("" : "+v"(lane_s));      // (the lane's byte offset is formed here, not kept)
            dst[static_cast<size_t>(q) * ld + lane_s] = static_cast<int16_t>(score);
        }
        if constexpr (DYN) task = resolve_wave_task(task_issued);
    } while (DYN && task < n_tasks);
}

// Subjects wider than kBitpalMaxPlain words: column blocks of NW words, the carry chains of a row
// crossing block boundaries through per-wave carry words (same scheme as myers_blocked_kernel;
// rows_ir.py: make_blocked, CPU-simulated in tests/test_rows_ir.py).
template <int NW, bool SEMI>
__global__ __launch_bounds__(256) void bitpal_blocked_kernel(
    const unsigned char *__restrict__ streams, const uint32_t *__restrict__ peq, int16_t *__restrict__ out,
    uint32_t *__restrict__ carry_all, int ref_len, int read_len, long long ld, int n_groups, int word_num,
    int n_queries, int q_tile, int stream_stride_bytes, int n_blocks, unsigned long long *task_counter,
    unsigned *__restrict__ fault_word)
{
    constexpr int semi = SEMI;
    constexpr int NC = kBitpalChains;
    constexpr int NS = kBitpalPlanes * NW;
    const int lane = threadIdx.x & (kLanes - 1);
    const int wave = threadIdx.x >> 6;
    const int n_chunks = (ref_len + 31) / 32;
    uint32_t *carry = carry_all + (static_cast<size_t>(blockIdx.x) * kWavesPerBlock + wave) * n_chunks * NC * kLanes;
    const unsigned long long carry_base = uniform_u64(reinterpret_cast<unsigned long long>(carry));
    const int q_tiles = (n_queries + q_tile - 1) / q_tile;
    const long long n_tasks = static_cast<long long>((n_groups + kWavesPerBlock - 1) / kWavesPerBlock) * q_tiles;
    const int tail_rows = ref_len & 31;
    dephase_persistent_workgroup();

    for (long long task = next_blocked_task(task_counter); task < n_tasks; task = next_blocked_task(task_counter)) {
        const int group = __builtin_amdgcn_readfirstlane(static_cast<int>(task / q_tiles) * kWavesPerBlock + wave);
        const int tile = static_cast<int>(task % q_tiles);
        if (group >= n_groups) continue;  // wave-uniform; the wave still meets the others at the next task fetch
        const uint32_t *g = peq + static_cast<size_t>(group) * kChars * word_num * kLanes + lane;
        const int q0 = tile * q_tile;
        const int q1 = (q0 + q_tile < n_queries) ? q0 + q_tile : n_queries;
        for (int q = q0; q < q1; q++) {
            for (int i = 0; i < n_chunks * NC; i++) carry[i * kLanes + lane] = 0u;  // every chain starts at carry-in 0
            const unsigned long long s =
                reinterpret_cast<unsigned long long>(streams) + static_cast<unsigned long long>(q) * stream_stride_bytes;
            int score = semi ? kBitpalGap * ref_len : kBitpalGap * (ref_len + read_len);
            int run = score;  // semi-global: S[m][j] walking right along the last row; score = its maximum
            for (int blk = 0; blk < n_blocks; blk++) {
                uint32_t P[kChars][NW];
#pragma unroll
                for (int c = 0; c < kChars; c++)
#pragma unroll
                    for (int w = 0; w < NW; w++) {
                        const int gw = blk * NW + w;
                        const int gwc = gw < word_num ? gw : word_num - 1;   // branch-free: see myers_blocked_kernel
                        P[c][w] = g[(c * word_num + gwc) * kLanes] & (gw < word_num ? ~0u : 0u);
                    }
                uint32_t st[NS + 2 * NC];
#pragma unroll
                for (int i = 0; i < NS; i++) st[i] = bitpal_init_plane(i % kBitpalPlanes, semi);
#pragma unroll
                for (int i = 0; i < NC; i++) {
                    st[NS + i] = carry[i * kLanes + lane];  // chunk 0
                    st[NS + NC + i] = 0u;
                }
                uint32_t voff = static_cast<uint32_t>(lane * 4);
                note_stream_fault(fault_word, bitpal_block_rows_asm<NW>(st, P, voff, carry_base, uniform_u64(s),
                                                                        __builtin_amdgcn_readfirstlane(stream_stride_bytes / 8 - 2)));
#pragma unroll
                for (int i = 0; i < NC; i++) {
                    const uint32_t word = tail_rows ? (st[NS + NC + i] << (32 - tail_rows)) : st[NS + NC + i];
                    carry[((n_chunks - 1) * NC + i) * kLanes + lane] = word;
                }
                if (semi)
                    bitpal_last_row_max<NW>(st, blk * NW, read_len, run, score);
                else
                    score += bitpal_column_sum<NW>(st, blk * NW, read_len);
            }
            out[static_cast<size_t>(q) * ld + static_cast<size_t>(group) * kLanes + lane] = static_cast<int16_t>(score);
        }
    }
}

// The same for score sets with so many carry chains that a register pair per chain does not fit (kBitpalPackedBlocks;
// rows_ir.py: make_blocked_packed): the carries of one row are bits of kBitpalCarryWords words per direction, and the
// row loop exchanges them with the neighbouring blocks every row — carry buffer [row][word][64 lanes] per wave, one row
// more than the query has (the loop fetches one row ahead), zeroed per query: every chain of block 0 starts at carry-in 0.
template <int NW, bool SEMI>
__global__ __launch_bounds__(256) void bitpal_packed_blocked_kernel(
    const unsigned char *__restrict__ streams, const uint32_t *__restrict__ peq, int16_t *__restrict__ out,
    uint32_t *__restrict__ carry_all, int ref_len, int read_len, long long ld, int n_groups, int word_num,
    int n_queries, int q_tile, int stream_stride_bytes, int n_blocks, unsigned long long *task_counter,
    unsigned *__restrict__ fault_word)
{
    constexpr int semi = SEMI;
    constexpr int CW = kBitpalCarryWords;
    constexpr int NS = kBitpalPlanes * NW;
    const int lane = threadIdx.x & (kLanes - 1);
    const int wave = threadIdx.x >> 6;
    const int n_rows = ref_len + 1;
    uint32_t *carry = carry_all + (static_cast<size_t>(blockIdx.x) * kWavesPerBlock + wave) * n_rows * CW * kLanes;
    const unsigned long long carry_base = uniform_u64(reinterpret_cast<unsigned long long>(carry));
    const int q_tiles = (n_queries + q_tile - 1) / q_tile;
    const long long n_tasks = static_cast<long long>((n_groups + kWavesPerBlock - 1) / kWavesPerBlock) * q_tiles;
    dephase_persistent_workgroup();

    for (long long task = next_blocked_task(task_counter); task < n_tasks; task = next_blocked_task(task_counter)) {
        const int group = __builtin_amdgcn_readfirstlane(static_cast<int>(task / q_tiles) * kWavesPerBlock + wave);
        const int tile = static_cast<int>(task % q_tiles);
        if (group >= n_groups) continue;
        const uint32_t *g = peq + static_cast<size_t>(group) * kChars * word_num * kLanes + lane;
        const int q0 = tile * q_tile;
        const int q1 = (q0 + q_tile < n_queries) ? q0 + q_tile : n_queries;
        for (int q = q0; q < q1; q++) {
            for (int i = 0; i < n_rows * CW; i++) carry[i * kLanes + lane] = 0u;
            const unsigned long long s =
                reinterpret_cast<unsigned long long>(streams) + static_cast<unsigned long long>(q) * stream_stride_bytes;
            int score = semi ? kBitpalGap * ref_len : kBitpalGap * (ref_len + read_len);
            int run = score;
            for (int blk = 0; blk < n_blocks; blk++) {
                uint32_t P[kChars][NW];
#pragma unroll
                for (int c = 0; c < kChars; c++)
#pragma unroll
                    for (int w = 0; w < NW; w++) {
                        const int gw = blk * NW + w;
                        const int gwc = gw < word_num ? gw : word_num - 1;
                        P[c][w] = g[(c * word_num + gwc) * kLanes] & (gw < word_num ? ~0u : 0u);
                    }
                uint32_t st[NS + 2 * CW], next_in[CW];
#pragma unroll
                for (int i = 0; i < NS; i++) st[i] = bitpal_init_plane(i % kBitpalPlanes, semi);
#pragma unroll
                for (int j = 0; j < CW; j++) {
                    st[NS + j] = 0u;
                    st[NS + CW + j] = 0u;
                    next_in[j] = carry[j * kLanes + lane];   // row 0
                }
                uint32_t voff = static_cast<uint32_t>(lane * 4);
                note_stream_fault(fault_word, bitpal_packed_block_rows_asm<NW>(st, P, next_in, voff, carry_base, uniform_u64(s),
                                                                               __builtin_amdgcn_readfirstlane(stream_stride_bytes / 8 - 2)));
                if (semi)
                    bitpal_last_row_max<NW>(st, blk * NW, read_len, run, score);
                else
                    score += bitpal_column_sum<NW>(st, blk * NW, read_len);
            }
            out[static_cast<size_t>(q) * ld + static_cast<size_t>(group) * kLanes + lane] = static_cast<int16_t>(score);
        }
    }
}

namespace {

// The set's kernel widths, from the generated lists (gen_rows_asm.py writes them as X-macros): what bitpal_select picks
// from and what the launchers dispatch on.
#define BGSA_WIDTH(N) .with<N>()
using PlainWidths = decltype(Widths<>{} BGSA_BITPAL_PLAIN_WIDTHS(BGSA_WIDTH));
using BlockWidths = decltype(Widths<>{} BGSA_BITPAL_BLOCK_WIDTHS(BGSA_WIDTH));
#undef BGSA_WIDTH

// Which kernel scores a subject of word_num words: set_launch dispatches on it, set_kernel_name formats it.
struct BitpalChoice {
    bool blocks;   // column blocks (in the set's carry form, kBitpalPackedBlocks) instead of the register-resident kernel
    int nw, n_blocks;
};
inline BitpalChoice bitpal_select(int word_num)
{
    BitpalChoice c = {word_num > kBitpalMaxPlain, word_num, 1};   // the plain kernels are exact widths: every word count has its own
    if (c.blocks) c.nw = BlockWidths::pick_blocks(word_num, &c.n_blocks);
    return c;
}

// Bytes of the packed-carry buffers (capi.hip sizes the workspace with the same formula: BitpalSet::carry_words).
inline size_t packed_carry_bytes(int ref_len)
{
    return static_cast<size_t>(ref_len + 1) * kBitpalCarryWords * kLanes * sizeof(uint32_t) * kWavesPerBlock * blocked_workgroups();
}

// Column blocks in the set's carry form (PACKED a template parameter so that only that form's row loops are instantiated):
// carry-token streams and a register pair per chain, or plain streams and the carries of a row packed into kBitpalCarryWords words.
template <int NW, bool PACKED>
int launch_blocked(const ScoreArgs &a, int n_blocks, int semi)
{
    const int nq = a.nq();
    const int token_stride = blocked_stream_layout(a.ref_len, nullptr, nullptr);
    const int stride = PACKED ? static_cast<int>(stream_stride(a.ref_len)) : token_stride;
    // one workspace split for both forms (capi.hip sizes the stream part for the longer CARRY-token stream)
    const size_t stream_bytes = (static_cast<size_t>(token_stride) * nq + 255) & ~static_cast<size_t>(255);
    if (int rc = PACKED ? launch_pack_queries(a.d_content, a.ref_len, a.ref_start, a.ref_end, a.d_workspace, a.stream)
                        : launch_pack_blocked(a.d_content, a.ref_len, a.ref_start, a.ref_end, a.d_workspace, a.stream))
        return rc;
    uint32_t *carry = reinterpret_cast<uint32_t *>(static_cast<unsigned char *>(a.d_workspace) + stream_bytes);
    unsigned long long *counter = reinterpret_cast<unsigned long long *>(
        reinterpret_cast<unsigned char *>(carry) + (PACKED ? packed_carry_bytes(a.ref_len) : blocked_carry_bytes(a.ref_len, kBitpalChains)));
    BGSA_HIP_TRY(hipMemsetAsync(counter, 0, sizeof(unsigned long long), a.stream));
    unsigned *fault = nullptr;
    if (int rc = stream_guard(a.d_workspace, stride, kCodeRefill, PACKED ? 7 : -1, a.stream, &fault)) return rc;
    const int q_tile = blocked_q_tile(nq, a.n_groups());
    note_query_tile(q_tile);
    auto kernel = [semi] {
        if constexpr (PACKED) return semi ? bitpal_packed_blocked_kernel<NW, true> : bitpal_packed_blocked_kernel<NW, false>;
        else return semi ? bitpal_blocked_kernel<NW, true> : bitpal_blocked_kernel<NW, false>;
    }();
    hipLaunchKernelGGL(kernel, dim3(blocked_workgroups()), dim3(256), 0, a.stream,
                       static_cast<const unsigned char *>(a.d_workspace), a.d_peq, a.results<int16_t>(), carry, a.ref_len, a.read_len,
                       static_cast<long long>(a.read_count), static_cast<int>(a.n_groups()), a.word_num, nq, q_tile, stride, n_blocks,
                       counter, fault);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

template <int NW>
int launch_nw(const ScoreArgs &a, int semi)
{
    const int nq = a.nq(), stride = static_cast<int>(stream_stride(a.ref_len));
    // a BitPAl row is 2-4x a Myers row.  Counter where the loop's registers cost no wave — asked of the runtime per score set,
    // width and mode, once (2/-3/-5: 5 words 98 -> 108 VGPRs, four waves per SIMD either way; 8 words 155 -> 169 would be
    // three -> two: 256 bp ran 10 % slower with it, profiles/r03_length_sweep.txt)
    static const bool counter_costs_no_wave[2] = {
        [] { int plain = 0, counter = 0;
             return hipOccupancyMaxActiveBlocksPerMultiprocessor(&plain, bitpal_asm_kernel<NW, false, false>, 256, 0) == hipSuccess &&
                    hipOccupancyMaxActiveBlocksPerMultiprocessor(&counter, bitpal_asm_kernel<NW, false, true>, 256, 0) == hipSuccess && counter >= plain && plain > 0; }(),
        [] { int plain = 0, counter = 0;
             return hipOccupancyMaxActiveBlocksPerMultiprocessor(&plain, bitpal_asm_kernel<NW, true, false>, 256, 0) == hipSuccess &&
                    hipOccupancyMaxActiveBlocksPerMultiprocessor(&counter, bitpal_asm_kernel<NW, true, true>, 256, 0) == hipSuccess && counter >= plain && plain > 0; }()};
    // A mixed-length bucket (global mode; capi.hip refused the rest) runs the LENS instantiation, of which a width has ONE: on the
    // counter up to 8 words — whatever the occupancy answer above and BGSA_DYNAMIC_TASKS say —, on the static grid beyond.
    const bool lens = a.d_read_lens != nullptr;
    if (lens && semi) {
        set_error_text("bitpal: per-subject lengths are scored in global mode only");
        return BGSA_HIP_EUNSUPPORTED;
    }
    const TaskPlan plan = plan_tasks(nq, a.n_groups(), static_cast<long long>(a.ref_len) * NW * 2, 16,
                                     NW <= 8 && (lens || counter_costs_no_wave[semi ? 1 : 0]), query_tile_max(), lens);
    if (lens && NW <= 8 && !plan.dynamic) {
        set_error_text("bitpal: too many tasks for one length-aware launch (split the query window)");
        return BGSA_HIP_EUNSUPPORTED;
    }
    note_query_tile(plan.q_tile);
    const auto on_counter = lens ? bitpal_asm_kernel<NW, false, NW <= 8, true> : semi ? bitpal_asm_kernel<NW, true, true> : bitpal_asm_kernel<NW, false, true>;
    LaunchGrid lg;   // the counter is zeroed by the packer
    if (int rc = plan_grid(plan, a.n_groups(), nq, task_counter_in(a.d_workspace, static_cast<size_t>(stride) * nq),
                           [&] { return persistent_blocks_for(on_counter); }, "bitpal", &lg))
        return rc;
    if (int rc = launch_pack_queries(a.d_content, a.ref_len, a.ref_start, a.ref_end, a.d_workspace, a.stream, lg.counter)) return rc;
    unsigned *fault = nullptr;
    if (int rc = stream_guard(a.d_workspace, stride, kCodeRefill, 7, a.stream, &fault)) return rc;
    const auto kernel = (lg.counter || lens) ? on_counter : (semi ? bitpal_asm_kernel<NW, true, false> : bitpal_asm_kernel<NW, false, false>);
    hipLaunchKernelGGL(kernel, lg.grid, dim3(256), 0, a.stream,
                       static_cast<const unsigned char *>(a.d_workspace), a.d_peq, a.results<int16_t>(), a.ref_len,
                       a.read_len, static_cast<long long>(a.read_count), static_cast<int>(a.n_groups()), a.word_num,
                       nq, plan.q_tile, stride, fault, lg.counter, a.d_read_lens);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

}  // namespace

const char *set_kernel_name(int word_num)
{
    static thread_local char name[64];
    const BitpalChoice c = bitpal_select(word_num);
    snprintf(name, sizeof name, !c.blocks ? "bitpal_asm_kernel<%d>" : kBitpalPackedBlocks ? "bitpal_packed_blocked_kernel<%d>" : "bitpal_blocked_kernel<%d>",
             c.nw);
    return name;
}

int set_launch(const ScoreArgs &a, int semi)
{
    const BitpalChoice c = bitpal_select(a.word_num);
    if (a.d_read_lens && c.blocks) {
        set_error_text("bitpal: per-subject lengths are scored by the register-resident kernel only; this score set's reaches fewer words");
        return BGSA_HIP_EUNSUPPORTED;
    }
    if (c.blocks)
        return BlockWidths::dispatch(c.nw, "bitpal column blocks",
                                     [&](auto nw) { return launch_blocked<decltype(nw)::value, kBitpalPackedBlocks>(a, c.n_blocks, semi); });
    return PlainWidths::dispatch(c.nw, "bitpal_asm_kernel", [&](auto nw) { return launch_nw<decltype(nw)::value>(a, semi); });
}
