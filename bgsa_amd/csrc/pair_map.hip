// pair_map.hip — paired reads: the windows in which a mate can lie, given the other end's placement, and the choice of the best
// proper pair (include/bgsa_hip.h "paired reads").  Two small kernels; verification, selection and placement
// of the windows named here are the calls of seed_map.hip and reference_windows.hip, unchanged.
//
// Geometry (the header states it; bgsa_amd/reference.py: rescue_slots, rescue_region and tests/pair_reference.py restate it).  The
// windows are those of reference_windows.hip: L mapped bytes, 1 <= S <= W <= L, n_windows = 1 + ceil((L - W) / S), start(w) =
// min(w * S, L - W).  Library type FR only: the mates lie on opposite strands, the forward-strand mate upstream.
//   region   an anchor on strand s with interval [b, e) puts its mate on strand 1 - s, inside [b, min(L, b + insert_max)) for
//            s = 0 and inside [max(0, e - insert_max), e) for s = 1.
//   rescue   the forward windows w with start(w) < region_hi and start(w) + W > region_lo, as ids on the mate's strand: one
//            contiguous id range of at most R = min(n_windows, ceil((insert_max + W - 1) / S) + 1) ids.
//   proper   slots r1, r2 of the two ends on different strands, F the forward one and R the reverse one, with F.begin <= R.begin,
//            F.end <= R.end and insert_min <= R.end - F.begin <= insert_max; cost = d1 + d2, the choice the minimum by (cost, r1, r2).
//
// rescue windows  one wave per pair: lane r reads slot r of the anchor list, a ballot of the kept slots ranks them, and anchor a's
//                 range (first id, count) is read from its lane and written by all 64 lanes, R entries per anchor, -1 behind
//                 the range.  The ids are values: nothing here or later forms an address from one without a range check.
// select          one wave per pair: lane r1 holds slot r1 of end 1, end 2's slots are read from their lanes one at a time
//                 (a wave-uniform index: v_readlane), every lane keeps the smallest key cost << 12 | r1 << 6 | r2 of its proper
//                 combinations, and a butterfly of __shfl_xor reduces it.  A second pass over the same combinations counts those
//                 at the chosen cost and finds the smallest cost above it.  No LDS, no scratch.
#include "reference_geometry.h"   // Geometry, make_geometry

namespace bgsa {

namespace {

constexpr int64_t kScoreFloor = -((1ll << 30) - 1);      // a live slot's score lies in [kScoreFloor, 0]: a cost fits an int32

// ---- rescue windows --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pair_rescue_windows_kernel(Geometry g, const int32_t *__restrict__ strand,
                                                                  const int64_t *__restrict__ ref_begin, const int64_t *__restrict__ ref_end,
                                                                  const int32_t *__restrict__ keep, int64_t n_pairs, int k, int k_anchor,
                                                                  int64_t insert_max, int64_t slots, int32_t *__restrict__ rescue)
{
    const int lane = threadIdx.x & (kLanes - 1);
    const int64_t pair = static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (pair >= n_pairs) return;     // wave-uniform
    const int64_t p = pair * k + lane;
    const bool kept = lane < k && keep[p] != 0;
    long long first = 0, count = 0;  // this lane's range, should it be an anchor
    if (kept) {
        const int s = strand[p];
        long long b = ref_begin[p], e = ref_end[p];
        if ((s == 0 || s == 1) && b >= 0 && e >= b && e <= g.ref_len) {      // anything else: an anchor without a region
            const long long region_lo = s ? (e - insert_max > 0 ? e - insert_max : 0) : b;
            const long long region_hi = s ? e : (b + insert_max < g.ref_len ? b + insert_max : g.ref_len);
            // start(w) in [lo, hi]: start(w) + W > region_lo and start(w) < region_hi
            long long lo = region_lo - g.window_len + 1;
            const long long hi = region_hi - 1;
            if (lo < 0) lo = 0;
            if (hi >= lo) {
                const bool last = lo <= g.last_start && g.last_start <= hi;       // the anchored last window
                long long w_lo = (lo + g.stride - 1) / g.stride, w_hi = hi / g.stride;   // the regular ones: start w * S, w <= n_windows - 2
                if (w_hi > g.n_windows - 2) w_hi = g.n_windows - 2;
                if (w_lo > g.n_windows - 1) w_lo = g.n_windows - 1;
                const long long w_end = last ? g.n_windows - 1 : w_hi;
                count = w_end >= w_lo ? w_end - w_lo + 1 : 0;
                if (count > slots) count = slots;                                 // cannot happen (the bound R); no write leaves the group
                first = (1 - s) * g.n_windows + w_lo;
            }
        }
    }
    const unsigned long long kept_mask = __ballot(kept);
    int32_t *out = rescue + pair * (static_cast<int64_t>(k_anchor) * slots);
    for (int a = 0; a < k_anchor; a++) {         // wave-uniform
        unsigned long long rest = kept_mask;
        for (int i = 0; i < a && rest; i++) rest &= rest - 1;     // drop the a lowest kept slots
        long long a_first = 0, a_count = 0;
        if (rest) {
            const int owner = __ffsll(rest) - 1;
            a_first = __shfl(first, owner);
            a_count = __shfl(count, owner);
        }
        for (int64_t j = lane; j < slots; j += kLanes)
            out[a * slots + j] = j < a_count ? static_cast<int32_t>(a_first + j) : -1;
    }
}

// ---- the pair ----------------------------------------------------------------------------------------------------------------
struct EndList {
    const int32_t *scores, *strand;
    const int64_t *ref_begin, *ref_end;
    const int32_t *keep;
    int k;
};

struct Slot {
    bool live;
    int strand;
    long long begin, end, distance;
};

__device__ __forceinline__ Slot load_slot(const EndList &list, int64_t pair, int lane)
{
    Slot s{false, -1, -1, -1, 0};
    if (lane < list.k) {
        const int64_t p = pair * list.k + lane;
        const long long score = list.scores[p];
        s.strand = list.strand[p];
        s.begin = list.ref_begin[p];
        s.end = list.ref_end[p];
        s.distance = -score;
        s.live = list.keep[p] != 0 && (s.strand == 0 || s.strand == 1) && s.begin >= 0 && score <= 0 && score >= kScoreFloor;
    }
    return s;
}

// Whether the combination (mine, other) is proper, and its insert.
__device__ __forceinline__ bool proper_pair(const Slot &mine, bool o_live, int o_strand, long long o_begin, long long o_end,
                                            long long insert_min, long long insert_max, long long *insert)
{
    const bool forward = mine.strand == 0;
    const long long f_begin = forward ? mine.begin : o_begin, f_end = forward ? mine.end : o_end;
    const long long r_begin = forward ? o_begin : mine.begin, r_end = forward ? o_end : mine.end;
    *insert = r_end - f_begin;
    return mine.live && o_live && mine.strand != o_strand && f_begin <= r_begin && f_end <= r_end && *insert >= insert_min &&
           *insert <= insert_max;
}

__global__ __launch_bounds__(256) void pair_select_kernel(EndList one, EndList two, int64_t n_pairs, long long insert_min, long long insert_max,
                                                          int32_t *__restrict__ proper_out, int32_t *__restrict__ slot1_out,
                                                          int32_t *__restrict__ slot2_out, int64_t *__restrict__ insert_out,
                                                          int32_t *__restrict__ cost_out, int32_t *__restrict__ n_best_out,
                                                          int32_t *__restrict__ next_cost_out)
{
    const int lane = threadIdx.x & (kLanes - 1);
    const int64_t pair = static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (pair >= n_pairs) return;     // wave-uniform
    const Slot mine = load_slot(one, pair, lane), theirs = load_slot(two, pair, lane);
    const unsigned long long none = ~0ull;
    unsigned long long best = none;
    for (int r2 = 0; r2 < two.k; r2++) {         // wave-uniform: every lane takes part in the shuffles
        const bool o_live = __shfl(static_cast<int>(theirs.live), r2) != 0;
        const int o_strand = __shfl(theirs.strand, r2);
        const long long o_begin = __shfl(theirs.begin, r2), o_end = __shfl(theirs.end, r2), o_distance = __shfl(theirs.distance, r2);
        long long insert;
        if (proper_pair(mine, o_live, o_strand, o_begin, o_end, insert_min, insert_max, &insert)) {
            const unsigned long long key = (static_cast<unsigned long long>(mine.distance + o_distance) << 12) |
                                           (static_cast<unsigned long long>(lane) << 6) | static_cast<unsigned long long>(r2);
            best = key < best ? key : best;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long other = __shfl_xor(best, off);
        best = other < best ? other : best;
    }
    if (best == none) {              // wave-uniform: no proper combination
        const unsigned long long live1 = __ballot(mine.live), live2 = __ballot(theirs.live);
        const int s1 = live1 ? __ffsll(live1) - 1 : -1, s2 = live2 ? __ffsll(live2) - 1 : -1;
        const long long d1 = __shfl(mine.distance, s1 < 0 ? 0 : s1), d2 = __shfl(theirs.distance, s2 < 0 ? 0 : s2);
        if (lane == 0) {
            proper_out[pair] = 0;
            slot1_out[pair] = s1;
            slot2_out[pair] = s2;
            insert_out[pair] = 0;
            cost_out[pair] = static_cast<int32_t>((s1 < 0 ? 0 : d1) + (s2 < 0 ? 0 : d2));
            n_best_out[pair] = 0;
            next_cost_out[pair] = -1;
        }
        return;
    }
    const long long cost = static_cast<long long>(best >> 12);
    const int r1 = static_cast<int>((best >> 6) & 63u), r2_best = static_cast<int>(best & 63u);
    int at_cost = 0;
    long long above = -1;            // this lane's smallest proper cost above the chosen one
    long long chosen_insert = 0;
    for (int r2 = 0; r2 < two.k; r2++) {
        const bool o_live = __shfl(static_cast<int>(theirs.live), r2) != 0;
        const int o_strand = __shfl(theirs.strand, r2);
        const long long o_begin = __shfl(theirs.begin, r2), o_end = __shfl(theirs.end, r2), o_distance = __shfl(theirs.distance, r2);
        long long insert;
        if (proper_pair(mine, o_live, o_strand, o_begin, o_end, insert_min, insert_max, &insert)) {
            const long long c = mine.distance + o_distance;
            at_cost += c == cost;
            if (c > cost && (above < 0 || c < above)) above = c;
            if (lane == r1 && r2 == r2_best) chosen_insert = insert;
        }
    }
    unsigned long long next = above < 0 ? none : static_cast<unsigned long long>(above);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        at_cost += __shfl_xor(at_cost, off);
        const unsigned long long other = __shfl_xor(next, off);
        next = other < next ? other : next;
    }
    chosen_insert = __shfl(chosen_insert, r1);
    if (lane == 0) {
        proper_out[pair] = 1;
        slot1_out[pair] = r1;
        slot2_out[pair] = r2_best;
        insert_out[pair] = chosen_insert;
        cost_out[pair] = static_cast<int32_t>(cost);
        n_best_out[pair] = at_cost;
        next_cost_out[pair] = next == none ? -1 : static_cast<int32_t>(next);
    }
}

// ---- checks ------------------------------------------------------------------------------------------------------------------
// The shape of reference_windows.hip's calls, then insert_max and R.  0, or BGSA_HIP_EINVAL with its text set.
int rescue_geometry(const char *who, int64_t ref_len, int window_len, int stride, int64_t insert_max, Geometry *out, int64_t *slots)
{
    if (int rc = make_geometry(who, ref_len, window_len, stride, out)) return rc;
    if (insert_max < 1 || insert_max > static_cast<int64_t>(INT32_MAX)) return refuse(who, BGSA_HIP_EINVAL, "insert_max must lie in [1, 2^31 - 1]");
    const int64_t span = (insert_max + window_len - 1 + stride - 1) / stride + 1;
    *slots = span < out->n_windows ? span : out->n_windows;
    return BGSA_HIP_OK;
}

bool end_list_ok(const int32_t *scores, const int32_t *strand, const int64_t *ref_begin, const int64_t *ref_end, const int32_t *keep)
{
    return scores && strand && ref_begin && ref_end && keep;
}

}  // namespace

}  // namespace bgsa

using namespace bgsa;

extern "C" {

int64_t bgsa_hip_pair_rescue_slots(int64_t ref_len, int window_len, int stride, int64_t insert_max)
{
    Geometry g;
    int64_t slots = 0;
    return rescue_geometry("pair_rescue_slots", ref_len, window_len, stride, insert_max, &g, &slots) ? -1 : slots;
}

int bgsa_hip_pair_rescue_windows_dev(int64_t ref_len, int window_len, int stride, const int32_t *d_strand, const int64_t *d_ref_begin,
                                     const int64_t *d_ref_end, const int32_t *d_keep, int64_t n_pairs, int k, int k_anchor,
                                     int64_t insert_max, int32_t *d_rescue, void *stream)
{
    const char *who = "pair_rescue_windows_dev";
    if (!d_strand || !d_ref_begin || !d_ref_end || !d_keep || !d_rescue) return refuse(who, BGSA_HIP_EINVAL, "a NULL pointer (only the stream may be NULL)");
    Geometry g;
    int64_t slots = 0;
    if (int rc = rescue_geometry(who, ref_len, window_len, stride, insert_max, &g, &slots)) return rc;
    if (2 * g.n_windows > static_cast<int64_t>(INT32_MAX)) return refuse(who, BGSA_HIP_EINVAL, "the windows on two strands do not fit int32 window ids");
    if (k < 1 || k > HIP_V_NUM) return refuse(who, BGSA_HIP_EINVAL, "k must lie in 1..64 (one wavefront holds a list, one slot per lane)");
    if (k_anchor < 1 || k_anchor > HIP_V_NUM) return refuse(who, BGSA_HIP_EINVAL, "k_anchor must lie in 1..64");
    if (n_pairs < 0 || n_pairs > static_cast<int64_t>(INT32_MAX) * kWavesPerBlock) return refuse(who, BGSA_HIP_EINVAL, "n_pairs is negative or beyond one launch");
    if (n_pairs == 0) return BGSA_HIP_OK;
    hipLaunchKernelGGL(pair_rescue_windows_kernel, dim3(static_cast<unsigned>((n_pairs + kWavesPerBlock - 1) / kWavesPerBlock)),
                       dim3(kWavesPerBlock * kLanes), 0, static_cast<hipStream_t>(stream), g, d_strand, d_ref_begin, d_ref_end, d_keep, n_pairs,
                       k, k_anchor, insert_max, slots, d_rescue);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

int bgsa_hip_pair_select_dev(const int32_t *d_scores1, const int32_t *d_strand1, const int64_t *d_ref_begin1, const int64_t *d_ref_end1,
                             const int32_t *d_keep1, int k1, const int32_t *d_scores2, const int32_t *d_strand2,
                             const int64_t *d_ref_begin2, const int64_t *d_ref_end2, const int32_t *d_keep2, int k2, int64_t n_pairs,
                             int64_t insert_min, int64_t insert_max, int32_t *d_proper, int32_t *d_slot1, int32_t *d_slot2,
                             int64_t *d_insert, int32_t *d_cost, int32_t *d_n_best, int32_t *d_next_cost, void *stream)
{
    const char *who = "pair_select_dev";
    if (!end_list_ok(d_scores1, d_strand1, d_ref_begin1, d_ref_end1, d_keep1) || !end_list_ok(d_scores2, d_strand2, d_ref_begin2, d_ref_end2, d_keep2) ||
        !d_proper || !d_slot1 || !d_slot2 || !d_insert || !d_cost || !d_n_best || !d_next_cost)
        return refuse(who, BGSA_HIP_EINVAL, "a NULL pointer (only the stream may be NULL)");
    if (k1 < 1 || k1 > HIP_V_NUM || k2 < 1 || k2 > HIP_V_NUM) return refuse(who, BGSA_HIP_EINVAL, "k1 and k2 must lie in 1..64 (one wavefront holds a list)");
    if (insert_min < 1 || insert_max < insert_min || insert_max > static_cast<int64_t>(INT32_MAX))
        return refuse(who, BGSA_HIP_EINVAL, "needs 1 <= insert_min <= insert_max <= 2^31 - 1");
    if (n_pairs < 0 || n_pairs > static_cast<int64_t>(INT32_MAX) * kWavesPerBlock) return refuse(who, BGSA_HIP_EINVAL, "n_pairs is negative or beyond one launch");
    if (n_pairs == 0) return BGSA_HIP_OK;
    const EndList one{d_scores1, d_strand1, d_ref_begin1, d_ref_end1, d_keep1, k1}, two{d_scores2, d_strand2, d_ref_begin2, d_ref_end2, d_keep2, k2};
    hipLaunchKernelGGL(pair_select_kernel, dim3(static_cast<unsigned>((n_pairs + kWavesPerBlock - 1) / kWavesPerBlock)),
                       dim3(kWavesPerBlock * kLanes), 0, static_cast<hipStream_t>(stream), one, two, n_pairs,
                       static_cast<long long>(insert_min), static_cast<long long>(insert_max), d_proper, d_slot1, d_slot2, d_insert, d_cost,
                       d_n_best, d_next_cost);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

}  // extern "C"
