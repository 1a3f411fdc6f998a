// sam_records.hip — the last stage of read mapping: a mapping quality per hit list, and the SAM text of every record written
// by the device into one byte buffer (include/bgsa_hip.h "SAM records").  Three kernels:
//   sam_mapq_kernel     one wave per read, one lane per slot of its hit list: the primary slot (the first kept one), the kept
//                       slots at its distance (a ballot), the smallest kept distance above it (a butterfly minimum), the MAPQ.
//   sam_measure_kernel  pass 1: one wave per record, the byte length of its line; a malformed record gets 0 and is counted.
//   sam_emit_kernel     pass 2: the same walk once more to check the record against the length the caller's scan was made
//                       from, then the text.  QNAME, RNAME, SEQ and QUAL are written by all lanes in contiguous pieces; the
//                       CIGAR one lane per run, a wave prefix sum of the runs' text widths giving the offsets, 64 runs at a time;
//                       MD by the same scheme — the '=' bases in front of a run are a segmented sum: a prefix sum of the '='
//                       lengths minus its value at the last X or D run (a prefix maximum) —, the letters of a run of more than
//                       kSerialBases bases written by the whole wave.
// The checked record and the walk over its runs are sam_record.h's, shared with bam_records.hip.
// Ids, coordinates, lengths and runs are values until checked (check_record): none forms an address before it has been compared
// with the extent the caller states, and pass 2 writes a record only if its recomputed length is the one its offsets leave
// room for and that room lies inside the text buffer.  No LDS, no scratch, vector stores only.
#include "sam_record.h"

namespace bgsa {

namespace {

// The line of a checked record: EMIT false returns its length, EMIT true writes it at out as well.
template <bool EMIT>
__device__ __forceinline__ long long record_line(const Batch &b, const Record &r, uint8_t *out, int lane)
{
    long long at = 0;
    auto bytes = [&](const uint8_t *src, long long n) {      // n bytes of src, then a tab
        if (EMIT) {
            for (long long j = lane; j < n; j += kLanes) out[at + j] = src[j];
            if (lane == 0) out[at + n] = '\t';
        }
        at += n + 1;
    };
    auto one = [&](char c, char close = '\t') {
        if (EMIT && lane == 0) {
            out[at] = static_cast<uint8_t>(c);
            out[at + 1] = static_cast<uint8_t>(close);
        }
        at += 2;
    };
    auto number = [&](unsigned long long v, bool negative = false) {
        if (negative) {
            if (EMIT && lane == 0) out[at] = '-';
            at += 1;
        }
        const int w = EMIT ? put_dec(out + at, v, lane) : dec_width(v);
        if (EMIT && lane == 0) out[at + w] = '\t';
        at += w + 1;
    };
    const bool named = r.mapped || r.mate_named;
    bytes(r.name, r.name_len);
    number(r.flag);
    if (named) bytes(r.rname, r.rname_len); else one('*');
    number(r.pos);
    number(r.mapq);
    const long long cigar_at = at;
    if (r.mapped) {
        if (EMIT && lane == 0) out[at + r.cigar_bytes] = '\t';
        at += r.cigar_bytes + 1;
    } else {
        one('*');
    }
    if (r.rnext) bytes(r.rnext, r.rnext_len); else one(r.mate_named ? '=' : '*');
    number(r.pnext);
    number(r.tlen_abs, r.tlen_negative && r.tlen_abs != 0);
    if (EMIT) {
        for (int j = lane; j < r.read_len; j += kLanes) {
            uint8_t c = r.seq[r.reverse ? r.read_len - 1 - j : j];
            if (r.reverse) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
            out[at + j] = c;
        }
        if (lane == 0) out[at + r.read_len] = '\t';
    }
    at += r.read_len + 1;
    if (r.qual) {
        if (EMIT)
            for (int j = lane; j < r.read_len; j += kLanes) out[at + j] = r.qual[r.reverse ? r.read_len - 1 - j : j];
        at += r.read_len;
    } else {
        if (EMIT && lane == 0) out[at] = '*';
        at += 1;
    }
    if (r.mapped) {
        if (EMIT && lane < 6) out[at + lane] = static_cast<uint8_t>("\tNM:i:"[lane]);
        at += 6;
        at += EMIT ? put_dec(out + at, r.distance, lane) : dec_width32(r.distance);
        if (EMIT && lane < 6) out[at + lane] = static_cast<uint8_t>("\tMD:Z:"[lane]);
        at += 6;
        if (EMIT) walk_runs<kWalkSamText>(r.runs, r.n_ops, r.ref, out + cigar_at, out + at, lane);
        at += r.md_bytes;
    }
    if (EMIT && lane == 0) out[at] = '\n';
    return at + 1;
}

template <bool CONTIGS>
__global__ __launch_bounds__(256) void sam_measure_kernel(Batch b, Contigs ct, int64_t n, int64_t *__restrict__ lengths, int32_t *__restrict__ malformed)
{
    const int lane = threadIdx.x & (kLanes - 1);
    const int64_t i = static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= n) return;              // wave-uniform
    const Record r = check_record<CONTIGS>(b, ct, i);
    long long bytes = 0;
    if (r.ok) bytes = record_line<false>(b, r, nullptr, lane);
    else count_malformed(malformed, lane);
    if (lane == 0) lengths[i] = bytes;
}

template <bool CONTIGS>
__global__ __launch_bounds__(256) void sam_emit_kernel(Batch b, Contigs ct, int64_t n, const int64_t *__restrict__ offsets,
                                                       uint8_t *__restrict__ text, int64_t text_bytes, int32_t *__restrict__ malformed)
{
    const int lane = threadIdx.x & (kLanes - 1);
    const int64_t i = static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= n) return;              // wave-uniform
    const Record r = check_record<CONTIGS>(b, ct, i);
    const long long lo = uniform_i64(offsets[i]), hi = uniform_i64(offsets[i + 1]);
    // written only where the line is exactly what its offsets leave room for, inside the buffer
    if (!r.ok || lo < 0 || hi < lo || hi > text_bytes || record_line<false>(b, r, nullptr, lane) != hi - lo) {
        count_malformed(malformed, lane);
        return;
    }
    record_line<true>(b, r, text + lo, lane);
}

// ---- MAPQ of a hit list ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int mapq_of(long long d1, int n1, long long d2, bool has_d2, long long bound)
{
    if (n1 >= 2) return n1 == 2 ? 3 : n1 == 3 ? 2 : n1 <= 9 ? 1 : 0;
    const long long gap = has_d2 ? d2 - d1 : bound >= 0 ? bound + 1 - d1 : 6;
    return gap <= 0 ? 0 : gap >= 6 ? 60 : static_cast<int>(10 * gap);
}

__global__ __launch_bounds__(256) void sam_mapq_kernel(const int32_t *__restrict__ scores, const int32_t *__restrict__ keep, int64_t ns, int k,
                                                       int bound, int32_t *__restrict__ primary_out, int32_t *__restrict__ mapq_out,
                                                       int32_t *__restrict__ n1_out, int32_t *__restrict__ d2_out)
{
    const int lane = threadIdx.x & (kLanes - 1);
    const int64_t read = static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (read >= ns) return;          // wave-uniform
    const int64_t p = read * k + lane;
    const bool kept = lane < k && keep[p] != 0;
    const long long d = kept ? -static_cast<long long>(scores[p]) : 0;
    const unsigned long long kept_mask = __ballot(kept);
    int primary = -1, mapq = 0, n1 = 0;
    long long d2 = -1;
    if (kept_mask) {                 // wave-uniform
        primary = __ffsll(kept_mask) - 1;
        const long long d1 = __shfl(d, primary);
        n1 = __popcll(__ballot(kept && d == d1));
        long long above = kept && d > d1 ? d : LLONG_MAX;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const long long other = __shfl_xor(above, off);
            above = other < above ? other : above;
        }
        const bool has_d2 = above != LLONG_MAX;
        if (has_d2) d2 = above;
        mapq = mapq_of(d1, n1, above, has_d2, bound);
    }
    if (lane == 0) {
        primary_out[read] = primary;
        mapq_out[read] = mapq;
        n1_out[read] = n1;
        d2_out[read] = static_cast<int32_t>(d2);
    }
}

// The two launches, shared by the one-sequence calls (CONTIGS false, an empty table) and the contig ones.
template <bool CONTIGS>
int launch_measure(const Batch *batch, const Contigs &ct, int64_t n, int64_t *d_lengths, int32_t *d_malformed, void *stream)
{
    hipLaunchKernelGGL(sam_measure_kernel<CONTIGS>, dim3(static_cast<unsigned>((n + kWavesPerBlock - 1) / kWavesPerBlock)),
                       dim3(kWavesPerBlock * kLanes), 0, static_cast<hipStream_t>(stream), *batch, ct, n, d_lengths, d_malformed);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

template <bool CONTIGS>
int launch_emit(const Batch *batch, const Contigs &ct, int64_t n, const int64_t *d_offsets, uint8_t *d_text, int64_t text_bytes,
                int32_t *d_malformed, void *stream)
{
    hipLaunchKernelGGL(sam_emit_kernel<CONTIGS>, dim3(static_cast<unsigned>((n + kWavesPerBlock - 1) / kWavesPerBlock)),
                       dim3(kWavesPerBlock * kLanes), 0, static_cast<hipStream_t>(stream), *batch, ct, n, d_offsets, d_text, text_bytes,
                       d_malformed);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

}  // namespace

}  // namespace bgsa

using namespace bgsa;

extern "C" {

int bgsa_hip_sam_mapq_dev(const int32_t *d_scores, const int32_t *d_keep, int64_t ns, int k, int bound, int32_t *d_primary, int32_t *d_mapq,
                          int32_t *d_n1, int32_t *d_d2, void *stream)
{
    const char *who = "sam_mapq_dev";
    if (!d_scores || !d_keep || !d_primary || !d_mapq || !d_n1 || !d_d2) return refuse(who, BGSA_HIP_EINVAL, "a NULL pointer (only the stream may be NULL)");
    if (k < 1 || k > HIP_V_NUM) return refuse(who, BGSA_HIP_EINVAL, "k must lie in 1..64 (one wavefront holds a read's list, one slot per lane)");
    if (bound < -1) return refuse(who, BGSA_HIP_EINVAL, "bound is below -1 (-1: the list is complete within no bound)");
    if (ns < 0 || ns > static_cast<int64_t>(INT32_MAX) * kWavesPerBlock) return refuse(who, BGSA_HIP_EINVAL, "ns is negative or beyond one launch");
    if (ns == 0) return BGSA_HIP_OK;
    hipLaunchKernelGGL(sam_mapq_kernel, dim3(static_cast<unsigned>((ns + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(kWavesPerBlock * kLanes), 0,
                       static_cast<hipStream_t>(stream), d_scores, d_keep, ns, k, bound, d_primary, d_mapq, d_n1, d_d2);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

int bgsa_hip_sam_measure_dev(const bgsa_hip_sam_batch_t *batch, int64_t n, int64_t *d_lengths, int32_t *d_malformed, void *stream)
{
    const char *who = "sam_measure_dev";
    if (int rc = check_batch(who, batch, n)) return rc;
    if (!d_lengths || !d_malformed) return refuse(who, BGSA_HIP_EINVAL, "d_lengths or d_malformed is NULL");
    if (n == 0) return BGSA_HIP_OK;
    return launch_measure<false>(batch, Contigs{}, n, d_lengths, d_malformed, stream);
}

int bgsa_hip_sam_emit_dev(const bgsa_hip_sam_batch_t *batch, int64_t n, const int64_t *d_offsets, uint8_t *d_text, int64_t text_bytes,
                          int32_t *d_malformed, void *stream)
{
    const char *who = "sam_emit_dev";
    if (int rc = check_batch(who, batch, n)) return rc;
    if (!d_offsets || !d_text || !d_malformed) return refuse(who, BGSA_HIP_EINVAL, "d_offsets, d_text or d_malformed is NULL");
    if (text_bytes < 0) return refuse(who, BGSA_HIP_EINVAL, "text_bytes is negative");
    if (n == 0) return BGSA_HIP_OK;
    return launch_emit<false>(batch, Contigs{}, n, d_offsets, d_text, text_bytes, d_malformed, stream);
}

int bgsa_hip_sam_measure_contigs_dev(const bgsa_hip_sam_batch_t *batch, const bgsa_hip_sam_contigs_t *contigs, int64_t n, int64_t *d_lengths,
                                     int32_t *d_malformed, void *stream)
{
    const char *who = "sam_measure_contigs_dev";
    if (int rc = check_contig_batch(who, batch, contigs, n)) return rc;
    if (!d_lengths || !d_malformed) return refuse(who, BGSA_HIP_EINVAL, "d_lengths or d_malformed is NULL");
    if (n == 0) return BGSA_HIP_OK;
    return launch_measure<true>(batch, *contigs, n, d_lengths, d_malformed, stream);
}

int bgsa_hip_sam_emit_contigs_dev(const bgsa_hip_sam_batch_t *batch, const bgsa_hip_sam_contigs_t *contigs, int64_t n, const int64_t *d_offsets,
                                  uint8_t *d_text, int64_t text_bytes, int32_t *d_malformed, void *stream)
{
    const char *who = "sam_emit_contigs_dev";
    if (int rc = check_contig_batch(who, batch, contigs, n)) return rc;
    if (!d_offsets || !d_text || !d_malformed) return refuse(who, BGSA_HIP_EINVAL, "d_offsets, d_text or d_malformed is NULL");
    if (text_bytes < 0) return refuse(who, BGSA_HIP_EINVAL, "text_bytes is negative");
    if (n == 0) return BGSA_HIP_OK;
    return launch_emit<true>(batch, *contigs, n, d_offsets, d_text, text_bytes, d_malformed, stream);
}

}  // extern "C"
