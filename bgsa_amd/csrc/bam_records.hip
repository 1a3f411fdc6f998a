// bam_records.hip — the records of sam_records.hip in BAM's binary layout (include/bgsa_hip.h "BAM records"; INTEGRATION.md §3q;
// SAMv1 §4.2), written by the device into one payload buffer that bgzf.hip then frames.  Two kernels, the two-pass contract of
// the SAM stage:
//   bam_measure_kernel  pass 1: one wave per record, its byte length including the 4-byte block_size; a malformed record gets 0
//                       and is counted.
//   bam_emit_kernel     pass 2: the record checked once more against the length the caller's scan was made from, then its bytes.
//                       The nine fixed words by lanes 0..35, a byte each; the name, SEQ (two bases a byte) and QUAL by all lanes
//                       in contiguous pieces; the CIGAR words one lane per run and the MD text by the SAM stage's own walk
//                       (sam_record.h: walk_runs<kWalkBamWords>).
// The record check is the SAM stage's (sam_record.h: check_record), then what BAM's narrower fields add (bam_fits).  A record
// starts at any byte address, so every store is a byte store.  No LDS, no scratch, vector stores only.
#include "sam_record.h"

namespace bgsa {

namespace {

// The 4-bit codes of 'A' + first .. 'A' + first + 15, a nibble each: the letter's index in "=ACMGRSVTWYHKDBN", 15 for any other.
constexpr unsigned long long seq_codes(int first)
{
    const char codes[] = "=ACMGRSVTWYHKDBN";
    unsigned long long table = 0;
    for (int i = 0; i < 16; i++) {
        unsigned long long code = 15;
        for (int k = 1; k < 16; k++)
            if (codes[k] == 'A' + first + i) code = static_cast<unsigned long long>(k);
        table |= code << (4 * i);
    }
    return table;
}
constexpr unsigned long long kSeqCodesAtoP = seq_codes(0), kSeqCodesQtoZ = seq_codes(16);

__device__ __forceinline__ unsigned seq_code(uint8_t c)      // case-insensitive
{
    if (c == '=') return 0u;
    const unsigned letter = (c & 0xdfu) - 'A';
    if (letter >= 26u) return 15u;
    return static_cast<unsigned>((letter < 16u ? kSeqCodesAtoP >> (4 * letter) : kSeqCodesQtoZ >> (4 * (letter - 16u))) & 15ull);
}

// reg2bin of the specification (SAMv1 §5.3) for the half-open interval [beg, end), beg >= 0, kept to 16 bits as the field is.
__device__ __forceinline__ unsigned reg2bin(long long beg, long long end)
{
    --end;
    long long bin = 0;
    if (beg >> 14 == end >> 14) bin = ((1 << 15) - 1) / 7 + (beg >> 14);
    else if (beg >> 17 == end >> 17) bin = ((1 << 12) - 1) / 7 + (beg >> 17);
    else if (beg >> 20 == end >> 20) bin = ((1 << 9) - 1) / 7 + (beg >> 20);
    else if (beg >> 23 == end >> 23) bin = ((1 << 6) - 1) / 7 + (beg >> 23);
    else if (beg >> 26 == end >> 26) bin = ((1 << 3) - 1) / 7 + (beg >> 26);
    return static_cast<unsigned>(bin) & 0xffffu;
}

// What BAM's fields add to the SAM stage's rules: l_read_name is a byte, n_cigar_op 16 bits, pos, next_pos and tlen int32.
__device__ __forceinline__ bool bam_fits(const Record &r)
{
    return r.name_len <= 254 && r.n_ops <= 65535 && r.pos <= 0x80000000ull && r.pnext <= 0x80000000ull &&
           r.tlen_abs <= (r.tlen_negative ? 0x80000000ull : 0x7fffffffull);
}

// The bytes of a checked record that fits: EMIT false returns their number, EMIT true writes them at out as well.
template <bool EMIT>
__device__ __forceinline__ long long bam_record(const Record &r, uint8_t *out, int lane)
{
    const int l_name = r.name_len + 1;
    const int n_cigar = r.mapped ? r.n_ops : 0;
    const long long seq_bytes = (static_cast<long long>(r.read_len) + 1) >> 1;
    const long long cigar_at = 36 + l_name, seq_at = cigar_at + 4ll * n_cigar, qual_at = seq_at + seq_bytes, tags_at = qual_at + r.read_len;
    const long long md_at = tags_at + 10;                      // behind 'N' 'M' 'i' int32 'M' 'D' 'Z'
    const long long total = r.mapped ? md_at + r.md_bytes + 1 : tags_at;
    if (!EMIT) return total;

    const long long pos0 = static_cast<long long>(r.pos) - 1, next0 = static_cast<long long>(r.pnext) - 1;
    const long long tlen = r.tlen_negative ? -static_cast<long long>(r.tlen_abs) : static_cast<long long>(r.tlen_abs);
    const long long end = pos0 + (r.mapped && r.ref_bases > 0 ? r.ref_bases : 1);
    const unsigned bin = pos0 < 0 ? 4680u : reg2bin(pos0, end);
    if (lane < 36) {
        const int k = lane >> 2;
        const uint32_t word = k == 0 ? static_cast<uint32_t>(total - 4)
                            : k == 1 ? static_cast<uint32_t>(r.ref_id)
                            : k == 2 ? static_cast<uint32_t>(pos0)
                            : k == 3 ? (bin << 16 | r.mapq << 8 | static_cast<uint32_t>(l_name))
                            : k == 4 ? (r.flag << 16 | static_cast<uint32_t>(n_cigar))
                            : k == 5 ? static_cast<uint32_t>(r.read_len)
                            : k == 6 ? static_cast<uint32_t>(r.next_ref_id)
                            : k == 7 ? static_cast<uint32_t>(next0)
                                     : static_cast<uint32_t>(tlen);
        out[lane] = static_cast<uint8_t>(word >> (8 * (lane & 3)));
    }
    for (int j = lane; j < r.name_len; j += kLanes) out[36 + j] = r.name[j];
    if (lane == 0) out[36 + r.name_len] = 0;
    auto base = [&](int t) -> uint8_t {                        // base t of SEQ as the SAM line prints it
        uint8_t c = r.seq[r.reverse ? r.read_len - 1 - t : t];
        if (r.reverse) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
        return c;
    };
    for (long long j = lane; j < seq_bytes; j += kLanes) {
        const int t = static_cast<int>(2 * j);
        const unsigned high = seq_code(base(t)), low = t + 1 < r.read_len ? seq_code(base(t + 1)) : 0u;
        out[seq_at + j] = static_cast<uint8_t>(high << 4 | low);
    }
    for (int j = lane; j < r.read_len; j += kLanes)
        out[qual_at + j] = r.qual ? static_cast<uint8_t>(r.qual[r.reverse ? r.read_len - 1 - j : j] - 33) : static_cast<uint8_t>(0xff);
    if (r.mapped) {
        if (lane < 3) out[tags_at + lane] = static_cast<uint8_t>("NMi"[lane]);
        else if (lane < 7) out[tags_at + lane] = static_cast<uint8_t>(r.distance >> (8 * (lane - 3)));
        else if (lane < 10) out[tags_at + lane] = static_cast<uint8_t>("MDZ"[lane - 7]);
        walk_runs<kWalkBamWords>(r.runs, r.n_ops, r.ref, out + cigar_at, out + md_at, lane);
        if (lane == 0) out[md_at + r.md_bytes] = 0;
    }
    return total;
}

template <bool CONTIGS>
__global__ __launch_bounds__(256) void bam_measure_kernel(Batch b, Contigs ct, int64_t n, int64_t *__restrict__ lengths, int32_t *__restrict__ malformed)
{
    const int lane = threadIdx.x & (kLanes - 1);
    const int64_t i = static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= n) return;              // wave-uniform
    const Record r = check_record<CONTIGS>(b, ct, i);
    long long bytes = 0;
    if (r.ok && bam_fits(r)) bytes = bam_record<false>(r, nullptr, lane);
    else count_malformed(malformed, lane);
    if (lane == 0) lengths[i] = bytes;
}

template <bool CONTIGS>
__global__ __launch_bounds__(256) void bam_emit_kernel(Batch b, Contigs ct, int64_t n, const int64_t *__restrict__ offsets,
                                                       uint8_t *__restrict__ payload, int64_t payload_bytes, int32_t *__restrict__ malformed)
{
    const int lane = threadIdx.x & (kLanes - 1);
    const int64_t i = static_cast<int64_t>(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= n) return;              // wave-uniform
    const Record r = check_record<CONTIGS>(b, ct, i);
    const long long lo = uniform_i64(offsets[i]), hi = uniform_i64(offsets[i + 1]);
    // written only where the record is exactly what its offsets leave room for, inside the buffer
    if (!r.ok || !bam_fits(r) || lo < 0 || hi < lo || hi > payload_bytes || bam_record<false>(r, nullptr, lane) != hi - lo) {
        count_malformed(malformed, lane);
        return;
    }
    bam_record<true>(r, payload + lo, lane);
}

// The two launches, shared by the one-sequence calls (CONTIGS false, an empty table) and the contig ones.
template <bool CONTIGS>
int launch_measure(const Batch *batch, const Contigs &ct, int64_t n, int64_t *d_lengths, int32_t *d_malformed, void *stream)
{
    hipLaunchKernelGGL(bam_measure_kernel<CONTIGS>, dim3(static_cast<unsigned>((n + kWavesPerBlock - 1) / kWavesPerBlock)),
                       dim3(kWavesPerBlock * kLanes), 0, static_cast<hipStream_t>(stream), *batch, ct, n, d_lengths, d_malformed);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

template <bool CONTIGS>
int launch_emit(const Batch *batch, const Contigs &ct, int64_t n, const int64_t *d_offsets, uint8_t *d_payload, int64_t payload_bytes,
                int32_t *d_malformed, void *stream)
{
    hipLaunchKernelGGL(bam_emit_kernel<CONTIGS>, dim3(static_cast<unsigned>((n + kWavesPerBlock - 1) / kWavesPerBlock)),
                       dim3(kWavesPerBlock * kLanes), 0, static_cast<hipStream_t>(stream), *batch, ct, n, d_offsets, d_payload, payload_bytes,
                       d_malformed);
    BGSA_HIP_TRY(hipGetLastError());
    return BGSA_HIP_OK;
}

}  // namespace

}  // namespace bgsa

using namespace bgsa;

extern "C" {

int bgsa_hip_bam_measure_dev(const bgsa_hip_sam_batch_t *batch, int64_t n, int64_t *d_lengths, int32_t *d_malformed, void *stream)
{
    const char *who = "bam_measure_dev";
    if (int rc = check_batch(who, batch, n)) return rc;
    if (!d_lengths || !d_malformed) return refuse(who, BGSA_HIP_EINVAL, "d_lengths or d_malformed is NULL");
    if (n == 0) return BGSA_HIP_OK;
    return launch_measure<false>(batch, Contigs{}, n, d_lengths, d_malformed, stream);
}

int bgsa_hip_bam_emit_dev(const bgsa_hip_sam_batch_t *batch, int64_t n, const int64_t *d_offsets, uint8_t *d_payload, int64_t payload_bytes,
                          int32_t *d_malformed, void *stream)
{
    const char *who = "bam_emit_dev";
    if (int rc = check_batch(who, batch, n)) return rc;
    if (!d_offsets || !d_payload || !d_malformed) return refuse(who, BGSA_HIP_EINVAL, "d_offsets, d_payload or d_malformed is NULL");
    if (payload_bytes < 0) return refuse(who, BGSA_HIP_EINVAL, "payload_bytes is negative");
    if (n == 0) return BGSA_HIP_OK;
    return launch_emit<false>(batch, Contigs{}, n, d_offsets, d_payload, payload_bytes, d_malformed, stream);
}

int bgsa_hip_bam_measure_contigs_dev(const bgsa_hip_sam_batch_t *batch, const bgsa_hip_sam_contigs_t *contigs, int64_t n, int64_t *d_lengths,
                                     int32_t *d_malformed, void *stream)
{
    const char *who = "bam_measure_contigs_dev";
    if (int rc = check_contig_batch(who, batch, contigs, n)) return rc;
    if (!d_lengths || !d_malformed) return refuse(who, BGSA_HIP_EINVAL, "d_lengths or d_malformed is NULL");
    if (n == 0) return BGSA_HIP_OK;
    return launch_measure<true>(batch, *contigs, n, d_lengths, d_malformed, stream);
}

int bgsa_hip_bam_emit_contigs_dev(const bgsa_hip_sam_batch_t *batch, const bgsa_hip_sam_contigs_t *contigs, int64_t n, const int64_t *d_offsets,
                                  uint8_t *d_payload, int64_t payload_bytes, int32_t *d_malformed, void *stream)
{
    const char *who = "bam_emit_contigs_dev";
    if (int rc = check_contig_batch(who, batch, contigs, n)) return rc;
    if (!d_offsets || !d_payload || !d_malformed) return refuse(who, BGSA_HIP_EINVAL, "d_offsets, d_payload or d_malformed is NULL");
    if (payload_bytes < 0) return refuse(who, BGSA_HIP_EINVAL, "payload_bytes is negative");
    if (n == 0) return BGSA_HIP_OK;
    return launch_emit<true>(batch, *contigs, n, d_offsets, d_payload, payload_bytes, d_malformed, stream);
}

}  // extern "C"
