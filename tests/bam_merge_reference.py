"""Host model of the merge of many calls' BAM records (include/bgsa_hip.h "BAM records: merge"), in plain Python
and the normative definition: no device, no library, one byte at a time.

  gather   output record i is source record s = order[i], the bytes src[src_offsets[s] : src_offsets[s + 1]]; in the sorted payload
           it occupies [dst_offsets[i], dst_offsets[i + 1]).  A call handles the output records first .. first + count - 1 and
           writes of each exactly the bytes whose sorted-payload position p lies in [lo, hi).  With `flag`, the record's bytes 18
           and 19 are flag[s] & 0xffff, little-endian; each of the two is written or not by the window rule on its own.  A record
           is refused — counted, not a byte of it written — when s is outside the source records, an offset pair is negative or
           not monotone, the source extent leaves src, the two lengths differ, or `flag` is given and the length is below 20.
  merged   the records of all batches in batch-major input order; their keys (the key of "coordinate order and index", which
           reads bit 16 of the flag only) sorted with ties in input order; with marking, the duplicate rule of "Duplicate marking"
           over ALL records, ties to the lowest global index, and bit 1024 ORed into bytes 18 | 19 of the flagged records and
           nowhere else; the sorted records laid end to end; the index of bai_reference over them.  That is what ONE sort=True
           call on the concatenated reads writes."""
import bai_reference as R
import bam_reference as M
import markdup_reference as MD

FLAG_AT = 18          # a BAM record's flag: two bytes, little-endian, counted from the start of its block_size field


def refused(src_bytes: int, src_offsets, n_src: int, s: int, d: int, d_end: int, with_flag: bool) -> bool:
    if s < 0 or s >= n_src or d < 0 or d_end < d:
        return True
    a, a_end = src_offsets[s], src_offsets[s + 1]
    if a < 0 or a_end < a or a_end > src_bytes or a_end - a != d_end - d:
        return True
    return with_flag and a_end - a < FLAG_AT + 2


def gather(src: bytes, src_offsets, order, dst_offsets, first: int, count: int, lo: int, hi: int, flag=None) -> tuple:
    """({sorted-payload position: byte} of what the call writes, the refused records' count)."""
    written, bad = {}, 0
    n_src = len(src_offsets) - 1
    for i in range(first, first + count):
        s, d, d_end = int(order[i]), int(dst_offsets[i]), int(dst_offsets[i + 1])
        if refused(len(src), src_offsets, n_src, s, d, d_end, flag is not None):
            bad += 1
            continue
        a = int(src_offsets[s])
        for j in range(max(0, lo - d), min(d_end, hi) - d):       # the bytes with lo <= d + j < hi
            byte = src[a + j]
            if flag is not None and j in (FLAG_AT, FLAG_AT + 1):
                byte = (int(flag[s]) & 0xffff) >> (8 * (j - FLAG_AT)) & 0xff
            assert d + j not in written, "two records write one byte"
            written[d + j] = byte
    return written, bad


def flag_of(record: bytes) -> int:
    return record[FLAG_AT] | record[FLAG_AT + 1] << 8


def merged(batches, P: int, starts, ref_lens, ref_names, mark_duplicates: bool = False, paired: bool = False) -> dict:
    """The one-call result of the batches' records.  batches: per batch the list of its records' bytes (block_size included) in
    input order; starts: the deflated blocks' starts (n_blocks + 1 entries) or None for stored blocks of P payload bytes.
    Returns records (sorted, patched), order (global input indices), offsets, flag (sorted), stats (or None) and index
    (bai_reference.build_index's dict)."""
    records = [x for batch in batches for x in batch]
    n = len(records)
    decoded = [M.decode(x, ref_names) for x in records]
    flags, stats = [flag_of(x) for x in records], None
    if mark_duplicates:
        flagged, stats = MD.duplicates_of_sam([d["line"] for d in decoded], paired)
        flags = [f | MD.DUPLICATE if i in flagged else f for i, f in enumerate(flags)]
    coords = [R.decoded_coordinates(d) for d in decoded]
    order = sorted(range(n), key=lambda i: (coords[i][0], i))                  # a stable sort of the keys
    src_offsets, dst_offsets = [0], [0]
    for x in records:
        src_offsets.append(src_offsets[-1] + len(x))
    for i in order:
        dst_offsets.append(dst_offsets[-1] + len(records[i]))
    written, bad = gather(b"".join(records), src_offsets, order, dst_offsets, 0, n, 0, dst_offsets[-1], flags)
    assert bad == 0 and sorted(written) == list(range(dst_offsets[-1]))
    payload = bytes(written[p] for p in range(dst_offsets[-1]))
    out = [payload[a:b] for a, b in zip(dst_offsets, dst_offsets[1:])]
    for i, x in zip(order, out):                                               # nothing but the flag's two bytes changed
        assert x[:FLAG_AT] == records[i][:FLAG_AT] and x[FLAG_AT + 2:] == records[i][FLAG_AT + 2:] and flag_of(x) == flags[i]
    sorted_coords = [coords[i] for i in order]
    index = R.build_index([c[1] for c in sorted_coords], [c[2] for c in sorted_coords], [c[3] for c in sorted_coords],
                          [c[4] for c in sorted_coords], dst_offsets, P, starts, ref_lens)
    return dict(records=out, order=order, offsets=dst_offsets, flag=[flags[i] for i in order], ref_id=[c[1] for c in sorted_coords], stats=stats,
                index=index)
