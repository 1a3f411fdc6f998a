"""Host model of a coordinate-sorted BAM's index (include/bgsa_hip.h "BAM records: coordinate order and index"; SAMv1 §5.2, §5.3),
in plain Python with struct and zlib: the coordinates and the sort key of a record, virtual offsets, the index arrays built from
sorted coordinates record by record, the .bai bytes both ways, and what a reader does with them — reg2bins, the region query of
§5.3 and a fetch that seeks by virtual offset.  Neither samtools, htslib nor pysam is needed: the region queries here stand in
for them.

DEFINITIONS (restated from the header).
  coordinates  refID, pos: a mapped record's contig index (0 on one sequence) and POS - 1; an unmapped end with rnext 1 takes its
               mate's; any other unmapped record -1, -1.  end: pos + (ref_end - ref_begin) mapped (pos + 1 where that is 0, as the
               record's own bin counts it), pos + 1 unmapped but placed, 0 with pos -1.  bin: reg2bin(pos, end) in full; 4680 with
               pos -1.
  key          ref' << 32 | (pos + 1) << 1 | reverse; ref' = refID, 0x7fffffff for -1; reverse = flag >> 4 & 1; ties keep input order.
  malformed    strand outside -1..1; rnext outside 0..1; pnext < 0; rnext 1 with pnext < 1; mapped with ref_begin < 0, ref_end <
               ref_begin or ref_end > ref_len; (contig form) ref_begin or pnext - 1 on no contig, or ref_end beyond the contig;
               pos + 1 or end beyond 2^29.  Key INT64_MAX, refID -1, pos -1, end 0, bin 4680.
  virtual offset  block_start(o // P) << 16 | o % P; block_start(b) = b * (P + 31) stored, block_offsets[b] deflated.
  chunks       over the sorted records with refID >= 0, every maximal run of equal (refID, bin): (refID, bin, voff_beg of the first,
               voff_end of the last); the list ordered by (refID, bin, beg).
  linear       ceil(len / 16384) windows per reference; the smallest voff_beg of a record with pos >> 14 <= w <= (end - 1) >> 14;
               n_intv = 1 + the last non-empty window; an empty window below it takes the next non-empty one's value.
  metadata     bin 37450 of a reference with records: (min voff_beg, max voff_end), (flag 4 clear, flag 4 set); n_no_coor: refID -1."""
import struct
import zlib

import bam_reference as M

INT64_MAX = 2 ** 63 - 1
NO_COORDINATE = 0x7fffffff
REACH = 1 << 29
META_BIN = 37450
UNPLACED = (INT64_MAX, -1, -1, 0, 4680)


# ---- a record's coordinates and key -----------------------------------------------------------------------------------------------------
def coordinates(rec: dict, ref_len: int, contigs=None) -> tuple:
    """(key, refID, pos, end, bin) of a record dict with strand, begin, end, flag, rnext, pnext (sam_reference.craft's keys).
    contigs: None for one sequence, else [(linear start, length), ...] with begin, end and pnext linear."""
    def locate(at):
        for c, (start, n) in enumerate(contigs):
            if start <= at < start + n:
                return c, start, start + n
        return None
    strand, rnext, pnext = rec["strand"], rec["rnext"], rec["pnext"]
    if not -1 <= strand <= 1 or rnext not in (0, 1) or pnext < 0 or (rnext == 1 and pnext < 1):
        return UNPLACED
    ref_id, pos, end = -1, -1, 0
    if rnext == 1:
        mate = (0, 0, ref_len) if contigs is None else locate(pnext - 1)
        if mate is None:
            return UNPLACED
        ref_id, pos = mate[0], pnext - 1 - mate[1]
        end = pos + 1
    if strand >= 0:
        begin, stop = rec["begin"], rec["end"]
        if begin < 0 or stop < begin or stop > ref_len:
            return UNPLACED
        own = (0, 0, ref_len) if contigs is None else locate(begin)
        if own is None or stop > own[2]:
            return UNPLACED
        ref_id, pos = own[0], begin - own[1]
        end = pos + max(stop - begin, 1)
    if pos + 1 > REACH or end > REACH:
        return UNPLACED
    return sort_key(ref_id, pos, rec["flag"]), ref_id, pos, end, 4680 if pos < 0 else M.reg2bin(pos, end)


def sort_key(ref_id: int, pos: int, flag: int) -> int:
    return (NO_COORDINATE if ref_id < 0 else ref_id) << 32 | (pos + 1) << 1 | (flag >> 4 & 1)


def decoded_coordinates(d: dict) -> tuple:
    """(key, refID, pos, end, bin) of a record bam_reference.decode returned: the reference bases of its CIGAR words."""
    span = sum(w >> 4 for w in d["cigar"] if w & 15 in (0, 2, 3, 7, 8))
    mapped = not d["flag"] & 4
    pos = d["pos"]
    end = 0 if pos < 0 else pos + (max(span, 1) if mapped else 1)
    return sort_key(d["ref_id"], pos, d["flag"]), d["ref_id"], pos, end, 4680 if pos < 0 else M.reg2bin(pos, end)


def virtual_offset(o: int, P: int, block_offsets=None) -> int:
    b = o // P
    return (b * (P + 31) if block_offsets is None else int(block_offsets[b])) << 16 | o % P


# ---- the index of sorted records -------------------------------------------------------------------------------------------------------
def windows(ref_lens) -> list:
    """window_base[n_refs + 1]: the exclusive scan of ceil(len / 16384)."""
    base = [0]
    for n in ref_lens:
        base.append(base[-1] + (int(n) + 16383) // 16384)
    return base


def build_index(ref_id, pos, end, bin_, offsets, P: int, block_offsets, ref_lens) -> dict:
    """The index of records in sorted order, one record at a time: voff_beg / voff_end per record, chunk_start per record, the
    chunks as (ref, bin, beg, end) in (ref, bin, beg) order, window_base, linear (flat, suffix minima, INT64_MAX behind the last
    record) and n_intv."""
    n = len(ref_id)
    base = windows(ref_lens)
    beg = [virtual_offset(int(offsets[i]), P, block_offsets) for i in range(n)]
    stop = [virtual_offset(int(offsets[i + 1]), P, block_offsets) for i in range(n)]
    raw = [INT64_MAX] * base[-1]
    chunks, starts = [], []
    for i in range(n):
        r = int(ref_id[i])
        start = r >= 0 and (i == 0 or (int(ref_id[i - 1]), int(bin_[i - 1])) != (r, int(bin_[i])))
        starts.append(int(start))
        if r < 0:
            continue
        if start:
            chunks.append([r, int(bin_[i]), beg[i], stop[i]])
        else:
            chunks[-1][3] = stop[i]
        for w in range(int(pos[i]) >> 14, (int(end[i]) - 1 >> 14) + 1):
            raw[base[r] + w] = min(raw[base[r] + w], beg[i])
    order = sorted(range(len(chunks)), key=lambda c: (chunks[c][0], chunks[c][1], chunks[c][2]))
    n_intv = [max([w + 1 for w in range(base[c + 1] - base[c]) if raw[base[c] + w] != INT64_MAX], default=0) for c in range(len(ref_lens))]
    linear = list(raw)
    for w in range(len(linear) - 2, -1, -1):
        linear[w] = min(linear[w], linear[w + 1])
    return dict(voff_beg=beg, voff_end=stop, chunk_start=starts, chunks=[tuple(chunks[c]) for c in order], window_base=base, linear=linear,
                n_intv=n_intv, raw_linear=raw, ref_lens=[int(x) for x in ref_lens])


def bai_bytes(index: dict, flag, ref_id, base: int = 0) -> bytes:
    """The .bai bytes of build_index's dict and the sorted records' flag and ref_id columns; every offset moved by base << 16."""
    shift = base << 16
    out = [b"BAI\x01", struct.pack("<i", len(index["ref_lens"]))]
    for c in range(len(index["ref_lens"])):
        mine = [x for x in index["chunks"] if x[0] == c]
        if not mine:
            out.append(struct.pack("<ii", 0, 0))
            continue
        bins = sorted({x[1] for x in mine})
        out.append(struct.pack("<i", len(bins) + 1))
        for b in bins:
            of_bin = [x for x in mine if x[1] == b]
            out.append(struct.pack("<Ii", b, len(of_bin)))
            out += [struct.pack("<QQ", x[2] + shift, x[3] + shift) for x in of_bin]
        own = [int(f) for f, r in zip(flag, ref_id) if int(r) == c]
        out.append(struct.pack("<Ii4Q", META_BIN, 2, min(x[2] for x in mine) + shift, max(x[3] for x in mine) + shift,
                               sum(1 for f in own if not f & 4), sum(1 for f in own if f & 4)))
        at, k = index["window_base"][c], index["n_intv"][c]
        out.append(struct.pack("<i", k))
        out += [struct.pack("<Q", v + shift) for v in index["linear"][at: at + k]]
    out.append(struct.pack("<Q", sum(1 for r in ref_id if int(r) < 0)))
    return b"".join(out)


def parse_bai(data: bytes) -> dict:
    """A .bai file as dict(refs=[dict(bins={bin: [(beg, end), ...]}, meta=None or ((beg, end), (mapped, unmapped)), linear=[...])],
    n_no_coor); every byte is consumed."""
    assert data[:4] == b"BAI\x01"
    n_ref, at, refs = struct.unpack_from("<i", data, 4)[0], 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", data, at)[0]
        at += 4
        bins, meta, seen = {}, None, []
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", data, at)
            at += 8
            pairs = [struct.unpack_from("<QQ", data, at + 16 * k) for k in range(n_chunk)]
            at += 16 * n_chunk
            seen.append(b)
            if b == META_BIN:
                assert n_chunk == 2
                meta = (pairs[0], pairs[1])
            else:
                assert n_chunk >= 1 and b not in bins and all(lo < hi for lo, hi in pairs)
                bins[b] = pairs
        assert seen == sorted(seen) and (not seen or seen[-1] == META_BIN)
        n_intv = struct.unpack_from("<i", data, at)[0]
        at += 4
        linear = list(struct.unpack_from(f"<{n_intv}Q", data, at))
        at += 8 * n_intv
        refs.append(dict(bins=bins, meta=meta, linear=linear))
    n_no_coor = struct.unpack_from("<Q", data, at)[0]
    assert at + 8 == len(data)
    return dict(refs=refs, n_no_coor=n_no_coor)


# ---- what a reader does -----------------------------------------------------------------------------------------------------------------
def reg2bins(beg: int, end: int) -> list:
    """SAMv1 §5.3: every bin that may hold a record overlapping [beg, end)."""
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += range(first + (beg >> shift), first + (end >> shift) + 1)
    return out


def query(parsed: dict, ref: int, beg: int, end: int) -> list:
    """The chunks a reader visits for [beg, end) of reference `ref`: those of reg2bins' bins, minus the ones that end at or before
    linear[beg >> 14] (no window that far: no lower bound), sorted by begin."""
    one = parsed["refs"][ref]
    w = beg >> 14
    floor = one["linear"][w] if w < len(one["linear"]) else (one["linear"][-1] if one["linear"] else 0)
    out = [pair for b in reg2bins(beg, end) for pair in one["bins"].get(b, ()) if pair[1] > floor]
    return sorted(out)


def block_at(file_bytes: bytes, at: int) -> tuple:
    """(payload, the block's length) of the BGZF block at file offset `at`."""
    assert file_bytes[at: at + 4] == b"\x1f\x8b\x08\x04" and file_bytes[at + 12: at + 16] == b"BC\x02\x00", at
    size = struct.unpack_from("<H", file_bytes, at + 16)[0] + 1
    piece = zlib.decompress(file_bytes[at + 18: at + size - 8], -15)
    assert struct.unpack_from("<II", file_bytes, at + size - 8) == (zlib.crc32(piece), len(piece))
    return piece, size


def fetch(file_bytes: bytes, chunks) -> list:
    """The records (block_size included) of every chunk (beg, end), in order: a seek to beg >> 16, the block inflated, records read
    from beg & 0xffff on — across blocks where they straddle — until the reader's own virtual offset reaches end."""
    out = []
    for beg, end in chunks:
        at, within = beg >> 16, beg & 0xffff
        piece, size = block_at(file_bytes, at)

        def take(k):
            nonlocal at, within, piece, size
            got = b""
            while k:
                if within == len(piece):
                    at, within = at + size, 0
                    piece, size = block_at(file_bytes, at)
                    continue
                step = piece[within: within + k]
                got += step
                within += len(step)
                k -= len(step)
            return got

        while True:
            now = at << 16 | within
            if now >= end or (within == len(piece) and (at + size) << 16 >= end):
                break
            head = take(4)
            out.append(head + take(struct.unpack("<i", head)[0]))
    return out


def overlaps(ref_id, pos, end, ref: int, beg: int, stop: int) -> list:
    """Brute force: the indices of the records of `ref` with pos < stop and end > beg."""
    return [i for i in range(len(ref_id)) if int(ref_id[i]) == ref and int(pos[i]) < stop and int(end[i]) > beg]
