"""Host model of the pileup (include/bgsa_hip.h "Pileup"), in plain Python and numpy.  Two readings of the same definitions:
pileup_of_batch walks the record dicts tests/test_bam_gpu.py: Batch takes (the read as handed to the mapper, the run words, the
interval, the strand); pileup_of_sam knows nothing of the batch and reads FLAG, POS, MAPQ, CIGAR, SEQ and QUAL of SAM text alone.
sites_of is the site test on a count matrix.  The count matrix is int32[ref_len][8]: A, C, G, T, other, deleted, inserted, reverse."""
import re

import numpy as np

COLUMNS = 8
OTHER, DELETED, INSERTED, REVERSE = 4, 5, 6, 7
STATS = ("records_used", "records_filtered", "records_malformed", "bases_counted", "bases_low_quality")
EXCLUDE = 0x704
COMPLEMENT = {65: 84, 67: 71, 71: 67, 84: 65}
REF_ONLY, READ_ONLY, EQUAL, DIFF = 1, 2, 7, 8      # the project's run codes; REF_ONLY prints as SAM D, READ_ONLY as SAM I


def base_class(byte: int) -> int:
    return b"ACGT".index(byte) if byte in b"ACGT" else OTHER


def as_written(read: bytes, qual, reverse: bool) -> tuple:
    """SEQ and QUAL of the record as the SAM stage writes it."""
    if not reverse:
        return read, qual
    return bytes(COMPLEMENT.get(c, 78) for c in reversed(read)), None if qual is None else qual[::-1]


def malformed(rec: dict, index: int, limits) -> bool:
    """The rules of "SAM records" on a record dict; limits: ref_len, stride, n_rows, cap (None: only the runs are checked)."""
    words = [int(w) for w in rec["words"]]
    read_len = rec.get("read_len", len(rec["read"]))
    if limits is not None:
        if not -1 <= rec["strand"] <= 1 or not 1 <= read_len <= limits["stride"] or not 0 <= rec.get("read_row", index) < limits["n_rows"]:
            return True
        if not 0 <= rec["flag"] <= 65535 or not 0 <= rec["mapq"] <= 255:
            return True
    if rec["strand"] < 0:
        return False
    if limits is not None and (rec.get("n_ops", len(words)) > limits["cap"] or not 0 <= rec["begin"] <= rec["end"] <= limits["ref_len"]):
        return True
    n_ops = rec.get("n_ops", len(words))
    words = (words + [0] * max(n_ops - len(words), 0))[:n_ops]      # the row behind the record's own runs holds zeros
    if any(w & 15 not in (REF_ONLY, READ_ONLY, EQUAL, DIFF) or w >> 4 == 0 for w in words):
        return True
    on_ref = sum(w >> 4 for w in words if w & 15 != READ_ONLY)
    on_read = sum(w >> 4 for w in words if w & 15 != REF_ONLY)
    return on_ref != rec["end"] - rec["begin"] or on_read != read_len


def walk(counts, stats, runs, begin: int, end: int, seq: bytes, qual, reverse: bool, min_base_quality: int) -> None:
    """The normative walk: runs [(length, op)] with the project's run codes, seq and qual as written."""
    p, j = begin, 0
    for n, op in runs:
        if op in (EQUAL, DIFF):
            for t in range(n):
                if qual is not None and qual[j + t] - 33 < min_base_quality:
                    stats[4] += 1
                    continue
                counts[p + t, base_class(seq[j + t])] += 1
                counts[p + t, REVERSE] += reverse
                stats[3] += 1
            p, j = p + n, j + n
        elif op == REF_ONLY:
            counts[p: p + n, DELETED] += 1
            counts[p: p + n, REVERSE] += reverse
            p += n
        else:
            if begin < p < end:
                counts[p - 1, INSERTED] += 1
            j += n
    assert p == end and j == len(seq)


def pileup_of_batch(records, quals, ref_len: int, min_mapq: int = 0, min_base_quality: int = 13, exclude_flags: int = EXCLUDE, limits=None,
                    into=None) -> tuple:
    """(counts, stats) of record dicts; into: a (counts, stats) pair to add to."""
    counts, stats = (np.zeros((ref_len, COLUMNS), np.int32), [0] * 5) if into is None else into
    for i, rec in enumerate(records):
        if malformed(rec, i, limits):
            stats[2] += 1
        elif rec["strand"] < 0 or rec["flag"] & exclude_flags or rec["mapq"] < min_mapq:
            stats[1] += 1
        else:
            stats[0] += 1
            reverse = rec["strand"] == 1
            seq, qual = as_written(rec["read"], None if quals is None else quals[i], reverse)
            walk(counts, stats, [(int(w) >> 4, int(w) & 15) for w in rec["words"]], rec["begin"], rec["end"], seq, qual, reverse, min_base_quality)
    return counts, stats


SAM_OP = {"=": EQUAL, "X": DIFF, "D": REF_ONLY, "I": READ_ONLY}


def pileup_of_sam(lines, ref_len: int, min_mapq: int = 0, min_base_quality: int = 13, exclude_flags: int = EXCLUDE, starts=None, into=None) -> tuple:
    """(counts, stats) from SAM lines alone.  starts: {RNAME: the contig's linear start} where POS is local to a contig."""
    counts, stats = (np.zeros((ref_len, COLUMNS), np.int32), [0] * 5) if into is None else into
    for line in lines:
        f = line.rstrip(b"\n").split(b"\t")
        flag, pos, mapq, cigar, seq, qual = int(f[1]), int(f[3]), int(f[4]), f[5].decode(), f[9], f[10]
        if flag & 4 or flag & exclude_flags or mapq < min_mapq:
            stats[1] += 1
            continue
        stats[0] += 1
        runs = [(int(n), SAM_OP[op]) for n, op in re.findall(r"(\d+)([=XDI])", cigar)]
        assert "".join(f"{n}{op}" for n, op in re.findall(r"(\d+)([=XDI])", cigar)) == cigar, cigar
        begin = pos - 1 + (0 if starts is None else starts[f[2]])
        end = begin + sum(n for n, op in runs if op != READ_ONLY)
        walk(counts, stats, runs, begin, end, seq, None if qual == b"*" else qual, bool(flag & 16), min_base_quality)
    return counts, stats


def sites_of(counts, reference_codes, min_cover: int = 8, min_alt: int = 3, min_percent: int = 20) -> dict:
    """The candidate sites of a count matrix over the reference's codes 0..4, in ascending position: a dict of numpy arrays."""
    out = dict(pos=[], ref=[], alt=[], alt_count=[], cover=[], alts_mask=[])
    for p in range(len(counts)):
        row = [int(x) for x in counts[p]]
        r, cover = int(reference_codes[p]), sum(row[:6])
        qualifying = [a for a in (0, 1, 2, 3, 5, 6) if a != r and row[a] >= min_alt and 100 * row[a] >= min_percent * cover]
        if r < 4 and cover >= min_cover and qualifying:
            alt = max(qualifying, key=lambda a: (row[a], -a))
            for key, value in zip(out, (p, r, alt, row[alt], cover, sum(1 << a for a in qualifying))):
                out[key].append(value)
    kinds = dict(pos=np.int64, ref=np.uint8, alt=np.uint8, alt_count=np.int32, cover=np.int32, alts_mask=np.uint8)
    return {key: np.array(value, dtype=kinds[key]) for key, value in out.items()}


def sites_of_fast(counts, reference_codes, min_cover: int = 8, min_alt: int = 3, min_percent: int = 20) -> dict:
    """sites_of for a long matrix: the rows that can be sites picked with numpy (a necessary condition), the test itself sites_of's."""
    counts = np.asarray(counts)
    maybe = np.flatnonzero((counts[:, [0, 1, 2, 3, 5, 6]].max(axis=1) >= min_alt) & (np.asarray(reference_codes) < 4))
    found = sites_of(counts[maybe], np.asarray(reference_codes)[maybe], min_cover, min_alt, min_percent)
    found["pos"] = maybe[found["pos"]].astype(np.int64)
    return found
