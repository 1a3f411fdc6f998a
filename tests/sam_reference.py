"""Host model of the SAM stage (include/bgsa_hip.h "SAM records"), in plain Python: from a ReferenceHits or PairedHits as the
existing entry points return them — CIGAR strings and all —, the reads, names, quals and the ASCII reference, the lines the device
must write.  The MAPQ formulas and the pair fields are restated here; MD comes from this file's own walk of the CIGAR string over
the reference.  craft() is the model's inverse: a read, its runs and its interval from an edit script, with no mapping involved."""
import re

import numpy as np

TO_SAM = {"I": "D", "D": "I", "=": "=", "X": "X"}      # the project's window-is-the-query letters -> SAM's
RUN_CODE = {"D": 1, "I": 2, "=": 7, "X": 8}            # SAM letter -> the project's run code (length << 4 | code)
COMPLEMENT = {65: 84, 67: 71, 71: 67, 84: 65}


def reverse_complement(seq: bytes) -> bytes:
    return bytes(COMPLEMENT.get(c, 78) for c in reversed(seq))


def sam_runs(cigar: str) -> list:
    """[(length, SAM letter)] of one of the project's CIGAR strings."""
    runs = [(int(n), TO_SAM[op]) for n, op in re.findall(r"(\d+)([IDX=])", cigar)]
    assert "".join(f"{n}{TO_SAM_BACK[op]}" for n, op in runs) == cigar
    return runs


TO_SAM_BACK = {v: k for k, v in TO_SAM.items()}


def cigar_text(runs) -> str:
    return "".join(f"{n}{op}" for n, op in runs)


def md_text(runs, reference: bytes, begin: int) -> str:
    """MD:Z of SAM runs laid along reference[begin:]: the count of '=' bases runs through I runs, is written (even 0) and reset
    before every X base and every D run, and is written once more at the end."""
    out, count, at = [], 0, begin
    for n, op in runs:
        if op == "=":
            count += n
            at += n
        elif op == "X":
            for _ in range(n):
                out.append(str(count) + chr(reference[at]))
                count = 0
                at += 1
        elif op == "D":
            out.append(str(count) + "^" + reference[at: at + n].decode())
            count = 0
            at += n
    return "".join(out) + str(count)


def consumed(runs) -> tuple:
    """(reference bases, read bases, X + I + D bases) of SAM runs."""
    return (sum(n for n, op in runs if op in "=XD"), sum(n for n, op in runs if op in "=XI"), sum(n for n, op in runs if op in "XID"))


def rebuild_reference(seq: bytes, cigar: str, md: str) -> bytes:
    """The reference bases a record spans, from its SEQ, CIGAR and MD alone (the round trip the model checks itself with)."""
    runs = [(int(n), op) for n, op in re.findall(r"(\d+)([IDX=])", cigar)]
    aligned, at = bytearray(), 0            # the read bases that sit on reference bases
    for n, op in runs:
        if op in "=X":
            aligned += seq[at: at + n]
        if op in "=XI":
            at += n
    assert re.fullmatch(r"[0-9]+(([ACGTN]|\^[ACGTN]+)[0-9]+)*", md), md
    out, at = bytearray(), 0
    for count, deleted, letter in re.findall(r"(\d+)|\^([ACGTN]+)|([ACGTN])", md):
        if count:
            out += aligned[at: at + int(count)]
            at += int(count)
        elif deleted:
            out += deleted.encode()
        else:
            out += letter.encode()
            at += 1
    assert at == len(aligned)
    return bytes(out)


# ---- MAPQ -----------------------------------------------------------------------------------------------------------------------
def table(n: int) -> int:
    return {2: 3, 3: 2}.get(n, 1 if n <= 9 else 0)


def list_fields(scores, keep, bound: int) -> tuple:
    """(primary slot, mapq, n1, d2) of one read's list."""
    kept = [r for r in range(len(keep)) if keep[r] != 0]
    if not kept:
        return -1, 0, 0, -1
    d1 = -int(scores[kept[0]])
    n1 = sum(1 for r in kept if -int(scores[r]) == d1)
    above = [-int(scores[r]) for r in kept if -int(scores[r]) > d1]
    d2 = min(above) if above else -1
    if n1 >= 2:
        return kept[0], table(n1), n1, d2
    gap = d2 - d1 if above else (bound + 1 - d1 if bound >= 0 else 6)
    return kept[0], max(0, min(60, 10 * gap)), n1, d2


def pair_fields(proper: int, n_best: int, cost: int, next_cost: int, alone1: int, alone2: int) -> tuple:
    if not proper:
        return alone1, alone2
    both = table(n_best) if n_best >= 2 else (60 if next_cost == -1 else min(60, 10 * (next_cost - cost)))
    return both, both


def tlen_fields(begin1: int, end1: int, begin2: int, end2: int) -> tuple:
    """(TLEN of end 1, of end 2) of two mapped ends: rightmost end minus leftmost begin, positive for the end with the smaller begin,
    end 1 on equal begins."""
    span = max(end1, end2) - min(begin1, begin2)
    return (span, -span) if begin1 <= begin2 else (-span, span)


# ---- lines ----------------------------------------------------------------------------------------------------------------------
def line(name: bytes, flag: int, rname: bytes, pos: int, mapq: int, cigar: str, rnext: bytes, pnext: int, tlen: int, seq: bytes, qual,
         nm=None, md=None) -> bytes:
    fields = [name, str(flag).encode(), rname, str(pos).encode(), str(mapq).encode(), cigar.encode(), rnext, str(pnext).encode(),
              str(tlen).encode(), seq, b"*" if qual is None else qual]
    if nm is not None:
        fields += [b"NM:i:" + str(nm).encode(), b"MD:Z:" + md.encode()]
    return b"\t".join(fields) + b"\n"


def placed(hits, c: int, r: int, read: bytes, qual, reference: bytes) -> dict:
    """What slot r of read c's list prints as: SEQ, QUAL, CIGAR, NM, MD, POS and the interval; r -1: the unmapped fields."""
    if r < 0:
        return dict(mapped=False, reverse=False, seq=read, qual=qual, cigar="*", pos=0, begin=-1, end=-1, nm=None, md=None)
    runs = sam_runs(hits.cigars[c][r])
    begin, end, reverse = int(hits.ref_begin[c, r]), int(hits.ref_end[c, r]), int(hits.strand[c, r]) == 1
    assert consumed(runs)[:2] == (end - begin, len(read))
    return dict(mapped=True, reverse=reverse, seq=reverse_complement(read) if reverse else read,
                qual=None if qual is None else (qual[::-1] if reverse else qual), cigar=cigar_text(runs), pos=begin + 1, begin=begin, end=end,
                nm=-int(hits.scores[c, r]), md=md_text(runs, reference, begin))


def default_names(n: int) -> list:
    return [f"r{i}".encode() for i in range(n)]


def single_records(hits, reads, names, quals, reference: bytes, rname: bytes, bound: int) -> tuple:
    """(lines, flag, pos, mapq, nm) of map_reads_sam from the result of the map_reads entry point on the same arguments."""
    names = default_names(len(reads)) if names is None else names
    lines, flags, poss, mapqs, nms = [], [], [], [], []
    for c, read in enumerate(reads):
        read = bytes(read)
        slot, mapq, _, _ = list_fields(hits.scores[c], hits.keep[c], bound)
        p = placed(hits, c, slot, read, None if quals is None else bytes(quals[c]), reference)
        flag = (16 if p["reverse"] else 0) if p["mapped"] else 4
        lines.append(line(names[c], flag, rname if p["mapped"] else b"*", p["pos"], mapq, p["cigar"], b"*", 0, 0, p["seq"], p["qual"], p["nm"], p["md"]))
        flags.append(flag)
        poss.append(p["pos"])
        mapqs.append(mapq)
        nms.append(-1 if p["nm"] is None else p["nm"])
    return lines, flags, poss, mapqs, nms


def pair_records(paired, reads1, reads2, names, quals1, quals2, reference: bytes, rname: bytes, bounds) -> tuple:
    """(lines, flag, pos, mapq, nm) of map_pairs_sam from map_pairs' result: two records per pair, end 1 then end 2."""
    names = default_names(len(reads1)) if names is None else names
    lines, flags, poss, mapqs, nms = [], [], [], [], []
    for c in range(len(reads1)):
        ends = []
        for hits, slot, reads, quals in ((paired.end1, paired.slot1, reads1, quals1), (paired.end2, paired.slot2, reads2, quals2)):
            ends.append(placed(hits, c, int(slot[c]), bytes(reads[c]), None if quals is None else bytes(quals[c]), reference))
        alone = [list_fields(hits.scores[c], hits.keep[c], bound) for hits, bound in zip((paired.end1, paired.end2), bounds)]
        assert [a[0] for a in alone] == [int(paired.slot1[c]), int(paired.slot2[c])] or paired.proper[c]
        mapq = pair_fields(int(paired.proper[c]), int(paired.n_best[c]), int(paired.cost[c]), int(paired.next_cost[c]), alone[0][1], alone[1][1])
        tlen = tlen_fields(ends[0]["begin"], ends[0]["end"], ends[1]["begin"], ends[1]["end"]) if ends[0]["mapped"] and ends[1]["mapped"] else (0, 0)
        for e, (me, mate) in enumerate(((ends[0], ends[1]), (ends[1], ends[0]))):
            flag = 1 | (2 if paired.proper[c] else 0) | (0 if me["mapped"] else 4) | (0 if mate["mapped"] else 8) | \
                (16 if me["reverse"] else 0) | (32 if mate["reverse"] else 0) | (64, 128)[e]
            named = me["mapped"] or mate["mapped"]
            pos = me["pos"] if me["mapped"] else mate["pos"]
            lines.append(line(names[c], flag, rname if named else b"*", pos, mapq[e] if me["mapped"] else 0, me["cigar"],
                              b"=" if mate["mapped"] else b"*", mate["pos"] if mate["mapped"] else 0, tlen[e], me["seq"], me["qual"], me["nm"],
                              me["md"]))
            flags.append(flag)
            poss.append(pos)
            mapqs.append(mapq[e] if me["mapped"] else 0)
            nms.append(-1 if me["nm"] is None else me["nm"])
    return lines, flags, poss, mapqs, nms


# ---- the inverse: a record from an edit script -------------------------------------------------------------------------------------
def craft(rng, reference: bytes, begin: int, runs, reverse: bool = False) -> dict:
    """A read that aligns to reference[begin:] by the SAM runs [(length, letter)]: '=' copies the reference, X writes another base
    (a reference N gives A), I writes random bases, D skips.  reverse: the read handed to the mapper is the reverse complement of
    that sequence.  Returns the read, the project's run words, the interval and the distance."""
    seq, at = bytearray(), begin
    for n, op in runs:
        if op == "=":
            seq += reference[at: at + n]
        elif op == "X":
            seq += bytes(b"CGTA"[b"ACGT".index(c)] if c in b"ACGT" else 65 for c in reference[at: at + n])
        elif op == "I":
            seq += bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=n).tolist())
        if op in "=XD":
            at += n
    assert at <= len(reference)
    words = np.array([n << 4 | RUN_CODE[op] for n, op in runs], dtype=np.uint32)
    forward = bytes(seq)
    return dict(read=reverse_complement(forward) if reverse else forward, forward=forward, words=words, begin=begin, end=at,
                distance=consumed(runs)[2], strand=1 if reverse else 0, runs=list(runs))


def crafted_line(rec: dict, name: bytes, qual, reference: bytes, rname: bytes, flag: int, mapq: int, rnext: int = 0, pnext: int = 0,
                 tlen: int = 0) -> bytes:
    """The line of a crafted record, by the model's forward direction."""
    reverse = rec["strand"] == 1
    return line(name, flag, rname, rec["begin"] + 1, mapq, cigar_text(rec["runs"]), b"=" if rnext else b"*", pnext, tlen, rec["forward"],
                None if qual is None else (qual[::-1] if reverse else qual), rec["distance"], md_text(rec["runs"], reference, rec["begin"]))
