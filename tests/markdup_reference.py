"""Host model of duplicate marking (include/bgsa_hip.h "Duplicate marking"), in plain Python and the normative definition: record by
record, with dictionaries, no sorting tricks.  The Picard core — no optical duplicates, no UMIs, no libraries.

A record is a dict with strand (-1 unmapped, 0 forward, 1 reverse), begin, end (the reference interval, linear) and read (its
bytes); read_len and read_row may be given where they differ from len(read) and the record's index (a malformed record).
  mapped        strand >= 0.
  5' coordinate begin on strand 0; end - 1 on strand 1 (begin where end == begin): the coordinate of the record AS WRITTEN.
  units         ends 1: every mapped record is a fragment unit.  ends 2: records 2u and 2u + 1 are pair u; both mapped: a pair unit;
                exactly one mapped: that end is a fragment unit.  Unmapped records are in no unit and are never flagged.
  score         of a unit: the sum of q - 33 over the QUAL bytes of its mapped records with q - 33 >= min_quality; 0 without QUAL.
  pair pass     the pair key is the two ends' (5', strand), the smaller first.  Among pair units of equal key the highest score
                stays, a tie goes to the lowest pair index; both records of every other one are flagged.
  end pass      every mapped record of a unit is an entry with key (5', strand), paired or fragment.  A group with a paired entry:
                every fragment in it is a duplicate.  Otherwise the fragment of the highest score stays, a tie goes to the lowest
                record index.  Paired entries are never flagged here; nor is the unmapped mate of a duplicate fragment.
  malformed     strand outside -1..1, read_len < 0 or above the row stride, read_row outside the rows, or — mapped — begin < 0,
                end < begin, end > ref_len: the record takes its whole unit out of marking and counts as skipped."""
INT64_MAX = 2 ** 63 - 1
INT32_MAX = 2 ** 31 - 1
DUPLICATE = 0x400
STATS = ("pair_units", "fragment_units", "duplicate_pair_units", "duplicate_fragment_units", "records_flagged", "records_skipped")


def five_prime(rec: dict) -> int:
    return rec["end"] - 1 if rec["strand"] == 1 and rec["end"] > rec["begin"] else rec["begin"]


def malformed(rec: dict, index: int, limits) -> bool:
    """limits: dict(ref_len, stride, n_rows), or None: nothing is checked but the strand."""
    if not -1 <= rec["strand"] <= 1:
        return True
    if limits is None:
        return False
    read_len, row = rec.get("read_len", len(rec["read"])), rec.get("read_row", index)
    if read_len < 0 or read_len > limits["stride"] or row < 0 or row >= limits["n_rows"]:
        return True
    return rec["strand"] >= 0 and (rec["begin"] < 0 or rec["end"] < rec["begin"] or rec["end"] > limits["ref_len"])


def quality_sum(qual, min_quality: int = 15) -> int:
    return 0 if qual is None else min(sum(q - 33 for q in qual if q - 33 >= min_quality), INT32_MAX)


def mark(entries, ends: int) -> tuple:
    """The two passes.  entries[i]: None where record i is in no unit, else (key, score): key = (5', strand) — with whatever names
    the reference in front —, score that record's own sum.  Returns (the flagged record indices, the stats without records_skipped)."""
    assert ends in (1, 2) and len(entries) % ends == 0
    pairs, fragments = [], []                                 # (records, score) in input order
    for u in range(len(entries) // ends):
        members = [i for i in range(u * ends, (u + 1) * ends) if entries[i] is not None]
        if len(members) == 2:
            pairs.append((members, entries[members[0]][1] + entries[members[1]][1]))
        else:
            fragments += [([i], entries[i][1]) for i in members]
    flagged, best = set(), {}
    for members, score in pairs:                              # the pair pass
        key = tuple(sorted(entries[i][0] for i in members))
        if key not in best or score > best[key][1]:
            best[key] = (members, score)
    dup_pairs = [members for members, _ in pairs if best[tuple(sorted(entries[i][0] for i in members))][0] is not members]
    for members in dup_pairs:
        flagged.update(members)
    groups = {}                                               # the end pass
    for members, _ in pairs:
        for i in members:
            groups.setdefault(entries[i][0], dict(paired=False, fragments=[]))["paired"] = True
    for (i,), score in fragments:
        groups.setdefault(entries[i][0], dict(paired=False, fragments=[]))["fragments"].append((i, score))
    dup_fragments = 0
    for group in groups.values():
        stays = None
        if not group["paired"]:
            for i, score in group["fragments"]:
                if stays is None or score > stays[1]:
                    stays = (i, score)
        for i, _ in group["fragments"]:
            if stays is None or i != stays[0]:
                flagged.add(i)
                dup_fragments += 1
    return flagged, dict(pair_units=len(pairs), fragment_units=len(fragments), duplicate_pair_units=len(dup_pairs),
                         duplicate_fragment_units=dup_fragments, records_flagged=len(flagged))


def entries_of(records, ends: int, quals=None, min_quality: int = 15, limits=None) -> tuple:
    """(mark's entries, the malformed records' count): a malformed record takes its whole unit out."""
    bad = [malformed(r, i, limits) for i, r in enumerate(records)]
    entries = []
    for i, r in enumerate(records):
        unit = range(i - i % ends, i - i % ends + ends)
        if any(bad[j] for j in unit) or r["strand"] < 0:
            entries.append(None)
        else:
            entries.append(((five_prime(r), r["strand"]), quality_sum(None if quals is None else quals[i], min_quality)))
    return entries, sum(bad)


def duplicates(records, ends: int, quals=None, min_quality: int = 15, limits=None) -> tuple:
    """(the set of flagged record indices, the stats dict) of a batch of record dicts and their QUAL strings (or None)."""
    entries, skipped = entries_of(records, ends, quals, min_quality, limits)
    flagged, stats = mark(entries, ends)
    return flagged, dict(stats, records_skipped=skipped)


def keys(records, ends: int, quals=None, min_quality: int = 15, limits=None) -> dict:
    """What the key kernel writes: end_key per record — (5' << 1 | strand) << 1 | tag, tag 1 for a fragment, INT64_MAX where the
    record is no entry —, and per unit the score and the pair key's halves (INT64_MAX where the unit is no pair unit)."""
    entries, _ = entries_of(records, ends, quals, min_quality, limits)
    half = [None if e is None else e[0][0] << 1 | e[0][1] for e in entries]
    out = dict(end_key=[], score=[], pair_key_a=[], pair_key_b=[])
    for u in range(len(records) // ends):
        members = [i for i in range(u * ends, (u + 1) * ends) if entries[i] is not None]
        paired = len(members) == 2
        for i in range(u * ends, (u + 1) * ends):
            out["end_key"].append(INT64_MAX if entries[i] is None else half[i] << 1 | (0 if paired else 1))
        out["score"].append(min(sum(entries[i][1] for i in members), INT32_MAX))
        both = sorted(half[i] for i in members) if paired else [INT64_MAX, INT64_MAX]
        out["pair_key_a"].append(both[0])
        out["pair_key_b"].append(both[1])
    return out


def cigar_reference_length(cigar: str) -> int:
    """The reference bases a CIGAR consumes: its =, X and D runs (and M, N for completeness)."""
    total, number = 0, ""
    for c in cigar:
        if c.isdigit():
            number += c
        else:
            total += int(number) if c in "=XDMN" else 0
            number = ""
    return total


def duplicates_of_sam(lines, paired: bool) -> tuple:
    """The same from SAM lines alone: FLAG (4: unmapped, 16: reverse), RNAME, POS, the reference length of the CIGAR, QUAL; the key
    is (RNAME, local 5', strand); the mate of line 2u is line 2u + 1."""
    entries = []
    for text in lines:
        f = text.rstrip(b"\n").split(b"\t")
        flag, begin = int(f[1]), int(f[3]) - 1
        if flag & 4:
            entries.append(None)
            continue
        strand, end = flag >> 4 & 1, begin + cigar_reference_length(f[5].decode())
        five = end - 1 if strand == 1 and end > begin else begin
        entries.append(((f[2], five, strand), quality_sum(None if f[10] == b"*" else f[10])))
    flagged, stats = mark(entries, 2 if paired else 1)
    return flagged, dict(stats, records_skipped=0)
