"""Host model of the BAM stage (include/bgsa_hip.h "BAM records"; SAMv1 §4.1, §4.2, §5.3), in plain Python with struct, zlib and
gzip: reg2bin, a record encoder from the record dicts of sam_reference.craft, a record decoder that prints a record as its SAM
line, the header both ways, a BGZF block walker that checks every byte of the framing itself, and a model of the sliced CRC the
framing kernel computes.  Neither samtools nor pysam is needed."""
import struct
import zlib

import sam_reference as S

SEQ_CODES = b"=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"
BAM_OP = {"I": 1, "D": 2, "=": 7, "X": 8}            # SAM letter -> BAM op
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
INT32 = range(-2 ** 31, 2 ** 31)


# ---- bins ---------------------------------------------------------------------------------------------------------------------------
def reg2bin(beg: int, end: int) -> int:
    """SAMv1 §5.3, for the half-open interval [beg, end)."""
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def smallest_bin(beg: int, end: int) -> int:
    """The definition reg2bin implements: the smallest bin of the UCSC scheme (one of 512 Mbp, 8 of 64 Mbp, 64 of 8 Mbp, 512 of 1 Mbp,
    4,096 of 128 kbp, 32,768 of 16 kbp, numbered level by level) that contains [beg, end)."""
    first, best = 0, 0
    for level in range(6):
        size = 2 ** (29 - 3 * level)
        for k in {beg // size, (end - 1) // size}:
            if k * size <= beg and end <= (k + 1) * size:
                best = first + k
        first += 8 ** level
    return best


# ---- records --------------------------------------------------------------------------------------------------------------------------
def seq_code(c: int) -> int:
    at = SEQ_CODES.find(bytes([c]).upper())
    return 15 if at < 0 else at


def pack_seq(seq: bytes) -> bytes:
    codes = [seq_code(c) for c in seq] + [0]
    return bytes(codes[2 * j] << 4 | codes[2 * j + 1] for j in range((len(seq) + 1) // 2))


def sam_seq(rec: dict) -> bytes:
    """SEQ as the SAM line prints it: the caller's bytes, a reverse hit reverse-complemented (anything but ACGT: N)."""
    return S.reverse_complement(rec["read"]) if rec["strand"] == 1 else rec["read"]


def encode(rec: dict, qual, reference: bytes, ref_id: int = 0, start: int = 0, mate=None) -> bytes:
    """The bytes of one record, block_size included.  rec: a dict of sam_reference.craft (or an unmapped one: strand -1) with name,
    flag, mapq, rnext, pnext, tlen.  One sequence: ref_id 0, start 0, pnext the mate's POS.  The contig form: rec's begin, end and
    pnext are LINEAR, ref_id / start are the index and linear start of the record's own contig (not used when it is unmapped),
    mate = (index, start) of the contig that holds pnext - 1."""
    mapped, named = rec["strand"] >= 0, rec["rnext"] == 1
    mate_id, mate_start = (0, 0) if mate is None else mate
    next_id, next_pos = (mate_id, rec["pnext"] - mate_start - 1) if named else (-1, rec["pnext"] - 1)
    if mapped:
        own_id, pos = ref_id, rec["begin"] - start
        end = pos + max(1, rec["end"] - rec["begin"])
    else:
        own_id, pos = (next_id, next_pos) if named else (-1, -1)
        end = pos + 1
    assert pos in INT32 and next_pos in INT32 and rec["tlen"] in INT32 and len(rec["name"]) <= 254
    bin_ = 4680 if pos < 0 else reg2bin(pos, end) & 0xffff
    seq = sam_seq(rec)
    if qual is not None and rec["strand"] == 1:
        qual = qual[::-1]
    cigar = [n << 4 | BAM_OP[op] for n, op in rec["runs"]] if mapped else []
    body = struct.pack("<iiBBHHHIiii", own_id, pos, len(rec["name"]) + 1, rec["mapq"] if mapped else 0, bin_, len(cigar), rec["flag"], len(seq),
                       next_id, next_pos, rec["tlen"])
    body += rec["name"] + b"\x00" + struct.pack(f"<{len(cigar)}I", *cigar) + pack_seq(seq)
    body += bytes([0xff]) * len(seq) if qual is None else bytes(q - 33 for q in qual)
    if mapped:
        body += b"NMi" + struct.pack("<i", rec["distance"]) + b"MDZ" + S.md_text(rec["runs"], reference, rec["begin"]).encode() + b"\x00"
    return struct.pack("<i", len(body)) + body


def split_records(payload: bytes) -> list:
    """The records of a payload, block_size included in each, by their block_size fields; nothing may be left over."""
    out, at = [], 0
    while at < len(payload):
        assert at + 4 <= len(payload), "a block_size field runs off the payload"
        size = struct.unpack_from("<i", payload, at)[0]
        assert size >= 32 and at + 4 + size <= len(payload), (at, size, len(payload))
        out.append(payload[at: at + 4 + size])
        at += 4 + size
    return out


def decode(record: bytes, ref_names) -> dict:
    """One record (block_size included) as a dict of its fields and `line`, its SAM line with '=' / 'X' ops, NM:i and MD:Z."""
    size, ref_id, pos, l_name, mapq, bin_, n_cigar, flag, l_seq, next_id, next_pos, tlen = struct.unpack_from("<iiiBBHHHIiii", record, 0)
    assert size == len(record) - 4
    at = 36
    name = record[at: at + l_name - 1]
    assert record[at + l_name - 1] == 0 and b"\x00" not in name and l_name >= 2
    at += l_name
    cigar = struct.unpack_from(f"<{n_cigar}I", record, at)
    at += 4 * n_cigar
    packed = record[at: at + (l_seq + 1) // 2]
    at += (l_seq + 1) // 2
    seq = bytes(SEQ_CODES[packed[j // 2] >> 4 if j % 2 == 0 else packed[j // 2] & 15] for j in range(l_seq))
    assert l_seq % 2 == 0 or packed[-1] & 15 == 0, "the odd last nibble is not 0"
    qual = record[at: at + l_seq]
    at += l_seq
    tags = {}
    while at < len(record):
        tag, kind = record[at: at + 2].decode(), chr(record[at + 2])
        at += 3
        if kind == "i":
            tags[tag] = struct.unpack_from("<i", record, at)[0]
            at += 4
        else:
            assert kind == "Z", kind
            stop = record.index(b"\x00", at)
            tags[tag] = record[at: stop].decode()
            at = stop + 1
    assert at == len(record)
    assert -1 <= ref_id < len(ref_names) and -1 <= next_id < len(ref_names)
    cigar_text = "".join(f"{w >> 4}{CIGAR_OPS[w & 15]}" for w in cigar) if n_cigar else "*"
    rnext = b"*" if next_id < 0 else b"=" if next_id == ref_id else ref_names[next_id]
    line = S.line(name, flag, b"*" if ref_id < 0 else ref_names[ref_id], pos + 1, mapq, cigar_text, rnext, next_pos + 1, tlen, seq,
                  None if all(q == 0xff for q in qual) else bytes(q + 33 for q in qual), tags.get("NM"), tags.get("MD"))
    assert list(tags) in ([], ["NM", "MD"])
    return dict(ref_id=ref_id, pos=pos, mapq=mapq, bin=bin_, flag=flag, next_ref_id=next_id, next_pos=next_pos, tlen=tlen, name=name, seq=seq,
                cigar=cigar, nm=tags.get("NM", -1), line=line)


# ---- the header -----------------------------------------------------------------------------------------------------------------------
def encode_header(text: bytes, references) -> bytes:
    out = b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(references))
    for name, n in references:
        out += struct.pack("<i", len(name) + 1) + name + b"\x00" + struct.pack("<i", n)
    return out


def decode_header(data: bytes) -> tuple:
    """(text, [(name, length)], the bytes the header takes) of an uncompressed BAM stream."""
    assert data[:4] == b"BAM\x01"
    l_text = struct.unpack_from("<i", data, 4)[0]
    text = data[8: 8 + l_text]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", data, at)[0]
    at += 4
    references = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", data, at)[0]
        name = data[at + 4: at + 4 + l_name]
        assert name.endswith(b"\x00")
        references.append((name[:-1], struct.unpack_from("<i", data, at + 4 + l_name)[0]))
        at += 8 + l_name
    return text, references, at


# ---- BGZF -----------------------------------------------------------------------------------------------------------------------------
def frame(data: bytes, block_payload: int) -> bytes:
    """The stored-block framing, block by block; no EOF block."""
    out = b""
    for at in range(0, len(data), block_payload):
        piece = data[at: at + block_payload]
        out += bytes.fromhex("1f8b08040000000000ff060042430200") + struct.pack("<H", len(piece) + 30)
        out += b"\x01" + struct.pack("<HH", len(piece), len(piece) ^ 0xffff) + piece + struct.pack("<II", zlib.crc32(piece), len(piece))
    return out


def walk_blocks(blocks: bytes, stored: bool = True) -> list:
    """The payload of every block of a BGZF stream, following BSIZE: every header byte, the CRC and ISIZE are checked here, the
    deflate data is inflated by zlib; stored: it must also be ONE stored block of exactly the payload."""
    out, at = [], 0
    while at < len(blocks):
        assert blocks[at: at + 12] == bytes.fromhex("1f8b08040000000000ff0600"), (at, blocks[at: at + 12].hex())
        assert blocks[at + 12: at + 16] == b"BC\x02\x00", at
        size = struct.unpack_from("<H", blocks, at + 16)[0] + 1
        assert at + size <= len(blocks), "BSIZE runs off the stream"
        deflate = blocks[at + 18: at + size - 8]
        piece = zlib.decompress(deflate, -15)
        crc, isize = struct.unpack_from("<II", blocks, at + size - 8)
        assert crc == zlib.crc32(piece) and isize == len(piece), (at, crc, isize)
        if stored and deflate != b"\x03\x00":
            assert deflate[:5] == b"\x01" + struct.pack("<HH", len(piece), len(piece) ^ 0xffff) and deflate[5:] == piece, at
        out.append(piece)
        at += size
    return out


# ---- the sliced CRC ---------------------------------------------------------------------------------------------------------------------
POLY = 0xedb88320
TABLE = []
for _n in range(256):
    _c = _n
    for _ in range(8):
        _c = (_c >> 1) ^ (POLY if _c & 1 else 0)
    TABLE.append(_c)


def gf_mul(a: int, b: int) -> int:
    """a * b in GF(2)[x] mod the CRC polynomial, both reflected (bit 31 is x^0)."""
    p = 0
    for _ in range(32):
        if a & 0x80000000:
            p ^= b
        a = (a << 1) & 0xffffffff
        b = (b >> 1) ^ (POLY if b & 1 else 0)
    return p


def x_pow_bytes(n: int) -> int:
    """x^(8n) mod the polynomial, by square-and-multiply on x^8."""
    result, power = 0x80000000, 0x00800000
    while n:
        if n & 1:
            result = gf_mul(result, power)
        power = gf_mul(power, power)
        n >>= 1
    return result


def sliced_crc(data: bytes, lanes: int = 256) -> int:
    """CRC-32 of data the way the framing kernel computes it: lane t folds the contiguous slice t of ceil(len / lanes) bytes into a
    state of its own (0, lane 0's ~0), multiplies it by x^(8 * bytes behind its slice), and the states are XORed."""
    n = len(data)
    slice_ = (n + lanes - 1) // lanes
    joined = 0
    for t in range(lanes):
        first = min(t * slice_, n)
        last = min(first + slice_, n)
        state = 0xffffffff if t == 0 else 0
        for byte in data[first:last]:
            state = TABLE[(state ^ byte) & 0xff] ^ (state >> 8)
        if state and last < n:
            state = gf_mul(state, x_pow_bytes(n - last))
        joined ^= state
    return joined ^ 0xffffffff
