"""Host model of the BGZF deflate stage (include/bgsa_hip.h "BAM records": deflate; RFC 1951 inside SAMv1 §4.1), in plain Python:
the match finder, the greedy parse, the length-limited Huffman codes, the bitstream and the choice between the dynamic and the
stored form, each as bgsa_amd/csrc/bgzf_deflate.hip computes it — the device output must equal deflate_blocks() byte for byte.
Also the payloads the tests share.  The model is NORMATIVE; what it fixes:
  tiles       positions are taken in tiles of TILE = 1,024 bytes, in order; a table of 2^15 entries holds, per hash of the 4 bytes
              at a position (little-endian word * 0x9E3779B1, top 15 bits), the greatest position of any EARLIER tile with it
  candidates  position i tries i - 1, and the table entry of its own hash if i + 4 <= LEN and the distance is <= 32,768; the length
              is by comparison, capped at 258 and at the block's end; the longer wins, a tie goes to distance 1; a match is used
              from length 4, or from length 3 at a distance below 4,096
  parse       greedy from position 0
  codes       Huffman lengths of the 286 + 30 symbol counts (EOB once) by Moffat and Katajainen's in-place method on the symbols
              sorted by (count, symbol), limited to 15 bits by miniz's rule (clamp, then repair the Kraft sum one step at a time),
              the shortest lengths handed to the greatest counts; canonical codes; a single used symbol gets length 1, no used
              distance symbol leaves all 30 lengths 0 (zlib accepts both)
  header      BFINAL 1, BTYPE 10, HLIT 286, HDIST 30, HCLEN 19; the code-length code is FIXED: symbols 0..15 at 4 bits, 16..18
              unused, so every one of the 316 lengths is its own 4-bit symbol: 17 + 57 + 1,264 = 1,338 bits
  choice      dynamic if and only if ceil(bits / 8) < LEN + 5, else stored."""
import functools
import struct
import zlib

import numpy as np

TILE = 1024
HASH_BITS = 15
WINDOW = 32768
MAX_MATCH = 258
HEADER_BITS = 17 + 19 * 3 + 316 * 4
CLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
BGZF_HEAD = bytes.fromhex("1f8b08040000000000ff060042430200")

# RFC 1951 §3.2.5, as tables: the model's symbol arithmetic is checked against them (test_bgzf_deflate_cpu.py)
LENGTH_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LENGTH_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


# ---- symbols: the arithmetic the kernel uses instead of tables --------------------------------------------------------------------------
def length_symbol(length: int) -> tuple:
    """(symbol, extra bits, extra value) of a match length 3..258."""
    l = length - 3
    if l < 8:
        return 257 + l, 0, 0
    if length == 258:
        return 285, 0, 0
    e = l.bit_length() - 3
    return 261 + 4 * e + ((l >> e) & 3), e, l & ((1 << e) - 1)


def dist_symbol(dist: int) -> tuple:
    """(symbol, extra bits, extra value) of a distance 1..32,768."""
    d = dist - 1
    if d < 4:
        return d, 0, 0
    hb = d.bit_length() - 1
    e = hb - 1
    return 2 * hb + ((d >> e) & 1), e, d & ((1 << e) - 1)


def litlen_extra(symbol: int) -> int:
    return 0 if symbol < 265 or symbol == 285 else (symbol - 261) >> 2


def dist_extra(symbol: int) -> int:
    return 0 if symbol < 4 else (symbol >> 1) - 1


# ---- the match finder and the parse -----------------------------------------------------------------------------------------------------
def hash4(data: bytes, p: int) -> int:
    return ((struct.unpack_from("<I", data, p)[0] * 0x9E3779B1) & 0xffffffff) >> (32 - HASH_BITS)


def match_length(data: bytes, a: int, b: int, cap: int) -> int:
    """How many bytes data[a:] and data[b:] share, cap at the most (a < b; the two may overlap)."""
    x, y = data[a: a + cap], data[b: b + cap]
    if x == y:
        return cap
    diff = int.from_bytes(x, "little") ^ int.from_bytes(y, "little")
    return ((diff & -diff).bit_length() - 1) >> 3


def find_matches(data: bytes) -> list:
    """[(length, distance)] per position of one block, (0, 0) where no match is used."""
    n = len(data)
    table = [0] * (1 << HASH_BITS)              # position + 1; 0: none
    out = [(0, 0)] * n
    for base in range(0, n, TILE):
        stop = min(base + TILE, n)
        hashes = [hash4(data, p) if p + 4 <= n else -1 for p in range(base, stop)]
        for p in range(base, stop):
            cap = min(MAX_MATCH, n - p)
            length, dist = 0, 0
            if p >= 1 and data[p - 1] == data[p]:
                length, dist = match_length(data, p - 1, p, cap), 1
            h = hashes[p - base]
            if h >= 0 and table[h] and p - (table[h] - 1) <= WINDOW:
                c = table[h] - 1
                if data[c] == data[p]:
                    far = match_length(data, c, p, cap)
                    if far > length:
                        length, dist = far, p - c
            if length >= 4 or (length == 3 and dist < 4096):
                out[p] = (length, dist)
        for p in range(base, stop):
            if hashes[p - base] >= 0:
                table[hashes[p - base]] = p + 1          # the greatest: p rises
    return out


def parse(data: bytes) -> list:
    """The greedy tokens of one block: (position, length, distance), length 0 for a literal."""
    matches, tokens, p = find_matches(data), [], 0
    while p < len(data):
        length, dist = matches[p]
        tokens.append((p, length, dist))
        p += length if length else 1
    return tokens


def histograms(data: bytes, tokens) -> tuple:
    litlen, dist = [0] * 286, [0] * 30
    for p, length, d in tokens:
        if length:
            litlen[length_symbol(length)[0]] += 1
            dist[dist_symbol(d)[0]] += 1
        else:
            litlen[data[p]] += 1
    litlen[256] = 1
    return litlen, dist


# ---- the codes --------------------------------------------------------------------------------------------------------------------------
def huffman_depths(keys: list) -> list:
    """Moffat and Katajainen's in-place minimum-redundancy lengths of ascending counts (n >= 2): element i's code length, unlimited."""
    a, n = list(keys), len(keys)
    a[0] += a[1]
    root, leaf = 0, 2
    for nxt in range(1, n - 1):
        if leaf >= n or a[root] < a[leaf]:
            a[nxt] = a[root]
            a[root] = nxt
            root += 1
        else:
            a[nxt] = a[leaf]
            leaf += 1
        if leaf >= n or (root < nxt and a[root] < a[leaf]):
            a[nxt] += a[root]
            a[root] = nxt
            root += 1
        else:
            a[nxt] += a[leaf]
            leaf += 1
    a[n - 2] = 0
    for nxt in range(n - 3, -1, -1):
        a[nxt] = a[a[nxt]] + 1
    avail, used, depth, root, nxt = 1, 0, 0, n - 2, n - 1
    while avail > 0:
        while root >= 0 and a[root] == depth:
            used += 1
            root -= 1
        while avail > used:
            a[nxt] = depth
            nxt -= 1
            avail -= 1
        avail, depth, used = 2 * used, depth + 1, 0
    return a


def code_lengths(counts: list, limit: int = 15) -> list:
    """The code length of every symbol (0: unused)."""
    order = sorted((c, s) for s, c in enumerate(counts) if c)
    lengths = [0] * len(counts)
    if not order:
        return lengths
    if len(order) == 1:
        lengths[order[0][1]] = 1
        return lengths
    depths = huffman_depths([c for c, _ in order])
    per = [0] * (max(max(depths), limit) + 1)
    for d in depths:
        per[d] += 1
    for d in range(limit + 1, len(per)):
        per[limit] += per[d]
    total = sum(per[d] << (limit - d) for d in range(1, limit + 1))
    while total != 1 << limit:
        per[limit] -= 1
        for d in range(limit - 1, 0, -1):
            if per[d]:
                per[d] -= 1
                per[d + 1] += 2
                break
        total -= 1
    at = len(order)
    for d in range(1, limit + 1):
        for _ in range(per[d]):
            at -= 1
            lengths[order[at][1]] = d
    return lengths


def canonical_codes(lengths: list) -> list:
    """RFC 1951 §3.2.2: the code of every symbol, most significant bit first."""
    per = [0] * 16
    for n in lengths:
        per[n] += 1
    per[0] = 0
    nxt, code = [0] * 16, 0
    for n in range(1, 16):
        code = (code + per[n - 1]) << 1
        nxt[n] = code
    out = [0] * len(lengths)
    for s, n in enumerate(lengths):
        if n:
            out[s] = nxt[n]
            nxt[n] += 1
    return out


# ---- the bitstream ----------------------------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.value, self.n = 0, 0

    def put(self, value: int, n: int):
        """n bits of value, least significant first."""
        self.value |= value << self.n
        self.n += n

    def code(self, code: int, n: int):
        """A Huffman code: most significant bit first."""
        self.put(int(format(code, f"0{n}b")[::-1], 2) if n else 0, n)

    def bytes(self) -> bytes:
        return self.value.to_bytes((self.n + 7) // 8, "little")


def dynamic_bits(litlen, dist, litlen_len, dist_len) -> int:
    """The exact length of the dynamic form in bits, from the counts and the code lengths alone."""
    return HEADER_BITS + sum(c * (litlen_len[s] + litlen_extra(s)) for s, c in enumerate(litlen)) + \
        sum(c * (dist_len[s] + dist_extra(s)) for s, c in enumerate(dist))


def dynamic_block(data: bytes, tokens=None) -> bytes:
    """The deflate data of one block in the dynamic form, whether or not it is the shorter one.  tokens: another parse of the same
    bytes than the model's (the tests code a block of literals alone with it)."""
    tokens = parse(data) if tokens is None else tokens
    litlen, dist = histograms(data, tokens)
    litlen_len, dist_len = code_lengths(litlen), code_lengths(dist)
    litlen_code, dist_code = canonical_codes(litlen_len), canonical_codes(dist_len)
    out = Bits()
    out.put(1, 1)
    out.put(2, 2)
    out.put(286 - 257, 5)
    out.put(30 - 1, 5)
    out.put(19 - 4, 4)
    for symbol in CLEN_ORDER:
        out.put(4 if symbol < 16 else 0, 3)
    for n in litlen_len + dist_len:
        out.code(n, 4)
    for p, length, d in tokens:
        if length:
            symbol, extra, value = length_symbol(length)
            out.code(litlen_code[symbol], litlen_len[symbol])
            out.put(value, extra)
            symbol, extra, value = dist_symbol(d)
            out.code(dist_code[symbol], dist_len[symbol])
            out.put(value, extra)
        else:
            out.code(litlen_code[data[p]], litlen_len[data[p]])
    out.code(litlen_code[256], litlen_len[256])
    assert out.n == dynamic_bits(litlen, dist, litlen_len, dist_len)
    return out.bytes()


@functools.lru_cache(maxsize=4096)
def _dynamic_once(data: bytes) -> bytes:
    return dynamic_block(data)


def stored_block(data: bytes) -> bytes:
    return b"\x01" + struct.pack("<HH", len(data), len(data) ^ 0xffff) + data


def deflate_block(data: bytes) -> bytes:
    """The deflate data of one block: dynamic if and only if that is strictly shorter than stored.  A block of up to 163 bytes is
    stored without a look: the dynamic header alone, one literal and EOB take 168 bytes."""
    if len(data) + 5 <= (HEADER_BITS + 2 + 7) // 8:
        return stored_block(data)
    dynamic = _dynamic_once(data)
    return dynamic if len(dynamic) < len(data) + 5 else stored_block(data)


def bgzf_block(data: bytes) -> bytes:
    deflate = deflate_block(data)
    return BGZF_HEAD + struct.pack("<H", len(deflate) + 25) + deflate + struct.pack("<II", zlib.crc32(data), len(data))


def deflate_blocks(payload: bytes, block_payload: int) -> list:
    """The BGZF blocks of a payload, one bytes object per block; no EOF block."""
    return [bgzf_block(payload[at: at + block_payload]) for at in range(0, len(payload), block_payload)]


def is_dynamic(block: bytes) -> bool:
    return block[18] & 7 == 5


# ---- payloads ---------------------------------------------------------------------------------------------------------------------------
def de_bruijn(k: int, n: int) -> bytes:
    """B(k, n) over the byte values 0..k-1: every n-gram exactly once, cyclically (the standard Lyndon-word construction)."""
    a, out = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                out.extend(a[1: p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return bytes(out)


def random_bytes(seed: int, n: int, values: int = 256) -> bytes:
    return np.random.default_rng(seed).integers(0, values, n, dtype=np.uint8).tobytes()


def planted(seed: int, n: int, source: int, dest: int, length: int) -> bytes:
    """n random bytes of 64 values (6 bits each: the block comes out dynamic) with bytes [source, source + length) repeated at dest."""
    data = bytearray(random_bytes(seed, n, 64))
    data[dest: dest + length] = data[source: source + length]
    return bytes(data)


def fibonacci_literals(seed: int = 7) -> bytes:
    """Literal counts 1, 1, 2, 3, 5, ... over 20 byte values (17,710 bytes), shuffled.  An unlimited Huffman code of these counts is
    19 deep.  No order of these bytes keeps the match finder quiet — the three most frequent values hold 13,530 of the bytes, the
    other 4,180 can break them into runs of three at 12,540 at the most, and 4-grams of three values number 81 — so the parse
    takes matches out of the frequent counts; the tests code this block as literals alone, and deep_literals() is the payload
    whose code is too deep under the model's own parse."""
    counts, a, b = [], 1, 1
    for _ in range(20):
        counts.append(a)
        a, b = b, a + b
    data = np.repeat(np.arange(20, dtype=np.uint8) + 65, counts)
    np.random.default_rng(seed).shuffle(data)
    return data.tobytes()


def deep_literals(seed: int = 5) -> bytes:
    """13,979 bytes of 30 values with counts 1, 2, 3, 5, ..., 1,597 (16 values) and 700 (14 values), drawn so that no 4-gram occurs
    twice and no byte four times in a row: the parse finds no match, the counts stay as they are, and with EOB's 1 an unlimited
    Huffman code of them is 17 deep."""
    counts = [1, 2]
    while len(counts) < 16:
        counts.append(counts[-1] + counts[-2])
    left = np.array(counts + [700] * 14, dtype=np.int64)
    rng = np.random.default_rng(seed)
    seen, out = set(), []
    for _ in range(int(left.sum())):
        order = rng.permutation(left.size)
        for s in order[np.argsort(-(left[order] * rng.random(left.size)), kind="stable")]:
            gram = tuple(out[-3:]) + (int(s),)
            if left[s] and not (len(gram) == 4 and (gram in seen or len(set(gram)) == 1)):
                seen.add(gram)
                out.append(int(s))
                left[s] -= 1
                break
        else:
            raise AssertionError("deep_literals: no value fits; try another seed")
    return bytes(65 + s for s in out)


def bam_like(regime: str, n_bytes: int, seed: int = 11) -> bytes:
    """n_bytes of BAM records of 150 bp reads (bam_reference.encode): random SEQ, sequential names, QUAL constant ('constant'), four
    binned values in runs ('binned') or uniform over 2..41 ('uniform')."""
    import bam_reference as M

    rng = np.random.default_rng(seed)
    reference = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 4096))
    out, i = b"", 0
    while len(out) < n_bytes:
        begin = int(rng.integers(0, len(reference) - 150))
        read = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 150))
        if regime == "constant":
            qual = np.full(150, 37)
        elif regime == "binned":
            qual = np.repeat(rng.choice(np.array([2, 12, 23, 37]), 30), rng.integers(1, 11, 30))[:150]
            qual = np.concatenate([qual, np.full(150 - qual.size, 37)])
        else:
            assert regime == "uniform", regime
            qual = rng.integers(2, 42, 150)
        rec = dict(name=f"read{i:07d}".encode(), flag=16 * (i % 2), mapq=60, rnext=0, pnext=0, tlen=0, read=read, strand=i % 2, begin=begin,
                   end=begin + 150, distance=0, runs=[(150, "=")])
        out += M.encode(rec, bytes((qual + 33).astype(np.uint8)), reference)
        i += 1
    return out[:n_bytes]


FULL = 0xff00


@functools.lru_cache(maxsize=None)
def payloads() -> dict:
    """name -> bytes: the smallest payloads at which each path of the compressor can go wrong."""
    out = {f"same{n}": b"\x07" * n for n in (1, 2, 3, 4)}
    out["zeros"] = bytes(FULL)
    out["random"] = random_bytes(1, 4096)
    out["debruijn"] = de_bruijn(16, 3)
    # a repeat of 64 bytes at distance exactly 32,768 (used) and one at 32,769 (out of the window: literals)
    out["dist32768"] = planted(3, 40000, 100, 100 + 32768, 64)
    out["dist32769"] = planted(3, 40000, 100, 100 + 32769, 64)
    # matches of 2, 3, 258 and 259 bytes available, two tiles back; the last is taken as 258 and a rest
    for n in (2, 3, 258, 259):
        data = bytearray(random_bytes(4, 4096, 64))
        data[3000: 3000 + n] = data[500: 500 + n]
        data[3000 + n] = data[500 + n] ^ 0x15
        out[f"avail{n}"] = bytes(data)
    out["ends_on_last"] = planted(5, 3000, 200, 3000 - 40, 40)
    # equal text on both sides of a boundary at 4,096 (and at every other P of the tests): no match across it
    out["boundary"] = random_bytes(6, 4096, 64) * 2
    out["same_tile"] = planted(8, 2048, 1030, 1500, 32)          # source and repeat inside tile 1: not found (the table holds earlier tiles)
    out["previous_tile"] = planted(8, 2048, 900, 1500, 32)       # the source lies in tile 0
    out["deep_code"] = deep_literals()                           # the literal/length code is limited to 15 bits
    for regime in ("constant", "binned", "uniform"):
        out[f"bam_{regime}"] = bam_like(regime, FULL + 61)
    return out


BLOCK_PAYLOADS = (1, 61, 256, 4096, FULL)


@functools.lru_cache(maxsize=None)
def modelled(name: str, block_payload: int) -> tuple:
    """The model's blocks of payloads()[name], computed once per session and shared."""
    return tuple(deflate_blocks(payloads()[name], block_payload))
