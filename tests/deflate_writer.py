"""A raw DEFLATE (RFC 1951) writer for tests: stored, fixed and dynamic blocks from a list of tokens, with every choice a
compressor makes left to the caller -- code lengths, HLIT / HDIST / HCLEN, the run-length coding of the code lengths -- so that
a test can aim a stream at one edge of a decoder.  A token is a literal byte (int 0..255) or a (length, distance) pair.
Standard library only.  zlib is the judge: write() decodes every stream it makes with zlib and refuses one that does not give
back exactly the intended text.

Then the named corpus the decoder tests share (corpus()): each item aims at one edge of the device decoder
(mitoflex_amd/csrc/mf_gzdev.hip) -- full-window matches across a chunk's start, overlapping copies around the round and staging
sizes, 15-bit codes, the two-literal table entry, small alphabets, empty and maximal blocks, fixed blocks' top codes -- next to
zlib streams of every strategy, memLevel and window size."""
import ctypes
import ctypes.util
import random
import zlib

# ---- the code tables of RFC 1951 3.2.5
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30


def len_code(length):
    """(symbol 257..285, extra value, extra bits) of a match length 3..258; 258 is code 285, not 284 + 31"""
    assert 3 <= length <= 258
    if length == 258:
        return 285, 0, 0
    i = max(j for j in range(28) if LEN_BASE[j] <= length)
    return 257 + i, length - LEN_BASE[i], LEN_EXTRA[i]


def dist_code(dist):
    assert 1 <= dist <= 32768
    i = max(j for j in range(30) if DIST_BASE[j] <= dist)
    return i, dist - DIST_BASE[i], DIST_EXTRA[i]


def canonical(lens):
    """RFC 1951 3.2.2: the code of every symbol from the code lengths"""
    bl = [0] * 16
    for n in lens:
        bl[n] += 1
    bl[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    codes = [0] * len(lens)
    for s, n in enumerate(lens):
        if n:
            codes[s] = nxt[n]
            nxt[n] += 1
    return codes


def kraft(lens):
    """sum of 2^-len over the used symbols, as a multiple of 2^-15 (32768 = complete)"""
    return sum(1 << (15 - n) for n in lens if n)


def limited_lengths(freqs, limit=15):
    """Optimal code lengths of at most `limit` bits (package-merge).  A single used symbol gets length 1."""
    used = sorted((f, s) for s, f in enumerate(freqs) if f > 0)
    lens = [0] * len(freqs)
    if not used:
        return lens
    if len(used) == 1:
        lens[used[0][1]] = 1
        return lens
    assert len(used) <= 1 << limit
    leaves = [(f, (s,)) for f, s in used]
    cur = list(leaves)
    for _ in range(limit - 1):
        pk = [(cur[i][0] + cur[i + 1][0], cur[i][1] + cur[i + 1][1]) for i in range(0, len(cur) - 1, 2)]
        cur = sorted(leaves + pk, key=lambda x: x[0])
    for _, syms in cur[:2 * len(used) - 2]:
        for s in syms:
            lens[s] += 1
    return lens


class Bits:
    """LSB-first bit writer"""
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, n):
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def huff(self, code, n):
        self.put(int(format(code, "0%db" % n)[::-1], 2) if n else 0, n)

    def align(self):
        if self.n & 7:
            self.put(0, 8 - (self.n & 7))

    def bit(self):
        return len(self.out) * 8 + self.n

    def done(self):
        self.align()
        return bytes(self.out)


class Block:
    """One block.  kind: 'stored' (tokens: literals only, at most 65 535), 'fixed' or 'dynamic'.  For dynamic blocks: lit_lens /
    dist_lens (lists of 286 / 30 code lengths, or shorter) or None for length-limited optimal ones from the tokens; hlit / hdist /
    hclen: how many code lengths the header sends (None: as few as the codes need, with the minimums 257 / 1 / 4); rle: code runs of
    code lengths with the precode symbols 16 (3..6 repeats), 17 (3..10 zeros), 18 (11..138 zeros), each run as long as it can be."""
    def __init__(self, kind, tokens, final=False, lit_lens=None, dist_lens=None, hlit=None, hdist=None, hclen=None, rle=True):
        self.kind, self.tokens, self.final = kind, list(tokens), final
        self.lit_lens, self.dist_lens, self.hlit, self.hdist, self.hclen, self.rle = lit_lens, dist_lens, hlit, hdist, hclen, rle


def rle_code_lengths(seq, rle=True):
    """the code lengths as precode symbols: (symbol, extra value, extra bits)"""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, run = seq[i], 1
        while i + run < n and seq[i + run] == v:
            run += 1
        if rle and v == 0 and run >= 3:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k - 11, 7)); i += k; run -= k
            if run >= 3:
                out.append((17, run - 3, 3)); i += run; run = 0
        elif rle and v != 0 and run >= 4:
            out.append((v, 0, 0)); i += 1; run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k - 3, 2)); i += k; run -= k
        while run > 0:
            out.append((v, 0, 0)); i += 1; run -= 1
    return out


def _tokens_symbols(tokens):
    lit, dist = [0] * 286, [0] * 30
    for t in tokens:
        if isinstance(t, int):
            lit[t] += 1
        else:
            lit[len_code(t[0])[0]] += 1
            dist[dist_code(t[1])[0]] += 1
    lit[256] += 1
    return lit, dist


def _write_dynamic_header(bw, b, tokens):
    lf, df = _tokens_symbols(tokens)
    ll = list(b.lit_lens) if b.lit_lens is not None else limited_lengths(lf)
    dl = list(b.dist_lens) if b.dist_lens is not None else limited_lengths(df)
    ll += [0] * (286 - len(ll))
    dl += [0] * (30 - len(dl))
    for s in range(286):
        assert not lf[s] or ll[s], "symbol %d used without a code" % s
    for s in range(30):
        assert not df[s] or dl[s], "distance code %d used without a code" % s
    hlit = b.hlit or max(257, max(s for s in range(286) if ll[s]) + 1)
    hdist = b.hdist or max(1, max([s + 1 for s in range(30) if dl[s]] or [1]))
    assert 257 <= hlit <= 286 and 1 <= hdist <= 30 and not any(ll[hlit:]) and not any(dl[hdist:])
    seq = rle_code_lengths(ll[:hlit] + dl[:hdist], b.rle)
    cf = [0] * 19
    for s, _, _ in seq:
        cf[s] += 1
    cl = limited_lengths(cf, 7)
    if sum(1 for n in cl if n) == 1:                # one precode symbol: a code of one length-1 entry is incomplete, which zlib refuses
        cl[16 if cl[0] else 0] = 1
    hclen = b.hclen or max(4, max(i for i in range(19) if cl[CL_ORDER[i]]) + 1)
    assert 4 <= hclen <= 19 and not any(cl[CL_ORDER[i]] for i in range(hclen, 19))
    bw.put(hlit - 257, 5); bw.put(hdist - 1, 5); bw.put(hclen - 4, 4)
    for i in range(hclen):
        bw.put(cl[CL_ORDER[i]], 3)
    cc = canonical(cl)
    for s, v, n in seq:
        bw.huff(cc[s], cl[s])
        bw.put(v, n)
    return ll, dl


def deflate(blocks):
    """raw DEFLATE of the blocks -> (bytes, text, boundaries): boundaries[i] = (bit of block i's header, text offset there, final)"""
    bw, text, bounds = Bits(), bytearray(), []
    for k, b in enumerate(blocks):
        assert b.final == (k == len(blocks) - 1), "exactly the last block is final"
        bounds.append((bw.bit(), len(text), b.final))
        bw.put(1 if b.final else 0, 1)
        if b.kind == "stored":
            data = bytes(b.tokens)
            assert len(data) <= 65535
            bw.put(0, 2); bw.align()
            bw.put(len(data), 16); bw.put(len(data) ^ 0xFFFF, 16)
            for x in data:
                bw.put(x, 8)
            text += data
            continue
        if b.kind == "fixed":
            bw.put(1, 2)
            ll, dl = FIXED_LIT, FIXED_DIST
        else:
            bw.put(2, 2)
            ll, dl = _write_dynamic_header(bw, b, b.tokens)
        lc, dc = canonical(ll), canonical(dl)
        for t in b.tokens:
            if isinstance(t, int):
                bw.huff(lc[t], ll[t])
                text.append(t)
            else:
                length, dist = t
                assert 1 <= dist <= min(len(text), 32768), "distance %d with %d bytes of text" % (dist, len(text))
                s, v, n = len_code(length)
                bw.huff(lc[s], ll[s]); bw.put(v, n)
                s, v, n = dist_code(dist)
                bw.huff(dc[s], dl[s]); bw.put(v, n)
                start = len(text) - dist
                if dist >= length:
                    text += text[start:start + length]
                else:
                    for i in range(length):
                        text.append(text[start + i])
        bw.huff(lc[256], ll[256])
    return bw.done(), bytes(text), bounds


def gzip_wrap(raw, text):
    """a plain 10-byte gzip header (no name, no extra field), the deflate data, CRC-32 and ISIZE"""
    return b"\x1f\x8b\x08\0\0\0\0\0\x00\x03" + raw + zlib.crc32(text).to_bytes(4, "little") + (len(text) & 0xFFFFFFFF).to_bytes(4, "little")


class _ZStream(ctypes.Structure):
    _fields_ = [("next_in", ctypes.c_void_p), ("avail_in", ctypes.c_uint), ("total_in", ctypes.c_ulong),
                ("next_out", ctypes.c_void_p), ("avail_out", ctypes.c_uint), ("total_out", ctypes.c_ulong),
                ("msg", ctypes.c_char_p), ("state", ctypes.c_void_p), ("zalloc", ctypes.c_void_p), ("zfree", ctypes.c_void_p),
                ("opaque", ctypes.c_void_p), ("data_type", ctypes.c_int), ("adler", ctypes.c_ulong), ("reserved", ctypes.c_ulong)]


def zlib_boundaries(raw):
    """The block boundaries zlib itself sees in a raw deflate stream: inflate() in Z_BLOCK mode (which Python's zlib module does not
    offer; the C library through ctypes) stops in front of every block and says how many bits of the last byte it has not used.
    -> ([(bit, text offset)] of every block's header, bit behind the final block, text)"""
    lib = ctypes.CDLL(ctypes.util.find_library("z") or "libz.so.1")
    zs = _ZStream()
    ver = lib.zlibVersion
    ver.restype = ctypes.c_char_p
    assert lib.inflateInit2_(ctypes.byref(zs), -15, ver(), ctypes.sizeof(zs)) == 0
    src = ctypes.create_string_buffer(bytes(raw), len(raw))
    obuf = ctypes.create_string_buffer(1 << 16)
    base = ctypes.addressof(src)
    zs.next_in, zs.avail_in = base, len(raw)
    bounds, text, end = [(0, 0)], bytearray(), None
    try:
        while True:
            zs.next_out, zs.avail_out = ctypes.addressof(obuf), len(obuf)
            rc = lib.inflate(ctypes.byref(zs), 5)                   # Z_BLOCK
            text += obuf.raw[:len(obuf) - zs.avail_out]
            assert rc in (0, 1), "zlib: %d" % rc
            bit = (zs.next_in - base) * 8 - (zs.data_type & 7)
            if rc == 1:
                end = bit
                break
            if zs.data_type & 128 and not zs.data_type & 64 and bounds[-1][0] != bit:
                bounds.append((bit, len(text)))
    finally:
        lib.inflateEnd(ctypes.byref(zs))
    return bounds, end, bytes(text)


def write(blocks):
    """-> (gzip member, text, boundaries in bits of the member) -- decoded by zlib, which must give back exactly the text"""
    raw, text, bounds = deflate(blocks)
    d = zlib.decompressobj(-15)
    got = d.decompress(raw) + d.flush()
    assert got == text and d.eof and not d.unused_data, "zlib does not decode the stream to its text"
    return gzip_wrap(raw, text), text, [(bit + 80, off, fin) for bit, off, fin in bounds]


def zlib_member(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, wbits=15):
    c = zlib.compressobj(level, zlib.DEFLATED, -wbits, mem_level, strategy)
    return gzip_wrap(c.compress(text) + c.flush(), text)


# ---------------------------------------------------------------------------------------------------------------- the corpus
def fastq_like(rng, n):
    out = []
    for i in range(n):
        L = rng.choice([150, 150, 151, 100])
        out.append("@SRR000.%d %d/1\n%s\n+\n%s\n" % (i, i, "".join(rng.choices("ACGTN", weights=[30, 20, 20, 30, 1], k=L)),
                                                  "".join(rng.choices("FFFFF:,#", k=L))))
    return "".join(out).encode()


def blocks_of(tokens, rng, lo, hi, kind="dynamic", **kw):
    """cut a token list into non-final blocks of lo..hi tokens"""
    out, i = [], 0
    while i < len(tokens):
        n = rng.randint(lo, hi)
        out.append(Block(kind, tokens[i:i + n], **kw))
        i += n
    return out


def finish(blocks):
    """the last block becomes the final one; -> write()'s (member, text, boundaries)"""
    blocks[-1].final = True
    return write(blocks)


def match_length(rng, sym):
    """a random length coded by length symbol sym"""
    i = sym - 257
    return 258 if sym == 285 else LEN_BASE[i] + rng.randrange(1 << LEN_EXTRA[i])


def chain_lengths(symbols):
    """code lengths 1, 2, .., 14, 15, 15 for 16 symbols (a complete code whose two last codes are 15 bits long)"""
    assert len(symbols) == 16
    return {s: min(i + 1, 15) for i, s in enumerate(symbols)}


def lens_from(d, n):
    v = [0] * n
    for s, L in d.items():
        v[s] = L
    return v


def full_window(period, seed, n_match=4000):
    """text with the given period, every repeat coded as matches at exactly that distance (and a literal now and then), with a
    non-final dynamic block every 100..250 tokens: a chunk that starts at one of them begins with a match that reaches back
    `period` bytes, i.e. with markers of index 32768 - period and up"""
    rng = random.Random(seed)
    toks = [rng.randrange(256) for _ in range(period)]
    blocks = blocks_of(toks, rng, 200, 400)
    m = []
    for _ in range(n_match):
        m.append((rng.choice([258, 258, 258, 3, 4, 100, 257, rng.randint(3, 258)]), period))
        if rng.random() < 0.05:
            m.append(rng.randrange(256))
    return finish(blocks + blocks_of(m, rng, 100, 250))


def overlapping(seed):
    """runs of overlapping copies (distance 1..8, lengths 258 = code 285 and 257 = code 284 + 30): 63, 64 and 65 tokens in a
    row (a round of the serial kernel lists 64), and groups of 1 023 / 1 024 / 1 025 symbols (its staging buffer holds 1 024);
    every block begins with such a run, so that a chunk starting there copies from its markers"""
    rng = random.Random(seed)
    blocks = [Block("dynamic", [rng.randrange(256) for _ in range(3000)])]
    for r in range(36):
        d = 1 + r % 8
        k = (63, 64, 65)[r % 3]
        toks = [(258 if j % 2 == 0 else 257, d) for j in range(k)]
        for extra in (1023, 1024, 1025):
            toks += [(258, d), (258, d), (258, d), (extra - 774, d)] + [rng.randrange(256) for _ in range(rng.randint(0, 3))]
        toks += [rng.randrange(256) for _ in range(rng.randint(1, 40))]
        blocks.append(Block("dynamic", toks))
    return finish(blocks)


def long_codes(seed, which):
    """a dynamic block whose literal/length code ('lit') or distance code ('dist') reaches 15 bits, every code used"""
    rng = random.Random(seed)
    blocks = [Block("dynamic", [rng.randrange(256) for _ in range(2000)])]
    if which == "lit":
        syms = [65, 67, 71, 84, 10, 64, 43, 70, 257, 256, 258, 265, 73, 58, 272, 285]
        ll, dl = lens_from(chain_lengths(syms), 286), None
        use = syms
    else:
        ll, dl = None, lens_from(chain_lengths(list(range(16))), 30)
        use = [65, 67, 71, 84, 257, 262, 270]
    for _ in range(12):
        toks = []
        for j in range(2500):
            s = use[j % len(use)] if j < 2 * len(use) else rng.choice(use)
            if s == 256:
                continue
            if s < 256:
                toks.append(s)
            else:
                dc = j % 16 if which == "dist" else rng.randrange(14)
                toks.append((match_length(rng, s), min(2000, DIST_BASE[dc] + rng.randrange(1 << DIST_EXTRA[dc]))))
        blocks.append(Block("dynamic", toks, lit_lens=ll, dist_lens=dl))
    return finish(blocks)


def literal_pairs(seed):
    """literal codes of 3..8 bits (pairs that fill exactly 10 and 11 bits of the first-level table) and short literals in front of
    length codes"""
    rng = random.Random(seed)
    lits = [65, 67] + [71, 84, 10, 64] + [43, 70, 73, 58] + list(range(97, 105)) + list(range(105, 121)) + list(range(128, 156))
    lens = {}
    for s, L in zip(lits, [3] * 2 + [4] * 4 + [5] * 4 + [6] * 8 + [7] * 16 + [8] * 28):
        lens[s] = L
    for s in (256, 257, 258, 265):
        lens[s] = 8
    assert kraft(lens_from(lens, 286)) == 32768
    blocks = [Block("dynamic", [rng.choice(lits) for _ in range(300)])]
    for _ in range(20):
        toks = []
        for _ in range(1500):
            x = rng.random()
            toks.append(rng.choice(lits) if x < 0.8 else (rng.choice([3, 4, 11, 12]), rng.randint(1, 200)))
        blocks.append(Block("dynamic", toks, lit_lens=lens_from(lens, 286)))
    return finish(blocks)


def small_alphabets(seed):
    """literal-only blocks with one distance code of length 1, with no distance code at all, and blocks of nothing but end-of-block
    and one literal"""
    rng = random.Random(seed)
    blocks = []
    for r in range(30):
        toks = [rng.choice(b"ACGT") for _ in range(rng.randint(50, 2000))]
        if r % 3 == 0:
            blocks.append(Block("dynamic", toks, dist_lens=[1]))
        elif r % 3 == 1:
            blocks.append(Block("dynamic", toks, dist_lens=[0], hdist=1))
        else:
            blocks.append(Block("dynamic", [78] * rng.randint(1, 3000), lit_lens=lens_from({78: 1, 256: 1}, 286), dist_lens=[0]))
    return finish(blocks)


def empty_and_stored(seed):
    """empty dynamic and fixed blocks, stored blocks of LEN 0 and 65 535, stored blocks over chunk edges, a stored final block"""
    rng = random.Random(seed)
    rnd = lambda n: [rng.randrange(256) for _ in range(n)]
    blocks = [Block("dynamic", rnd(500)), Block("dynamic", [], lit_lens=lens_from({256: 1}, 286), dist_lens=[0]),
              Block("fixed", []), Block("stored", []), Block("stored", rnd(65535)), Block("dynamic", rnd(3000) + [(258, 1)] * 10),
              Block("dynamic", [], ), Block("stored", rnd(5000)), Block("fixed", rnd(100) + [(50, 3000)]), Block("stored", []),
              Block("stored", rnd(65535)), Block("dynamic", rnd(4000)), Block("stored", rnd(9000))]
    return finish(blocks)


def tiny_blocks(seed):
    """hundreds of blocks of a few bits or bytes each, of all three kinds, between ordinary dynamic blocks"""
    rng = random.Random(seed)
    blocks = []
    for r in range(12):
        blocks.append(Block("dynamic", [rng.choice(b"ACGTN\n") for _ in range(3000)]))
        for _ in range(60):
            k = rng.randrange(3)
            toks = [rng.choice(b"ACGT") for _ in range(rng.randint(0, 3))]
            blocks.append(Block(("fixed", "dynamic", "stored")[k], toks if k == 2 or not toks else toks + [(3, 1)]))
    return finish(blocks)


def fixed_top_codes(seed):
    """fixed blocks with length codes 280..285 (lengths 115..258) and distance code 29 (24 577..32 768)"""
    rng = random.Random(seed)
    blocks = blocks_of([rng.randrange(256) for _ in range(33000)], rng, 3000, 6000, "fixed")
    m = []
    for _ in range(3000):
        m.append((rng.choice([115, 130, 131, 162, 163, 194, 195, 226, 227, 257, 258, rng.randint(115, 258)]), rng.randint(24577, 32768)))
        if rng.random() < 0.1:
            m.append(rng.randrange(256))
    return finish(blocks + blocks_of(m, rng, 50, 200, "fixed"))


def header_extremes(seed):
    """HLIT 286, HDIST 30, HCLEN 19; the code lengths coded with the longest runs (18 x 138 zeros, 17 x 10 zeros, 16 x 6 repeats)
    and, in every other block, with no runs at all"""
    rng = random.Random(seed)
    lens = {}
    for s in range(138, 146):
        lens[s] = 4
    for s in range(156, 160):
        lens[s] = 5
    lens[256] = 3
    for s in range(257, 261):
        lens[s] = 5
    for s in range(265, 273):
        lens[s] = 6
    ll = lens_from(lens, 286)
    dl = [3] * 6 + [4] * 4 + [0] * 20
    assert kraft(ll) == 32768 and kraft(dl) == 32768
    lits = [s for s in lens if s < 256]
    blocks = [Block("dynamic", [rng.choice(lits) for _ in range(500)])]
    for r in range(16):
        toks = []
        for _ in range(2000):
            s = rng.choice(lits + [257, 258, 259, 260, 265, 272])
            toks.append(s if s < 256 else (match_length(rng, s), rng.randint(1, 12)))
        blocks.append(Block("dynamic", toks, lit_lens=ll, dist_lens=dl, hlit=286 if r % 4 else None, hdist=30 if r % 4 else None,
                            hclen=19 if r % 4 else None, rle=r % 2 == 0))
    return finish(blocks)


ZLIB_VARIANTS = {       # name: (level, strategy, memLevel, window bits)
    "zlib_filtered": (6, zlib.Z_FILTERED, 8, 15), "zlib_huffman_only": (6, zlib.Z_HUFFMAN_ONLY, 8, 15),
    "zlib_rle": (6, zlib.Z_RLE, 8, 15), "zlib_fixed": (6, zlib.Z_FIXED, 8, 15),
    "zlib_mem1": (6, zlib.Z_DEFAULT_STRATEGY, 1, 15), "zlib_mem9": (6, zlib.Z_DEFAULT_STRATEGY, 9, 15),
    "zlib_wbits9": (6, zlib.Z_DEFAULT_STRATEGY, 8, 9), "zlib_wbits12": (6, zlib.Z_DEFAULT_STRATEGY, 8, 12),
    "zlib_level1": (1, zlib.Z_DEFAULT_STRATEGY, 8, 15), "zlib_level9": (9, zlib.Z_DEFAULT_STRATEGY, 8, 15),
    "zlib_level9_mem1": (9, zlib.Z_DEFAULT_STRATEGY, 1, 15),
}

# name: (maker, what the item is there for: 'far' = markers of index < 262, 'spec' = chunks behind the first start at a true
# boundary and are verified there (dynamic blocks at every chunk's range))
WRITER_ITEMS = {
    "full_window_32768": (lambda: full_window(32768, 1), {"far", "spec"}),
    "full_window_32767": (lambda: full_window(32767, 2), {"far", "spec"}),
    "full_window_32600": (lambda: full_window(32600, 3), {"far", "spec"}),
    "full_window_32507": (lambda: full_window(32507, 4), {"far", "spec"}),
    "overlapping_copies": (lambda: overlapping(5), {"spec"}),
    "long_lit_codes": (lambda: long_codes(6, "lit"), {"spec"}),
    "long_dist_codes": (lambda: long_codes(7, "dist"), {"spec"}),
    "literal_pairs": (lambda: literal_pairs(8), {"spec"}),
    "small_alphabets": (lambda: small_alphabets(9), set()),
    "empty_and_stored": (lambda: empty_and_stored(10), set()),
    "tiny_blocks": (lambda: tiny_blocks(11), set()),
    "fixed_top_codes": (lambda: fixed_top_codes(12), set()),
    "header_extremes": (lambda: header_extremes(13), {"spec"}),
}

_CACHE = {}


def corpus():
    """name -> (gzip member, text, writer's boundaries or None for zlib's streams, tags); built once per process"""
    if not _CACHE:
        for name, (make, tags) in WRITER_ITEMS.items():
            gz, text, bounds = make()
            _CACHE[name] = (gz, text, bounds, tags)
        text = fastq_like(random.Random(20), 1500)
        for name, (level, strategy, mem, wbits) in ZLIB_VARIANTS.items():
            tags = {"spec"} if strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE) else set()
            _CACHE[name] = (zlib_member(text, level, strategy, mem, wbits), text, None, tags)
    return _CACHE


def fastq_full_window(records, repeats, seed=0):
    """a FASTQ file made of one block of records padded to exactly 32 768 bytes (a comment line of the last record takes up the
    slack), repeated: the first copy as literals, every later one as distance-32 768 matches, a dynamic block every 150 tokens"""
    assert len(records) < 32768 - 64
    pad = 32768 - len(records)
    unit = records + b"@pad " + b"x" * (pad - 12) + b"\nA\n+\nF\n"
    assert len(unit) == 32768
    rng = random.Random(seed)
    toks = list(unit)
    n, r = divmod((repeats - 1) * 32768, 258)
    m = [(258, 32768)] * n + ([(r, 32768)] if r >= 3 else [(258 + r - 3, 32768), (3, 32768)] if r else [])
    return finish(blocks_of(toks, rng, 300, 600) + blocks_of(m, rng, 100, 200))
