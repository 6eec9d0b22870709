"""A Zstandard frame WRITER for tests, written from RFC 8878: every encoding is chosen by the caller (literals
format and size format, Huffman weights and how they are described, sequence table modes and accuracy logs,
Offset_Value codes including the repeat codes, frame header fields).  There is no compressor and no heuristic.
A frame comes back magicless (what a NAF section holds) together with the bytes the writer's own model says it
decodes to, and the set of features it exercises.  Test helper only."""

MAGIC = b"\x28\xb5\x2f\xfd"

# ------------------------------------------------------------------------------------------------ bit writers


class ForwardBits:
    """Little-endian bit packing, first field in the lowest bits (FSE table descriptions)."""

    def __init__(self):
        self.acc = 0
        self.n = 0

    def put(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0 and value == 0
        self.acc |= value << self.n
        self.n += nbits

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


class BackwardBits:
    """A bitstream read from its end (Huffman streams, FSE streams): fields are given in the order the DECODER reads
    them; the stream is written in the opposite order and closed with the end mark."""

    def __init__(self):
        self.fields = []

    def put(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0 and value == 0, (value, nbits)
        self.fields.append((value, nbits))

    def bytes(self):
        acc, n = 0, 0
        for value, nbits in reversed(self.fields):
            acc |= value << n
            n += nbits
        acc |= 1 << n                                            # the end mark
        return acc.to_bytes(n // 8 + 1, "little")

    def nbits(self):
        return sum(b for _, b in self.fields)


# ------------------------------------------------------------------------------------------------ FSE


def fse_describe(norm, al):
    """Normalised counts -> FSE_Table_Description bytes (RFC 8878 4.1.1)."""
    assert 5 <= al <= 9 and sum(abs(c) for c in norm) == 1 << al
    last = max(i for i, c in enumerate(norm) if c != 0)
    w = ForwardBits()
    w.put(al - 5, 4)
    remaining, threshold, nbits = (1 << al) + 1, 1 << al, al + 1
    s = 0
    while s <= last:
        c = norm[s]
        mx = 2 * threshold - 1 - remaining
        remaining -= abs(c)
        v = c + 1
        if v >= threshold:
            v += mx
        if v < mx:
            w.put(v, nbits - 1)
        else:
            w.put(v, nbits)
        while remaining < threshold:
            nbits -= 1
            threshold >>= 1
        s += 1
        if c == 0:                                               # zero-probability run after a zero: 2-bit repeat flags
            run = 0
            while s + run <= last and norm[s + run] == 0:
                run += 1
            s += run
            while run >= 3:
                w.put(3, 2)
                run -= 3
            w.put(run, 2)
    assert remaining == 1
    return w.bytes()


def fse_table(norm, al):
    """Decoding table: per state (symbol, nb_bits, baseline), spread as RFC 8878 4.1.1 describes."""
    size = 1 << al
    sym = [None] * size
    high = size - 1
    nxt = {}
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s
            high -= 1
            nxt[s] = 1
        elif c > 0:
            nxt[s] = c
    step = (size >> 1) + (size >> 3) + 3
    pos = 0
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & (size - 1)
            while pos > high:
                pos = (pos + step) & (size - 1)
    assert pos == 0
    table = []
    for u in range(size):
        s = sym[u]
        x = nxt[s]
        nxt[s] += 1
        nb = al - (x.bit_length() - 1)
        table.append((s, nb, (x << nb) - size))
    return table


class FseEncoder:
    """For each symbol, the decoding state that outputs it and leads to a wanted next state."""

    def __init__(self, norm, al):
        self.al = al
        self.table = fse_table(norm, al) if al else None
        self.by_sym = {}
        if al:
            for u, (s, nb, base) in enumerate(self.table):
                self.by_sym.setdefault(s, []).append((u, nb, base))

    def any_state(self, s):
        return self.by_sym[s][0][0]

    def step(self, s, next_state):
        """-> (state, bits value, nb_bits): the state of symbol s whose update reads `bits` to reach next_state"""
        for u, nb, base in self.by_sym[s]:
            if base <= next_state < base + (1 << nb):
                return u, next_state - base, nb
        raise AssertionError("no state of symbol %d reaches %d" % (s, next_state))


def normalise(counts, al):
    """Some normalised distribution over the symbols with counts > 0: at least 1 each, the rest shared out by count;
    a symbol given count -1 keeps it ("less than 1")."""
    size = 1 << al
    norm = [0] * len(counts)
    fixed = sum(1 for c in counts if c != 0)
    assert fixed <= size
    for i, c in enumerate(counts):
        if c != 0:
            norm[i] = -1 if c < 0 else 1
    left = size - fixed
    pos = [i for i, c in enumerate(counts) if c > 0]
    tot = sum(counts[i] for i in pos)
    for i in pos:
        add = left * counts[i] // tot if tot else 0
        norm[i] += add
    short = size - sum(abs(c) for c in norm)
    norm[max(pos, key=lambda i: counts[i])] += short
    return norm


# ------------------------------------------------------------------------------------------------ Huffman


def huf_codes(weights):
    """weights[symbol] (0: absent) -> {symbol: (code, nb_bits)}, the canonical assignment of RFC 8878 4.2.1."""
    total = sum(1 << (w - 1) for w in weights if w)
    max_bits = total.bit_length() - 1
    assert total == 1 << max_bits and 1 <= max_bits <= 11, (total, max_bits)
    start, at = {}, 0
    for w in range(1, max_bits + 1):
        start[w] = at
        at += sum(1 for x in weights if x == w) << (w - 1)
    codes = {}
    for s, w in enumerate(weights):
        if w:
            nb = max_bits + 1 - w
            codes[s] = (start[w] >> (w - 1), nb)
            start[w] += 1 << (w - 1)
    return codes, max_bits


def weights_for_depths(depths):
    """{symbol: code length} of a complete prefix code -> weights list"""
    max_bits = max(depths.values())
    assert sum(2.0 ** -d for d in depths.values()) == 1.0
    w = [0] * (max(depths) + 1)
    for s, d in depths.items():
        w[s] = max_bits + 1 - d
    return w


def huf_describe(weights, form):
    """Huffman_Tree_Description: the weights of all symbols but the last, direct (4 bits each) or FSE-compressed."""
    last = max(i for i, w in enumerate(weights) if w)
    listed = weights[:last]
    if form == "direct":
        assert len(listed) <= 128
        pad = listed + [0] * (len(listed) & 1)
        return bytes([127 + len(listed)]) + bytes((pad[i] << 4) | pad[i + 1] for i in range(0, len(pad), 2))
    assert form == "fse" and 2 <= len(listed) <= 255
    counts = [0] * 13
    for w in listed:
        counts[w] += 1
    al = 6
    norm = normalise(counts[:max(i for i, c in enumerate(counts) if c) + 1], al)
    enc = FseEncoder(norm, al)
    # two interleaved states: state 1 decodes weights 0, 2, 4..., state 2 weights 1, 3, 5...; after the second-to-last
    # weight its state's update must run past the start of the stream, which ends the decode with one more weight
    n = len(listed)
    states = [None] * n
    ups = [None] * n
    for i in range(n - 1, -1, -1):
        if i + 2 < n:
            states[i], v, nb = enc.step(listed[i], states[i + 2])
            ups[i] = (v, nb)
        else:
            cands = [u for u, nb, _ in enc.by_sym[listed[i]] if i == n - 1 or nb > 0]
            assert cands, "the second-to-last weight needs a state that reads bits"
            states[i] = cands[0]
    bw = BackwardBits()
    bw.put(states[0], al)
    bw.put(states[1], al)
    for i in range(n - 2):
        bw.put(*ups[i])
    body = fse_describe(norm, al) + bw.bytes()
    assert len(body) < 128
    return bytes([len(body)]) + body


def huf_stream(data, codes):
    bw = BackwardBits()
    for b in data:
        bw.put(*codes[b])
    return bw.bytes()


# ------------------------------------------------------------------------------------------------ sequences

LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = [c + 3 for c in range(32)] + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195,
                                        16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
LL_DEF = ([4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1], 6)
ML_DEF = ([1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7, 6)
OF_DEF = ([1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5, 5)
MAX_AL = {"ll": 9, "of": 8, "ml": 9}


def code_of(value, base):
    for c in range(len(base) - 1, -1, -1):
        if value >= base[c]:
            return c
    raise ValueError(value)


def ll_code(v):
    return code_of(v, LL_BASE)


def ml_code(v):
    return code_of(v, ML_BASE)


def of_code(v):
    assert v >= 1
    return v.bit_length() - 1


# ------------------------------------------------------------------------------------------------ blocks and frames


class Lit:
    """How a compressed block's literals are written.  kind: raw / rle / huf / treeless.  sf: the Size_Format bits
    (None: the smallest that fits).  For huf: weights (list per byte value), form direct / fse, streams 1 or 4."""

    def __init__(self, kind, sf=None, weights=None, form="direct", streams=1):
        self.kind, self.sf, self.weights, self.form, self.streams = kind, sf, weights, form, streams


class Tbl:
    """A sequence table mode: predefined / rle (code) / fse (norm, al) / repeat."""

    def __init__(self, mode, code=None, norm=None, al=None):
        self.mode, self.code, self.norm, self.al = mode, code, norm, al


def auto_tables(seqs, al=None):
    """FSE tables for exactly the codes a list of (ll, ml, of_value) uses (accuracy logs: al dict or the smallest >= 5)"""
    out = {}
    for k, codes in (("ll", [ll_code(s[0]) for s in seqs]), ("ml", [ml_code(s[1]) for s in seqs]),
                     ("of", [of_code(s[2]) for s in seqs])):
        counts = [0] * (max(codes) + 1)
        for c in codes:
            counts[c] += 1
        a = (al or {}).get(k) or max(5, (sum(1 for c in counts if c) - 1).bit_length())
        out[k] = Tbl("fse", norm=normalise(counts, a), al=a)
    return out


class Frame:
    """Builder of ONE frame.  Blocks are added in order; the model of the decoder's state (output, repeat offsets,
    the previous Huffman tree and sequence tables) is kept alongside, and the frame's expected output comes from it."""

    def __init__(self, window_log=None, window_desc=None, single_segment=False, fcs=None, fcs_bytes=None,
                 checksum=False, dict_id=0):
        self.window_desc = window_desc if window_desc is not None else (None if window_log is None else (window_log - 10) << 3)
        self.single = single_segment
        self.fcs, self.fcs_bytes = fcs, fcs_bytes
        self.checksum, self.dict_id = checksum, dict_id
        self.blocks = []
        self.out = bytearray()
        self.rep = [1, 4, 8]
        self.huf = None
        self.tables = {}
        self.features = set()
        self.counts = {}           # literal sections per kind, sequence table modes per table: what the oracle's statistics count

    # ---- blocks
    def raw(self, data, size=None):
        self._block(0, bytes(data), len(data) if size is None else size)
        self.out += data
        self.features.add("block_raw")

    def rle(self, byte, n):
        self._block(1, bytes([byte]), n)
        self.out += bytes([byte]) * n
        self.features.add("block_rle")

    def compressed(self, literals, seqs=(), lit=None, tables=None, nseq_form=None, trailing=b""):
        """literals: the block's literal bytes; seqs: (ll, ml, offset_value) triples (sum of ll <= len(literals))"""
        lit = lit or Lit("raw")
        body = self._literals(bytes(literals), lit) + self._sequences(bytes(literals), list(seqs), tables or {}, nseq_form)
        self._block(2, body + trailing, len(body) + len(trailing))
        self.features.add("block_compressed")

    def _count(self, what, k=1):
        self.counts[what] = self.counts.get(what, 0) + k

    def _block(self, typ, body, size):
        self.blocks.append([typ, size, body])

    def _literals(self, data, lit):
        n = len(data)
        if lit.kind in ("raw", "rle"):
            t = 0 if lit.kind == "raw" else 1
            if lit.kind == "rle":
                assert n > 0 and data == data[:1] * n
            sf = lit.sf if lit.sf is not None else (0 if n < 32 else (1 if n < 4096 else 3))
            if sf in (0, 2):
                assert n < 32
                hdr = bytes([t | (sf << 2) | (n << 3)])
            elif sf == 1:
                assert n < 4096
                hdr = bytes([t | (1 << 2) | ((n & 15) << 4), n >> 4])
            else:
                assert n < 1 << 20
                hdr = bytes([t | (3 << 2) | ((n & 15) << 4), (n >> 4) & 255, n >> 12])
            self.features.add("lit_%s_hdr%d" % (lit.kind, len(hdr)))
            self._count("lit_" + lit.kind)
            return hdr + (data if t == 0 else data[:1])
        if lit.kind == "huf":
            tree = huf_describe(lit.weights, lit.form)
            self.huf = huf_codes(lit.weights)
            t = 2
            self.features.add("huf_weights_" + lit.form)
            if lit.form == "direct":
                self.features.add("huf_direct_%s" % ("odd" if (tree[0] - 127) & 1 else "even"))
        else:
            assert lit.kind == "treeless" and self.huf is not None
            tree, t = b"", 3
        codes, max_bits = self.huf
        self.features.add("huf_depth_%d" % max_bits)
        if lit.streams == 1:
            streams = huf_stream(data, codes)
        else:
            q = (n + 3) // 4
            parts = [huf_stream(data[k * q:(k + 1) * q], codes) for k in range(4)]
            assert all(len(p) < 65536 for p in parts[:3])
            streams = b"".join(len(p).to_bytes(2, "little") for p in parts[:3]) + b"".join(parts)
        comp = len(tree) + len(streams)
        sf = lit.sf
        if sf is None:
            big = max(n, comp)
            sf = (0 if lit.streams == 1 else 1) if big < 1024 else (2 if big < 16384 else 3)
        assert (sf == 0) == (lit.streams == 1)
        if sf <= 1:
            assert n < 1024 and comp < 1024
            v = t | (sf << 2) | (n << 4) | (comp << 14)
            hdr = v.to_bytes(3, "little")
        elif sf == 2:
            assert n < 16384 and comp < 16384
            hdr = (t | (sf << 2) | (n << 4) | (comp << 18)).to_bytes(4, "little")
        else:
            assert n < 1 << 18 and comp < 1 << 18
            hdr = (t | (sf << 2) | (n << 4) | (comp << 22)).to_bytes(5, "little")
        self.features.add("lit_%s_%dstream_hdr%d" % ("huf" if t == 2 else "treeless", lit.streams, len(hdr)))
        self._count("lit_huf" if t == 2 else "lit_treeless")
        return hdr + tree + streams

    def _sequences(self, lits, seqs, tables, nseq_form):
        n = len(seqs)
        if n < 128 and nseq_form != 2 or nseq_form == 1:
            assert n < 128
            hdr = bytes([n])
        elif n < 0x7F00 and nseq_form != 3:
            hdr = bytes([128 + (n >> 8), n & 255])
        else:
            hdr = bytes([255, (n - 0x7F00) & 255, (n - 0x7F00) >> 8])
        self.features.add("nseq_%db" % len(hdr) if n else "nseq_0")
        self._count("sequences", n)
        lpos = 0
        for ll, ml, ov in seqs:                           # the model: repeat offsets, then the bytes
            self.out += lits[lpos:lpos + ll]
            lpos += ll
            if ov > 3:
                off = ov - 3
                self.rep = [off] + self.rep[:2]
            else:
                idx = ov - 1 + (ll == 0)
                if idx == 0:
                    off = self.rep[0]
                elif idx < 3:
                    off = self.rep[idx]
                    self.rep = [off] + [r for k, r in enumerate(self.rep) if k != idx]
                else:
                    off = self.rep[0] - 1
                    self.rep = [off] + self.rep[:2]
                self.features.add("rep_%d_ll%s" % (ov, "0" if ll == 0 else "x"))
            assert 1 <= off <= len(self.out) and ml >= 3, (off, len(self.out), ml)
            for _ in range(ml):
                self.out.append(self.out[-off])
            self.features.update(("ll_code_%d" % ll_code(ll), "ml_code_%d" % ml_code(ml), "of_code_%d" % of_code(ov)))
        assert lpos <= len(lits)
        self.out += lits[lpos:]
        if n == 0:
            return hdr
        self.features.add("seq_few" if n <= 64 else "seq_many")
        modes, descr, enc = 0, b"", {}
        for k, shift, default in (("ll", 6, LL_DEF), ("of", 4, OF_DEF), ("ml", 2, ML_DEF)):
            t = tables.get(k) or Tbl("predefined")
            self.features.add("seq_%s_%s" % (k, t.mode))
            self._count("mode_%s_%s" % (k, t.mode))
            if t.mode == "predefined":
                modes |= 0 << shift
                enc[k] = FseEncoder(*default)
            elif t.mode == "rle":
                modes |= 1 << shift
                descr += bytes([t.code])
                enc[k] = ("rle", t.code)
            elif t.mode == "fse":
                modes |= 2 << shift
                descr += fse_describe(t.norm, t.al)
                enc[k] = FseEncoder(t.norm, t.al)
                self.features.add("seq_%s_al%d" % (k, t.al))
            else:
                modes |= 3 << shift
                enc[k] = self.tables[k]
            self.tables[k] = enc[k]
        codes = {"ll": [ll_code(s[0]) for s in seqs], "ml": [ml_code(s[1]) for s in seqs], "of": [of_code(s[2]) for s in seqs]}
        states, ups = {}, {}
        for k in ("ll", "of", "ml"):
            e, cs = enc[k], codes[k]
            if isinstance(e, tuple):
                assert all(c == e[1] for c in cs), (k, cs)
                states[k] = [0] * n
                ups[k] = [(0, 0)] * n
                continue
            st = [0] * n
            up = [(0, 0)] * n
            st[n - 1] = e.any_state(cs[n - 1])
            for i in range(n - 2, -1, -1):
                st[i], v, nb = e.step(cs[i], st[i + 1])
                up[i] = (v, nb)
            states[k], ups[k] = st, up
        al = {k: (0 if isinstance(enc[k], tuple) else enc[k].al) for k in enc}
        bw = BackwardBits()
        bw.put(states["ll"][0], al["ll"])
        bw.put(states["of"][0], al["of"])
        bw.put(states["ml"][0], al["ml"])
        for i, (ll, ml, ov) in enumerate(seqs):
            oc, mc, lc = codes["of"][i], codes["ml"][i], codes["ll"][i]
            bw.put(ov - (1 << oc), oc)
            bw.put(ml - ML_BASE[mc], ML_BITS[mc])
            bw.put(ll - LL_BASE[lc], LL_BITS[lc])
            if i < n - 1:
                bw.put(*ups["ll"][i])
                bw.put(*ups["ml"][i])
                bw.put(*ups["of"][i])
        return hdr + bytes([modes]) + descr + bw.bytes()

    # ---- the frame
    def payload(self):
        """-> (magicless frame bytes, expected decoded bytes, features)"""
        f = self.features
        fcs = len(self.out) if self.fcs is None and (self.fcs_bytes or self.single) else self.fcs
        if fcs is not None:
            nb = self.fcs_bytes or (1 if fcs < 256 and self.single else (2 if 256 <= fcs < 65536 + 256 else (4 if fcs < 1 << 32 else 8)))
        else:
            nb = 0
        flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[nb]
        assert nb != 1 or self.single
        dflag = 0 if not self.dict_id else (1 if self.dict_id < 256 else (2 if self.dict_id < 65536 else 3))
        fhd = (flag << 6) | (0x20 if self.single else 0) | (0x04 if self.checksum else 0) | dflag
        out = bytearray([fhd])
        if not self.single:
            out.append(self.window_desc if self.window_desc is not None else (17 - 10) << 3)
        out += self.dict_id.to_bytes([0, 1, 2, 4][dflag], "little")
        if nb:
            out += (fcs - 256 if nb == 2 else fcs).to_bytes(nb, "little")
            f.add("fcs_%d" % nb)
        f.add("single_segment" if self.single else "window_descriptor")
        if not self.blocks:
            self.blocks.append([0, 0, b""])
            f.add("block_empty_last")
        for k, (typ, size, body) in enumerate(self.blocks):
            last = k == len(self.blocks) - 1
            out += (int(last) | (typ << 1) | (size << 3)).to_bytes(3, "little") + body
        if self.checksum:
            out += (xxh64(bytes(self.out)) & 0xFFFFFFFF).to_bytes(4, "little")
            f.add("checksum")
        return bytes(out), bytes(self.out), set(f)

    def window_size(self):
        if self.single:
            return len(self.out)
        wd = self.window_desc if self.window_desc is not None else (17 - 10) << 3
        base = 1 << (10 + (wd >> 3))
        return base + (base // 8) * (wd & 7)


def xxh64(data, seed=0):
    """XXH64 (the xxHash specification)."""
    P1, P2, P3, P4, P5 = 11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579, 2870177450012600261
    M = (1 << 64) - 1

    def rotl(x, r):
        return ((x << r) | (x >> (64 - r))) & M

    def rnd(acc, lane):
        return (rotl((acc + lane * P2) & M, 31) * P1) & M

    n, p = len(data), 0
    if n >= 32:
        v = [(seed + P1 + P2) & M, (seed + P2) & M, seed, (seed - P1) & M]
        while p + 32 <= n:
            for k in range(4):
                v[k] = rnd(v[k], int.from_bytes(data[p + 8 * k:p + 8 * k + 8], "little"))
            p += 32
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & M
        for k in range(4):
            h = ((h ^ rnd(0, v[k])) * P1 + P4) & M
    else:
        h = (seed + P5) & M
    h = (h + n) & M
    while p + 8 <= n:
        h = (rotl(h ^ rnd(0, int.from_bytes(data[p:p + 8], "little")), 27) * P1 + P4) & M
        p += 8
    if p + 4 <= n:
        h = (rotl(h ^ ((int.from_bytes(data[p:p + 4], "little") * P1) & M), 23) * P2 + P3) & M
        p += 4
    while p < n:
        h = (rotl(h ^ ((data[p] * P5) & M), 11) * P1) & M
        p += 1
    h ^= h >> 33
    h = (h * P2) & M
    h ^= h >> 29
    h = (h * P3) & M
    h ^= h >> 32
    return h
