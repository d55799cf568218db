"""Test-side Parquet builder and plain reference decoders (pure Python + numpy; no pyarrow, no GPU).

Written from the public format descriptions: the Snappy format description (raw block format), parquet-format's Encodings.md and
the Thrift compact protocol.  Three parts:

* ``SnappyComposer``: a stream is built from an explicit list of elements -- literal(bytes, nb), copy1 / copy2 / copy4(offset, len) --
  and the uncompressed bytes are their RESULT, so any legal (offset, length, header form) can be put at any stream position.  It returns
  a census of the shapes the stream holds, counted with the geometry of the workgroup decoder (4096-byte stream windows, 8192-byte
  output tiles, the 256 bytes kept in front of a tile), so that a test can assert that a case holds what it is named for.
  ``snappy_decode`` is the plain sequential reference; it raises on every malformed stream.
* ``HybridComposer``: explicit RLE / bit-packed runs at a given bit width, with the last group's padding cut short or the last run
  over-counted on request; ``hybrid_decode`` is its reference.
* ``build_file``: a minimal Parquet file around pages whose payload bytes (and, for SNAPPY, compressed bytes) the caller supplies:
  several row groups / columns / pages, data pages v1 and v2, an optional dictionary page, REQUIRED or OPTIONAL flat columns.
"""
import struct
from collections import Counter

import numpy as np

# ------------------------------------------------------------------------------------------------ Thrift compact protocol (writer)
T_TRUE, T_FALSE, T_BYTE, T_I16, T_I32, T_I64, T_DOUBLE, T_BINARY, T_LIST, T_SET, T_MAP, T_STRUCT = range(1, 13)


def varint(v):
    assert v >= 0
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def zigzag(v):
    return varint((v << 1) ^ (v >> 63) if v >= 0 else ((-v) << 1) - 1)


class ThriftWriter:
    def __init__(self):
        self.b = bytearray()
        self.last = [0]

    def _field(self, fid, ty):
        delta = fid - self.last[-1]
        if 0 < delta <= 15:
            self.b.append((delta << 4) | ty)
        else:
            self.b.append(ty)
            self.b += zigzag(fid)
        self.last[-1] = fid

    def i32(self, fid, v):
        self._field(fid, T_I32)
        self.b += zigzag(v)

    def i64(self, fid, v):
        self._field(fid, T_I64)
        self.b += zigzag(v)

    def boolean(self, fid, v):
        self._field(fid, T_TRUE if v else T_FALSE)

    def string(self, fid, s):
        self._field(fid, T_BINARY)
        s = s.encode() if isinstance(s, str) else s
        self.b += varint(len(s)) + s

    def list_header(self, fid, elem_type, n):
        self._field(fid, T_LIST)
        if n < 15:
            self.b.append((n << 4) | elem_type)
        else:
            self.b.append(0xF0 | elem_type)
            self.b += varint(n)

    def begin_struct(self, fid=None):  # fid None: an element of a list
        if fid is not None:
            self._field(fid, T_STRUCT)
        self.last.append(0)

    def end_struct(self):
        self.b.append(0)
        self.last.pop()


# ------------------------------------------------------------------------------------------------ Parquet file
BOOLEAN, INT32, INT64, FLOAT, DOUBLE = 0, 1, 2, 4, 5
UNCOMPRESSED, SNAPPY = 0, 1
PLAIN, PLAIN_DICTIONARY, RLE, RLE_DICTIONARY = 0, 2, 3, 8
NP_OF = {INT32: np.int32, INT64: np.int64, FLOAT: np.float32, DOUBLE: np.float64}


class Page:
    """kind: 'v1' | 'v2' | 'dict'.  raw: the uncompressed payload (v2: the values part only; levels: the v2 definition levels, stored
    as they are in front of it).  comp: the payload as stored when the chunk's codec is SNAPPY (None: stored uncompressed -- legal in a
    v2 page, is_compressed = false).  declared_raw overrides the header's uncompressed size (malformed-input cases only)."""

    def __init__(self, kind, num_values, encoding, raw, comp=None, levels=b"", num_nulls=0, declared_raw=None):
        self.kind, self.num_values, self.encoding, self.raw, self.comp = kind, num_values, encoding, bytes(raw), comp
        self.levels, self.num_nulls, self.declared_raw = bytes(levels), num_nulls, declared_raw

    def serialise(self, codec):
        stored = self.raw if (codec == UNCOMPRESSED or self.comp is None) else bytes(self.comp)
        assert codec == UNCOMPRESSED or self.comp is not None or self.kind == "v2", "a SNAPPY v1 / dictionary page needs its compressed bytes"
        raw_size = len(self.levels) + len(self.raw) if self.declared_raw is None else self.declared_raw
        t = ThriftWriter()
        t.i32(1, {"v1": 0, "dict": 2, "v2": 3}[self.kind])
        t.i32(2, raw_size)
        t.i32(3, len(self.levels) + len(stored))
        if self.kind == "v1":
            t.begin_struct(5)
            t.i32(1, self.num_values)
            t.i32(2, self.encoding)
            t.i32(3, RLE)
            t.i32(4, RLE)
            t.end_struct()
        elif self.kind == "dict":
            t.begin_struct(7)
            t.i32(1, self.num_values)
            t.i32(2, self.encoding)
            t.end_struct()
        else:
            t.begin_struct(8)
            t.i32(1, self.num_values)
            t.i32(2, self.num_nulls)
            t.i32(3, self.num_values)
            t.i32(4, self.encoding)
            t.i32(5, len(self.levels))
            t.i32(6, 0)
            t.boolean(7, codec == SNAPPY and self.comp is not None)
            t.end_struct()
        t.b.append(0)
        return bytes(t.b) + self.levels + stored, raw_size + len(t.b)


class Chunk:
    def __init__(self, name, physical, optional, codec, pages):
        self.name, self.physical, self.optional, self.codec, self.pages = name, physical, optional, codec, list(pages)


def build_file(row_groups):
    """row_groups: [(num_rows, [Chunk, ...]), ...]; every row group has the same columns.  Returns the file bytes."""
    out = bytearray(b"PAR1")
    placed = []
    for num_rows, chunks in row_groups:
        infos = []
        for ch in chunks:
            start = len(out)
            dict_off, data_off, raw_total = None, None, 0
            encodings = {RLE}
            for pg in ch.pages:
                if pg.kind == "dict":
                    dict_off = len(out)
                elif data_off is None:
                    data_off = len(out)
                encodings.add(PLAIN if pg.kind == "dict" else pg.encoding)
                blob, raw_size = pg.serialise(ch.codec)
                out += blob
                raw_total += raw_size
            infos.append((start, len(out) - start, raw_total, dict_off, data_off, sorted(encodings)))
        placed.append(infos)
    t = ThriftWriter()
    t.i32(1, 2)
    cols = row_groups[0][1]
    t.list_header(2, T_STRUCT, len(cols) + 1)
    t.begin_struct()
    t.string(4, "schema")
    t.i32(5, len(cols))
    t.end_struct()
    for ch in cols:
        t.begin_struct()
        t.i32(1, ch.physical)
        t.i32(3, 1 if ch.optional else 0)
        t.string(4, ch.name)
        t.end_struct()
    t.i64(3, sum(r for r, _ in row_groups))
    t.list_header(4, T_STRUCT, len(row_groups))
    for (num_rows, chunks), infos in zip(row_groups, placed):
        t.begin_struct()
        t.list_header(1, T_STRUCT, len(chunks))
        for ch, (start, size, raw_total, dict_off, data_off, encodings) in zip(chunks, infos):
            t.begin_struct()
            t.i64(2, start)
            t.begin_struct(3)
            t.i32(1, ch.physical)
            t.list_header(2, T_I32, len(encodings))
            for e in encodings:
                t.b += zigzag(e)
            t.list_header(3, T_BINARY, 1)
            t.b += varint(len(ch.name.encode())) + ch.name.encode()
            t.i32(4, ch.codec)
            t.i64(5, num_rows)
            t.i64(6, raw_total)
            t.i64(7, size)
            t.i64(9, data_off)
            if dict_off is not None:
                t.i64(11, dict_off)
            t.end_struct()
            t.end_struct()
        t.i64(2, sum(i[2] for i in infos))
        t.i64(3, num_rows)
        t.end_struct()
    t.string(6, "pdx test builder")
    t.b.append(0)
    out += t.b
    out += struct.pack("<I", len(t.b)) + b"PAR1"
    return bytes(out)


def plain_values(physical, values):
    """PLAIN encoding of the (non-null) values"""
    if physical == BOOLEAN:
        return np.packbits(np.asarray(values, bool), bitorder="little").tobytes()
    return np.ascontiguousarray(values, dtype=NP_OF[physical]).tobytes()


# ------------------------------------------------------------------------------------------------ Snappy
WIN, TILE, TAIL, DIRECT = 4096, 8192, 256, 2048  # the workgroup decoder's geometry (census only)


class SnappyComposer:
    def __init__(self):
        self.stream = bytearray()
        self.out = bytearray()
        self.elems = []  # (stream position, kind, header bytes, offset, length, output position)

    # ---- elements
    def literal(self, data, nb=None):
        data = bytes(data)
        n = len(data)
        assert n >= 1
        if nb is None:
            nb = 0 if n <= 60 else (n - 1).bit_length() + 7 >> 3
        assert nb in (0, 1, 2, 3, 4) and (n <= 60 if nb == 0 else n - 1 < 1 << (8 * nb))
        self.elems.append((len(self.stream), "lit%d" % nb, 1 + nb, 0, n, len(self.out)))
        if nb == 0:
            self.stream.append((n - 1) << 2)
        else:
            self.stream.append((59 + nb) << 2)
            self.stream += (n - 1).to_bytes(nb, "little")
        self.stream += data
        self.out += data
        return self

    def _copy(self, kind, hdr, off, n):
        assert 1 <= off <= len(self.out), (off, len(self.out))
        self.elems.append((len(self.stream) - hdr, kind, hdr, off, n, len(self.out)))  # (the header bytes are in the stream already)
        start = len(self.out) - off
        pattern = bytes(self.out[start:start + min(off, n)])  # a copy that overlaps its own output repeats its source with period `off`
        self.out += (pattern * (n // len(pattern) + 1))[:n]
        return self

    def copy1(self, off, n):
        assert 4 <= n <= 11 and off < 2048
        self.stream += bytes([1 | ((n - 4) << 2) | ((off >> 8) << 5), off & 0xFF])
        return self._copy("copy1", 2, off, n)

    def copy2(self, off, n):
        assert 1 <= n <= 64 and off < 65536
        self.stream += bytes([2 | ((n - 1) << 2)]) + off.to_bytes(2, "little")
        return self._copy("copy2", 3, off, n)

    def copy4(self, off, n):
        assert 1 <= n <= 64 and off < 1 << 32
        self.stream += bytes([3 | ((n - 1) << 2)]) + off.to_bytes(4, "little")
        return self._copy("copy4", 5, off, n)

    def copy(self, kind, off, n):
        return getattr(self, kind)(off, n)

    def raw_bytes(self, b):
        """stream bytes that produce nothing here: malformed-input cases only"""
        self.stream += bytes(b)
        return self

    # ---- results
    def finish(self, announce=None):
        """-> (compressed bytes incl. the length preamble, uncompressed bytes)"""
        return varint(len(self.out) if announce is None else announce) + bytes(self.stream), bytes(self.out)

    def census(self):
        c = Counter()
        for _, kind, hdr, off, n, _ in self.elems:
            c[kind] += 1
            canonical = {"lit0": True, "lit1": n > 60, "lit2": n > 256, "lit3": n > 65536, "lit4": n > 1 << 24, "copy1": True,
                         "copy2": not (4 <= n <= 11 and off < 2048), "copy4": off > 65535}[kind]
            c["noncanonical"] += not canonical
            c["overlapping"] += 0 < off < n
        c["max_offset"] = max([e[3] for e in self.elems], default=0)
        # windows, the way the decoder advances them: a window begins on an element, takes every element that BEGINS within 4096 stream
        # bytes of it, and the next one begins where the last of those ends (a literal's bytes included)
        i, ne, prev_s = 0, len(self.elems), 0
        edge, deltas = Counter(), Counter()
        prev_tile_len = None
        while i < ne:
            s = self.elems[i][0]
            j = i
            while j < ne and self.elems[j][0] < s + WIN:
                j += 1
            c["windows"] += 1
            c["max_window_elements"] = max(c["max_window_elements"], j - i)
            for pos, kind, hdr, off, n, opos in self.elems[i:j]:
                if pos - s >= WIN - 5:
                    edge[(kind, pos - s)] += 1
            if i > 0:
                c["window_starts_past_%d" % (s - prev_s - WIN)] += 1  # how far behind the previous window's 4096 bytes this one begins
            # tiles of the window's output: a literal with >= 2048 bytes left at a tile start goes straight to the output
            op, end = self.elems[i][5], self.elems[j - 1][5] + self.elems[j - 1][4]
            t0, k = op, i
            while t0 < end:
                while self.elems[k][5] + self.elems[k][4] <= t0:
                    k += 1
                _, kind, hdr, off, n, opos = self.elems[k]
                rem = opos + n - t0
                if kind.startswith("lit") and rem >= DIRECT:
                    c["direct_literals"] += 1
                    t0 += rem
                    prev_tile_len = rem
                    continue
                t1 = min(t0 + TILE, end)
                c["tiles"] += 1
                c["short_tiles"] += t1 - t0 < TAIL
                m = k
                while m < j and self.elems[m][5] < t1:
                    _, kind2, _, off2, n2, opos2 = self.elems[m]
                    p0 = max(opos2, t0)  # the copy's first byte inside this tile (it may reach in from the tile before)
                    n2 -= p0 - opos2
                    if off2 and p0 - off2 < t0:  # a copy that reads in front of the tile
                        src0 = p0 - off2
                        c["src_straddles_tile"] += src0 + n2 > t0
                        c["src_in_tail"] += src0 + n2 > t0 - TAIL
                        c["src_readback"] += src0 < t0 - TAIL
                        deltas[t0 - src0] += 1
                        # the bytes kept from BEFORE a short previous tile (the decoder shuffles them down instead of dropping them)
                        if prev_tile_len is not None and prev_tile_len < TAIL and t0 - TAIL <= src0 < t0 - prev_tile_len:
                            c["kept_tail_reads"] += 1
                    m += 1
                prev_tile_len = t1 - t0
                t0 = t1
            prev_s = s
            i = j
        c["edge_starts"] = edge      # (kind, window position) of the elements that begin on the last 5 bytes of a window
        c["tile_src_deltas"] = deltas  # (tile start - source start) of the copies that read in front of their tile
        return c


def merge_census(items):
    tot = Counter()
    for c in items:
        for k, v in c.items():
            if isinstance(v, Counter):
                tot[k] = tot.get(k, Counter()) + v
            elif k.startswith("max_"):
                tot[k] = max(tot.get(k, 0), v)
            else:
                tot[k] += v
    return tot


class SnappyError(ValueError):
    pass


def snappy_decode(buf, flaw=None):
    """Plain sequential reference: one element at a time, copies one byte at a time.  Raises SnappyError on any malformed stream.
    `flaw` selects a deliberately WRONG reading (tests prove with them that the cases bite): 'tag3_short' reads a 4-byte-offset copy
    with a 2-byte offset, 'nb3_masked' keeps 2 of a literal's 3 length bytes, 'memmove' copies an overlapping source as it lay before
    the copy, 'copy1_low' drops the offset bits a 1-byte-offset copy keeps in its tag."""
    buf = bytes(buf)
    n, ip, want, shift = len(buf), 0, 0, 0
    while True:
        if ip >= n or shift > 28:
            raise SnappyError("bad length preamble")
        b = buf[ip]
        ip += 1
        want |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            break
    out = bytearray()
    while ip < n:
        tag = buf[ip]
        ip += 1
        kind = tag & 3
        if kind == 0:
            ln = tag >> 2
            if ln >= 60:
                nb = ln - 59
                if ip + nb > n:
                    raise SnappyError("stream ends inside a literal header")
                ln = int.from_bytes(buf[ip:ip + (2 if flaw == "nb3_masked" and nb == 3 else nb)], "little")
                ip += nb
            ln += 1
            if ip + ln > n:
                raise SnappyError("stream ends inside a literal")
            out += buf[ip:ip + ln]
            ip += ln
        else:
            nb = (1, 2, 4)[kind - 1]
            if ip + nb > n:
                raise SnappyError("stream ends inside a copy header")
            if kind == 1:
                ln, off = 4 + ((tag >> 2) & 7), (0 if flaw == "copy1_low" else (tag >> 5) << 8) | buf[ip]
            else:
                if flaw == "tag3_short" and kind == 3:
                    nb = 2
                ln, off = (tag >> 2) + 1, int.from_bytes(buf[ip:ip + nb], "little")
            ip += nb
            if off == 0 or off > len(out):
                raise SnappyError("copy offset %d with %d bytes produced" % (off, len(out)))
            if flaw == "memmove":
                out += (bytes(out[len(out) - off:]) + bytes(ln))[:ln]
            else:
                for _ in range(ln):
                    out.append(out[-off])
        if len(out) > want:
            raise SnappyError("output runs past the announced length")
    if len(out) != want:
        raise SnappyError("output of %d bytes, %d announced" % (len(out), want))
    return bytes(out)


def snappy_encode_given(raw, rng, max_literal=3000, p_copy=0.8):
    """a legal stream for GIVEN bytes (pages whose content is fixed: index streams, values of nullable columns): literals of random
    length and header form, copies where a 4-byte match is known, in a random legal header form"""
    raw = bytes(raw)
    sn, n, i, seen = SnappyComposer(), len(raw), 0, {}
    while i < n:
        j = seen.get(raw[i:i + 4]) if i + 4 <= n else None
        if j is not None and rng.random() < p_copy:
            off, ln, cap = i - j, 4, int(rng.integers(4, 65))
            while ln < cap and i + ln < n and raw[i + ln] == raw[i + ln - off]:
                ln += 1
            forms = [k for k, ok in (("copy1", ln <= 11 and off < 2048), ("copy2", off < 65536), ("copy4", True)) if ok]
            sn.copy(forms[int(rng.integers(len(forms)))], off, ln)
        else:
            ln = min(n - i, int(rng.integers(1, max_literal)))
            least = 0 if ln <= 60 else (ln - 1).bit_length() + 7 >> 3
            sn.literal(raw[i:i + ln], int(rng.integers(max(least, 0 if ln <= 60 else 1), 5)) if rng.random() < 0.5 else None)
        for k in range(i, min(i + ln, n - 3), 1 if ln < 64 else 5):  # (long literals: every fifth position is enough to find matches)
            seen[raw[k:k + 4]] = k
        i += ln
    assert bytes(sn.out) == raw
    return sn


# ------------------------------------------------------------------------------------------------ RLE / bit-packed hybrid
def pack_bits(values, bw):
    """values -> bw bits each, LSB first"""
    if bw == 0 or len(values) == 0:
        return b""
    v = np.asarray(values, np.uint64)
    bits = ((v[:, None] >> np.arange(bw, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint8)
    return np.packbits(bits.reshape(-1), bitorder="little").tobytes()


class HybridComposer:
    def __init__(self, bw):
        self.bw, self.b, self.values, self.runs = bw, bytearray(), [], Counter()

    def rle(self, count, value, declared=None):
        """`count` values; the header announces `declared` (more than `count`: an over-counting LAST run)"""
        declared = count if declared is None else declared
        self.b += varint(declared << 1) + int(value).to_bytes((self.bw + 7) // 8, "little")
        self.values += [int(value)] * count
        self.runs["rle"] += 1
        self.runs["rle_header_%d" % len(varint(declared << 1))] += 1
        self.runs["overcount_rle"] += declared > count
        return self

    def packed(self, values, groups=None, cut=0):
        """values in groups of 8 (zero padding; more `groups` than the values need: an over-counting LAST run); `cut` bytes of the last
        group's padding are left out"""
        values = [int(x) for x in values]
        need = (len(values) + 7) // 8
        groups = need if groups is None else groups
        assert groups >= need and groups >= 1
        body = pack_bits(values + [0] * (groups * 8 - len(values)), self.bw)
        assert cut <= len(body) - (len(values) * self.bw + 7) // 8, "only padding may be cut"
        self.b += varint((groups << 1) | 1) + body[:len(body) - cut]
        self.values += values
        self.runs["packed"] += 1
        self.runs["packed_header_%d" % len(varint((groups << 1) | 1))] += 1
        self.runs["overcount_packed"] += groups > need
        self.runs["cut"] += cut > 0
        return self

    def finish(self):
        return bytes(self.b)


class HybridError(ValueError):
    pass


def hybrid_decode(buf, bw, need):
    """Plain reference: the first `need` values of the runs in buf.  Raises HybridError on a zero-count run or a stream that ends
    before the values it announces (padding behind the last needed value may be missing)."""
    buf = bytes(buf)
    out, pos, n = [], 0, len(buf)
    while len(out) < need:
        if pos >= n:
            raise HybridError("stream ends after %d of %d values" % (len(out), need))
        h, shift = 0, 0
        while True:
            if pos >= n:
                raise HybridError("stream ends inside a run header")
            b = buf[pos]
            pos += 1
            h |= (b & 0x7F) << shift
            shift += 7
            if not b & 0x80:
                break
        if h >> 1 == 0:
            raise HybridError("run of zero values")
        if h & 1:
            take = min((h >> 1) * 8, need - len(out))
            if pos + (take * bw + 7) // 8 > n:
                raise HybridError("stream ends inside a bit-packed run")
            word = int.from_bytes(buf[pos:pos + (h >> 1) * bw], "little")
            out += [(word >> (k * bw)) & ((1 << bw) - 1) for k in range(take)]
            pos += (h >> 1) * bw
        else:
            vb = (bw + 7) // 8
            if pos + vb > n:
                raise HybridError("stream ends inside an RLE run")
            out += [int.from_bytes(buf[pos:pos + vb], "little")] * min(h >> 1, need - len(out))
            pos += vb
    return out


def hybrid_from_values(values, bw, rng, p_rle=0.5):
    """a random legal run structure for GIVEN values: RLE where >= 8 equal values follow (or at random for shorter runs), bit-packed
    groups otherwise (whole groups of 8, except at the end)"""
    v = [int(x) for x in values]
    h, i, n = HybridComposer(bw), 0, len(v)
    while i < n:
        r = 1
        while i + r < n and v[i + r] == v[i]:
            r += 1
        if (r >= 8 and rng.random() < 0.9) or rng.random() < p_rle * 0.2 or (bw == 0):
            r = r if rng.random() < 0.5 else int(rng.integers(1, r + 1))
            h.rle(r, v[i])
            i += r
        else:
            g = int(rng.integers(1, 9))
            take = min(8 * g, n - i)
            h.packed(v[i:i + take])
            i += take
    return h
