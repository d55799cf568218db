"""The Parquet decoder cases: files built by tests/_parquet_build.py, each with the arrays it encodes and a census of the shapes it
holds.  Shared by tests/test_parquet_build.py (CPU: reference decoders, pyarrow as the judge of the builder, census assertions) and
tests/test_gpu_parquet_decoders.py (the kernels).  Everything is deterministic from the seeds written here."""
import functools
import struct
import zlib
from collections import Counter

import numpy as np

import _parquet_build as B

ALL_KINDS = ("lit0", "lit1", "lit2", "lit3", "lit4", "copy1", "copy2", "copy4")
NP_OUT = {B.BOOLEAN: np.bool_, B.INT32: np.int64, B.INT64: np.int64, B.FLOAT: np.float64, B.DOUBLE: np.float64}  # what the reader makes of them


class Col:
    def __init__(self, name, physical, pages, values, valid=None, codec=B.SNAPPY):
        self.chunk = B.Chunk(name, physical, valid is not None, codec, pages)
        self.name, self.physical, self.values, self.valid = name, physical, np.asarray(values), None if valid is None else np.asarray(valid, bool)


class Case:
    def __init__(self, name, cols, composers=(), hybrids=()):
        self.name, self.cols = name, list(cols)
        self.rows = len(self.cols[0].values)
        assert all(len(c.values) == self.rows for c in self.cols), name
        self.blob = B.build_file([(self.rows, [c.chunk for c in self.cols])])
        self.streams = [sn.finish() for sn in composers]            # (compressed, uncompressed) of every composed Snappy stream
        self.censuses = [sn.census() for sn in composers]
        self.census = B.merge_census(self.censuses)
        self.hybrids = [(h.finish(), h.bw, list(h.values)) for h in hybrids]
        self.runs = sum((h.runs for h in hybrids), Counter())


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def add_random(sn, rng, count, kinds=ALL_KINDS, max_lit=300):
    for _ in range(count):
        produced = len(sn.out)
        k = kinds[int(rng.integers(len(kinds)))]
        if produced == 0 and not k.startswith("lit"):
            k = "lit0"
        if k.startswith("lit"):
            nb = int(k[3])
            n = int(rng.integers(1, 61)) if nb == 0 else int(rng.integers(1, min(max_lit, 1 << (8 * nb)) + 1))
            sn.literal(rng.bytes(n), nb)
            continue
        reach = {"copy1": 2047, "copy2": 65535, "copy4": 1 << 40}[k]
        top = min(produced, reach)
        off = int(rng.integers(1, min(top, 300) + 1)) if rng.random() < 0.5 else int(rng.integers(1, top + 1))
        sn.copy(k, off, int(rng.integers(4, 12)) if k == "copy1" else int(rng.integers(1, 65)))
    return sn


def pad8(sn, rng, end="lit0"):
    """a last element of the given kind that brings the output to a multiple of 8 bytes"""
    p = (-len(sn.out)) % 8 or 8
    if end.startswith("lit"):
        return sn.literal(rng.bytes(p), int(end[3]))
    if end == "copy1" and p < 4:
        p += 8
    return sn.copy(end, min(len(sn.out), 7), p)


def i64_col(name, composers, codec=B.SNAPPY):
    pages, vals = [], []
    for sn in composers:
        comp, raw = sn.finish()
        assert len(raw) % 8 == 0 and raw, name
        pages.append(B.Page("v1", len(raw) // 8, B.PLAIN, raw, comp))
        vals.append(np.frombuffer(raw, np.int64))
    return Col(name, B.INT64, pages, np.concatenate(vals), None, codec)


def snappy_case(name, composers):
    return Case(name, [i64_col("v", composers)], composers)


# ================================================================================================ Snappy
LIT_LENGTHS = (1, 59, 60, 61, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 65535, 65536, 65537, 1 << 20)


def literal_forms():
    """every length-field form of a literal at every length of the list that it can hold (58 pages), then literals that are the page"""
    rng, sns = _rng("literal_forms"), []
    for n in LIT_LENGTHS:
        for nb in range(5):
            if (nb == 0 and n <= 60) or (nb > 0 and n - 1 < 1 << (8 * nb)):
                sns.append(pad8(B.SnappyComposer().literal(rng.bytes(n), nb), rng, "lit%d" % int(rng.integers(0, 5))))
    for n, nb in ((8, 0), (8, 4), (8, 3), (4096, 2), (4096, 3), (65536, 2), (1 << 20, 3), (1 << 20, 4)):
        sns.append(B.SnappyComposer().literal(rng.bytes(n), nb))
    return snappy_case("literal_forms", sns)


def window_straddle():
    """the element behind a leading literal begins on stream bytes 4090..4097 of the first window, for every element kind (headers of
    1..5 bytes cross the edge; the 30-byte literals cross the 16 bytes of slack behind the window as well)"""
    rng, sns = _rng("window_straddle"), []
    for kind in ALL_KINDS:
        for pos in range(4090, 4098):
            sn = B.SnappyComposer().literal(rng.bytes(pos - 3), 2)  # 3 header bytes + the literal = `pos` stream bytes
            if kind.startswith("lit"):
                sn.literal(rng.bytes(30), int(kind[3]))
            else:
                sn.copy(kind, int(rng.integers(1, 2048)), int(rng.integers(4, 12)))
            add_random(sn, rng, 40)
            sns.append(pad8(sn, rng))
    return snappy_case("window_straddle", sns)


def literal_past_window():
    """a first literal that ends 63 / 64 / 65 / 127 / 128 bytes behind the first window: the next window begins inside (63) or outside
    the bytes fetched ahead of time; dense elements follow, so that every byte of the next window counts"""
    rng, sns = _rng("literal_past_window"), []
    for d in (0, 1, 62, 63, 64, 65, 127, 128, 129, 4096):
        sn = B.SnappyComposer().literal(rng.bytes(4096 + d - 3), 2)
        add_random(sn, rng, 2500, ("lit0", "copy1", "copy2", "copy4", "lit1"), 40)
        sns.append(pad8(sn, rng))
    return snappy_case("literal_past_window", sns)


def copy1_full_range():
    rng = _rng("copy1_full_range")
    sn = B.SnappyComposer().literal(rng.bytes(2048))
    for off in range(1, 2048):
        for n in range(4, 12):
            sn.copy1(off, n)
    return snappy_case("copy1_full_range", [pad8(sn, rng, "copy1")])


def copy2_offsets():
    rng = _rng("copy2_offsets")
    sn = B.SnappyComposer().literal(rng.bytes(65536))
    for off in (1, 2047, 2048, 32767, 32768, 65535):
        for n in (1, 4, 11, 12, 63, 64):
            sn.copy2(off, n)
            sn.literal(rng.bytes(int(rng.integers(1, 20))))
    add_random(sn, rng, 300, ("copy2",))
    return snappy_case("copy2_offsets", [pad8(sn, rng, "copy2")])


def copy4_far():
    """4-byte offsets, small and beyond anything a 64 KB-block encoder emits, up to the page's first byte; two pages of > 1 MB"""
    rng, sns = _rng("copy4_far"), []
    for page in range(2):
        sn = B.SnappyComposer().literal(rng.bytes((1 << 20) + 8 * page))
        for off in (1, 5, 100, 2047, 2048, 65535, 65536, 65537, 100000, 1 << 19, 1 << 20):
            for n in (1, 7, 64):
                sn.copy4(off, n)
                sn.literal(rng.bytes(int(rng.integers(1, 9))))
        for back in (0, 1, 2, 63, 64, 8191, 8192):  # the source begins on the page's first byte, or just behind it
            sn.copy4(len(sn.out) - back, 64)
        sn.literal(rng.bytes(5000))
        add_random(sn, rng, 400, ("copy4", "copy4", "copy2", "lit0"))
        sn.copy4(len(sn.out), 64)
        sns.append(pad8(sn, rng, "copy4"))
    return snappy_case("copy4_far", sns)


def noncanonical():
    """forms an encoder with a choice would not take: wide offsets for near sources, wide length fields for short literals, one-byte
    literals one after the other"""
    rng = _rng("noncanonical")
    sn = B.SnappyComposer().literal(rng.bytes(3000), 4)
    for off in (1, 3, 100, 2047):
        for n in (4, 8, 11):
            sn.copy2(off, n).copy4(off, n)
    for n in (1, 2, 59, 60):
        for nb in (1, 2, 3, 4):
            sn.literal(rng.bytes(n), nb)
    for n in (61, 256):
        for nb in (2, 3, 4):
            sn.literal(rng.bytes(n), nb)
    for _ in range(100):
        sn.literal(rng.bytes(1), int(rng.integers(0, 5)))
    add_random(sn, rng, 600, ("copy2", "copy4", "lit3", "lit4"), 50)
    return snappy_case("noncanonical", [pad8(sn, rng, "lit4")])


OVERLAP_OFFSETS = (1, 2, 3, 5, 7, 63, 64, 65)


def overlap_chains():
    """copies of length 64 whose source is the copy in front of them: 19 KB descend from one seed of `offset` bytes, through two tile
    borders -- the deepest pointer chains the tiles have to resolve"""
    rng, sns = _rng("overlap_chains"), []
    for off in OVERLAP_OFFSETS:
        sn = B.SnappyComposer().literal(rng.bytes(off))
        for k in range(300):
            sn.copy("copy4" if k % 7 == 3 else "copy2", off, 64)
        sns.append(pad8(sn, rng, "copy2"))
    return snappy_case("overlap_chains", sns)


def _fill_to(sn, rng, target):
    """short literals and copies until the output is `target` bytes long (the next element begins there)"""
    while len(sn.out) < target:
        gap = target - len(sn.out)
        if gap >= 64 and rng.random() < 0.93:
            sn.copy2(int(rng.integers(64, min(len(sn.out), 1400) + 1)), 64)
        else:
            sn.literal(rng.bytes(min(gap, int(rng.integers(1, 30)))))


def tile_tail():
    """copies that begin on (or just behind) a tile's first byte and read 255 / 256 / 257 bytes in front of it -- the switch between the
    256 bytes kept in LDS and the read-back from the output -- and copies whose source lies across the tile's first byte"""
    rng = _rng("tile_tail")
    sn = B.SnappyComposer().literal(rng.bytes(1500))
    for tile_at, kind in ((8192, "copy2"), (16384, "copy4"), (24576, "copy2")):
        for jj, delta in ((0, 256), (64, 255), (128, 257), (200, 1), (300, 20), (400, 256 + 300), (500, 8000)):
            _fill_to(sn, rng, tile_at + jj)
            sn.copy(kind, jj + delta, 50)  # source begins `delta` bytes in front of the tile
        _fill_to(sn, rng, tile_at + 600)
        sn.copy1(610, 11).copy1(700, 4)     # one-byte-offset forms of the same: sources 10 / 96 bytes in front of the tile
    assert len(sn.stream) < 4096, "one window, so that the tiles lie where the case wants them"
    return snappy_case("tile_tail", [pad8(sn, rng)])


def short_last_tile():
    """a window whose output is one full tile + 100 bytes: the short tile keeps 156 of the older bytes in the 256-byte tail, and the
    next window's first copies read exactly those (and the bytes on both sides of them)"""
    rng = _rng("short_last_tile")
    sn = B.SnappyComposer()
    for _ in range(10):
        sn.literal(rng.bytes(60))
    sn.literal(rng.bytes(3276), 2)
    for _ in range(69):
        sn.copy2(int(rng.integers(64, 3000)), 64)
    assert len(sn.stream) == 4096 and len(sn.out) == 8192 + 100
    for k, back in enumerate((200, 150, 101, 100, 99, 255, 256, 257, 1)):
        sn.copy1(back + 8 * k, 8)  # the source begins `back` bytes in front of the second window's output
    add_random(sn, rng, 50, ("copy1", "lit0"))
    return snappy_case("short_last_tile", [pad8(sn, rng)])


def dense_windows():
    """windows of 2048 two-byte elements (one-byte literals, 1-byte-offset copies, both), and windows of 3-byte copies of 64 bytes
    (1365 elements -> 87 KB of output, eleven tiles, from one window)"""
    rng, sns = _rng("dense_windows"), []
    sn = B.SnappyComposer()
    for _ in range(3 * 2048 + 8):
        sn.literal(rng.bytes(1))
    sns.append(pad8(sn, rng))
    sn = B.SnappyComposer().literal(rng.bytes(1)).literal(rng.bytes(1)).literal(rng.bytes(1))
    for _ in range(3 * 2048):
        sn.copy1(int(rng.integers(1, min(len(sn.out), 2047) + 1)), int(rng.integers(4, 12)))
    sns.append(pad8(sn, rng, "copy1"))
    sn = B.SnappyComposer().literal(rng.bytes(1))
    for k in range(3 * 2048):
        if rng.random() < 0.5:
            sn.literal(rng.bytes(1))
        else:
            sn.copy1(int(rng.integers(1, min(len(sn.out), 2047) + 1)), int(rng.integers(4, 12)))
    sns.append(pad8(sn, rng))
    sn = B.SnappyComposer().literal(rng.bytes(2))  # 3 stream bytes, like every element behind it
    for _ in range(4 * 1366):
        top = min(len(sn.out), 65535)
        sn.copy2(int(rng.integers(1, min(top, 200) + 1)) if rng.random() < 0.3 else int(rng.integers(1, top + 1)), 64)
    sns.append(pad8(sn, rng, "copy2"))
    return snappy_case("dense_windows", sns)


SIZES = (8, 120, 128, (1 << 14) - 8, 1 << 14, (1 << 14) + 8, (1 << 21) - 8, 1 << 21, (1 << 21) + 8)


def _sized(rng, size, ends="lit0"):
    """a page of exactly `size` bytes: 64 KB literals where there is room, a mix of elements, and a last element of kind `ends`"""
    sn = B.SnappyComposer()
    while size - len(sn.out) > 70000:
        sn.literal(rng.bytes(65536))
        add_random(sn, rng, 3, ("copy2", "copy4", "copy1"))
    while size - len(sn.out) > 400:
        add_random(sn, rng, 1, max_lit=200)
    last = {"copy1": 8, "copy2": 16, "copy4": 16}.get(ends, 8)
    if size - len(sn.out) > last:
        sn.literal(rng.bytes(size - len(sn.out) - last), 2 if size - len(sn.out) - last > 60 else None)
    if ends.startswith("lit"):
        sn.literal(rng.bytes(size - len(sn.out)), int(ends[3]))
    else:
        sn.copy(ends, min(len(sn.out), 5), size - len(sn.out))
    assert len(sn.out) == size
    return sn


def page_sizes():
    """uncompressed sizes whose length preamble takes 1, 2, 3 and 4 bytes; a stream of exactly two windows behind its preamble; pages
    that end on every element kind"""
    rng = _rng("page_sizes")
    sns = [_sized(rng, 8)] + [_sized(rng, s) for s in SIZES[1:]]
    sn = B.SnappyComposer()
    add_random(sn, rng, 500, max_lit=20)
    while len(sn.stream) < 8192 - 50:
        add_random(sn, rng, 1, ("copy1", "copy2"))
    x = 8192 - len(sn.stream) - 3 - 1  # a last literal (1 header byte) and a last copy (3 bytes) fill the stream to 8192 bytes
    sn.literal(rng.bytes(x))
    sn.copy2(9, (-len(sn.out)) % 8 or 8)
    assert len(sn.stream) == 8192
    sns.append(sn)
    for kind in ALL_KINDS:
        sns.append(_sized(rng, 4000, kind))
    return snappy_case("page_sizes", sns)


def _random_page(rng, size):
    sn = B.SnappyComposer()
    while size - len(sn.out) > 64:
        add_random(sn, rng, 1, max_lit=min(int(rng.choice([60, 300, 5000])), size - len(sn.out) - 64))
    if size > len(sn.out):
        sn.literal(rng.bytes(size - len(sn.out)), 4 if rng.random() < 0.3 else None)
    return sn


def _split_rows(rng, rows, npages):
    cuts = np.sort(rng.choice(np.arange(1, rows), npages - 1, replace=False))
    return np.diff(np.concatenate([[0], cuts, [rows]])).tolist()


def random_mix():
    """seeded random sequences over every element kind: one column of 4400 small pages (more Snappy segments than the decoder's grid has
    workgroups: the loop over segments), two of 30 larger ones, INT32 / DOUBLE beside INT64"""
    rng = _rng("random_mix")
    rows = 70000
    cols, composers = [], []
    for name, physical, npages in (("many", B.INT64, 4400), ("wide", B.DOUBLE, 30), ("i32", B.INT32, 30)):
        width = 8 if physical in (B.INT64, B.DOUBLE) else 4
        pages, raws = [], []
        for r in _split_rows(rng, rows, npages):
            sn = _random_page(rng, r * width)
            comp, raw = sn.finish()
            pages.append(B.Page("v1" if rng.random() < 0.5 else "v2", r, B.PLAIN, raw, comp))
            raws.append(raw)
            composers.append(sn)
        vals = np.frombuffer(b"".join(raws), B.NP_OF[physical])
        cols.append(Col(name, physical, pages, vals.astype(NP_OUT[physical])))
    return Case("random_mix", cols, composers)


def mixed_codecs():
    """Snappy and uncompressed chunks in one file, and v2 pages stored uncompressed inside a Snappy chunk"""
    rng = _rng("mixed_codecs")
    rows, composers = 40000, []
    a = [_random_page(rng, r * 8) for r in _split_rows(rng, rows, 9)]
    c = [_random_page(rng, r * 8) for r in _split_rows(rng, rows, 5)]
    plain = rng.integers(-2 ** 62, 2 ** 62, rows)
    pb = [B.Page("v1", len(x), B.PLAIN, x.tobytes()) for x in np.array_split(plain, 4)]
    d = rng.standard_normal(rows)
    pd = []
    for k, x in enumerate(np.array_split(d, 6)):
        sn = B.snappy_encode_given(x.tobytes(), rng)
        composers.append(sn)
        pd.append(B.Page("v2", len(x), B.PLAIN, x.tobytes(), sn.finish()[0] if k % 2 else None))
    f = rng.standard_normal(rows).astype(np.float32)
    f[:4] = [np.inf, -0.0, np.float32(1e-45), -np.inf]
    pf = []
    for x in np.array_split(f, 3):
        sn = B.snappy_encode_given(x.tobytes(), rng)
        composers.append(sn)
        pf.append(B.Page("v1", len(x), B.PLAIN, x.tobytes(), sn.finish()[0]))
    return Case("mixed_codecs", [i64_col("a", a), Col("b", B.INT64, pb, plain, None, B.UNCOMPRESSED), i64_col("c", c), Col("d", B.DOUBLE, pd, d),
                                 Col("f32", B.FLOAT, pf, f.astype(np.float64))], a + c + composers)


# ================================================================================================ levels, dictionaries, booleans
def optional_col(name, physical, values, valid, page_rows, version, codec, rng, composers, hybrids, bool_rle=False, dictionary=None):
    """pages of an OPTIONAL column: definition levels as random legal runs, PLAIN values (or RLE booleans / dictionary indices) of the
    valid rows; SNAPPY: a stream composed for exactly those bytes"""
    pages, at = [], 0
    if dictionary is not None:
        raw = B.plain_values(physical, dictionary)
        sn = B.snappy_encode_given(raw, rng)
        composers.append(sn)
        pages.append(B.Page("dict", len(dictionary), B.PLAIN, raw, sn.finish()[0]))
    for r in page_rows:
        ok = valid[at:at + r]
        lev = B.hybrid_from_values(ok.astype(int), 1, rng)
        hybrids.append(lev)
        live = values[at:at + r][ok]
        encoding = B.PLAIN
        if dictionary is not None:
            bw = max(int(len(dictionary) - 1).bit_length(), 1) + int(rng.integers(0, 3))
            idx = B.hybrid_from_values(live, bw, rng)
            hybrids.append(idx)
            body, encoding = bytes([bw]) + idx.finish(), B.RLE_DICTIONARY
        elif bool_rle:
            h = B.hybrid_from_values(live.astype(int), 1, rng)
            hybrids.append(h)
            body, encoding = struct.pack("<I", len(h.finish())) + h.finish(), B.RLE
        else:
            body = B.plain_values(physical, live)
        nulls = int(r - ok.sum())
        if version == 1:
            raw, levels = struct.pack("<I", len(lev.finish())) + lev.finish() + body, b""
        else:
            raw, levels = body, lev.finish()
        comp = None
        if codec == B.SNAPPY:
            sn = B.snappy_encode_given(raw, rng) if raw else B.SnappyComposer()
            composers.append(sn)
            comp = sn.finish()[0]
        pages.append(B.Page("v%d" % version, r, encoding, raw, comp, levels, nulls))
        at += r
    assert at == len(values)
    expect = values if dictionary is None else np.asarray(dictionary)[values]
    return Col(name, physical, pages, np.asarray(expect).astype(NP_OUT[physical]), valid, codec)


LEVEL_ROWS = (1, 63, 64, 65, 100003)


def _level_pages(rng):
    """validity of the pages the issue lists, in order"""
    pages = [np.zeros(70, bool), np.ones(70, bool), np.zeros(1, bool), np.ones(1, bool)]
    for n in (2, 64, 65, 1000):
        a, b = np.ones(n, bool), np.ones(n, bool)
        a[0], b[-1] = False, False
        pages += [a, b]
    for n, at in ((64, 0), (64, 63), (128, 64), (128, 127), (192, 128), (192, 63)):
        a = np.zeros(n, bool)
        a[at] = True
        pages.append(a)
    for n in LEVEL_ROWS:
        for density in (0.01, 0.5, 0.99):
            pages.append(rng.random(n) >= density)
    pages += [np.zeros(100003, bool), np.ones(4097, bool), np.zeros(64, bool)]
    return pages


def definition_levels(version, codec):
    name = "levels_v%d_%s" % (version, "snappy" if codec == B.SNAPPY else "plain")
    rng = _rng(name)
    pages = _level_pages(rng)
    valid = np.concatenate(pages)
    rows = [len(p) for p in pages]
    composers, hybrids = [], []
    i = rng.integers(-2 ** 62, 2 ** 62, len(valid))
    f = rng.standard_normal(len(valid))
    cols = [optional_col("i", B.INT64, i, valid, rows, version, codec, rng, composers, hybrids),
            optional_col("f", B.DOUBLE, f, valid[::-1].copy(), rows[::-1], version, codec, rng, composers, hybrids)]
    return Case(name, cols, composers, hybrids)


def booleans():
    """BOOLEAN columns with nulls: bit-packed PLAIN values in v1 and v2 pages, RLE values in v2 pages, with and without Snappy"""
    rng = _rng("booleans")
    rows = [1, 7, 8, 9, 63, 64, 65, 1000, 30011]
    n = sum(rows)
    composers, hybrids, cols = [], [], []
    for name, version, codec, rle, density in (("p1", 1, B.UNCOMPRESSED, False, 0.3), ("p2", 2, B.SNAPPY, False, 0.5), ("r2", 2, B.UNCOMPRESSED, True, 0.1),
                                               ("r2s", 2, B.SNAPPY, True, 0.9), ("r1s", 1, B.SNAPPY, True, 0.5)):
        vals = rng.random(n) < 0.5
        vals[n // 2: n // 2 + 3000] = True  # (long runs for the RLE form)
        cols.append(optional_col(name, B.BOOLEAN, vals, rng.random(n) >= density, rows, version, codec, rng, composers, hybrids, bool_rle=rle))
    return Case("booleans", cols, composers, hybrids)


def _dict_col(name, dictionary, index_pages, codec, rng, composers, dict_composer=None):
    """REQUIRED INT64 column: a PLAIN dictionary page and one RLE_DICTIONARY page per (bit width, HybridComposer)"""
    raw = B.plain_values(B.INT64, dictionary)
    pages = [B.Page("dict", len(dictionary), B.PLAIN, raw, dict_composer.finish()[0] if dict_composer else None)]
    vals = []
    for k, h in enumerate(index_pages):
        body = bytes([h.bw]) + h.finish()
        comp = None
        if codec == B.SNAPPY:
            sn = B.snappy_encode_given(body, rng)
            composers.append(sn)
            comp = sn.finish()[0]
        pages.append(B.Page("v2" if k % 2 else "v1", len(h.values), B.RLE_DICTIONARY, body, comp))
        vals.append(np.asarray(dictionary)[np.asarray(h.values, np.int64)])
    return Col(name, B.INT64, pages, np.concatenate(vals), None, codec)


def dict_bit_widths():
    """dictionary indices at every declared bit width 1..32 over a dictionary of five entries (and of 300, so that an RLE value's
    second byte counts), far above the width the dictionary needs"""
    rng = _rng("dict_bit_widths")
    small = rng.integers(-2 ** 62, 2 ** 62, 5)
    big = rng.integers(-2 ** 62, 2 ** 62, 300)
    hs, hb = [], []
    for bw in range(1, 33):
        top = min(5, 1 << bw)
        h = B.HybridComposer(bw)
        h.rle(3, int(rng.integers(top))).packed(rng.integers(0, top, 16)).rle(270, int(rng.integers(top))).packed(rng.integers(0, top, 21))
        hs.append(h)
        if bw >= 9:
            h = B.HybridComposer(bw)
            h.packed(rng.integers(0, 300, 64)).rle(10, 299).rle(200, 256).packed(rng.integers(0, 300, 3))
            hb.append(h)
    rows = sum(len(h.values) for h in hs)
    rest = rows - sum(len(h.values) for h in hb)
    hb.append(B.HybridComposer(9).rle(rest, 257))
    return Case("dict_bit_widths", [_dict_col("small", small, hs, B.UNCOMPRESSED, rng, []), _dict_col("big", big, hb, B.UNCOMPRESSED, rng, [])], (), hs + hb)


def dict_width_zero():
    """a one-entry dictionary whose index pages declare bit width 0: RLE runs without value bytes, and bit-packed runs without bytes"""
    rng = _rng("dict_width_zero")
    hs = [B.HybridComposer(0).rle(100, 0), B.HybridComposer(0).packed([0] * 64), B.HybridComposer(0).rle(1, 0), B.HybridComposer(0).rle(20000, 0).packed([0] * 5)]
    return Case("dict_width_zero", [_dict_col("one", np.array([-123456789012345], np.int64), hs, B.UNCOMPRESSED, rng, [])], (), hs)


RLE_COUNTS = (1, 2, 63, 64, 65, 127, 128, 20000)
PACKED_GROUPS = (1, 7, 8, 9, 64)


def hybrid_runs():
    """run shapes of the index stream: RLE counts with headers of 1, 2 and 3 bytes, bit-packed runs of 1..64 groups, strict
    alternation, a last group whose padding is cut short, last runs that announce more values than the page has, RLE values of
    1..4 bytes"""
    rng = _rng("hybrid_runs")
    d = rng.integers(-2 ** 62, 2 ** 62, 300)
    hs = []
    for bw in (9, 16, 24, 32):  # RLE values of 2, 2, 3, 4 bytes (1 byte: below)
        h = B.HybridComposer(bw)
        for c in RLE_COUNTS:
            h.rle(c, int(rng.integers(300)))
        for g in PACKED_GROUPS:
            h.packed(rng.integers(0, 300, 8 * g))
        hs.append(h)
    h = B.HybridComposer(8)
    for c in RLE_COUNTS:
        h.rle(c, int(rng.integers(256))).packed(rng.integers(0, 256, 8))
    hs.append(h)
    h = B.HybridComposer(5)  # strict alternation
    for _ in range(200):
        h.rle(1, int(rng.integers(32))).packed(rng.integers(0, 32, 8))
    hs.append(h)
    for bw, nvals in ((9, 9), (3, 17), (12, 1), (32, 15), (17, 33), (32, 9), (31, 1)):  # the padding of the last group is cut as far as it goes
        h = B.HybridComposer(bw).rle(5, 1)
        groups = (nvals + 7) // 8
        h.packed(rng.integers(0, min(300, 1 << bw), nvals), cut=groups * bw - (nvals * bw + 7) // 8)
        hs.append(h)
    hs.append(B.HybridComposer(9).packed(rng.integers(0, 300, 8)).rle(5, 7, declared=9))
    hs.append(B.HybridComposer(9).rle(1, 299, declared=1 << 30))
    hs.append(B.HybridComposer(9).rle(3, 1).packed(rng.integers(0, 300, 9), groups=5))
    hs.append(B.HybridComposer(20).packed(rng.integers(0, 300, 1), groups=64))
    return Case("hybrid_runs", [_dict_col("v", d, hs, B.UNCOMPRESSED, rng, [])], (), hs)


def dict_snappy_copy4():
    """a dictionary page that is itself a Snappy stream with 4-byte-offset copies reaching > 64 KB back; Snappy index pages behind it"""
    rng = _rng("dict_snappy_copy4")
    sn = B.SnappyComposer().literal(rng.bytes(80000))
    for _ in range(1200):
        sn.copy4(int(rng.integers(65536, len(sn.out) + 1)), 64)
        if rng.random() < 0.2:
            sn.literal(rng.bytes(int(rng.integers(1, 100))))
    pad8(sn, rng, "copy4")
    d = np.frombuffer(sn.finish()[1], np.int64)
    bw = int(len(d) - 1).bit_length()
    composers = [sn]
    hs = [B.hybrid_from_values(np.where(rng.random(r) < 0.3, 7, rng.integers(0, len(d), r)), bw, rng) for r in (5000, 1, 20000)]
    return Case("dict_snappy_copy4", [_dict_col("v", d, hs, B.SNAPPY, rng, composers, sn)], composers, hs)


def v2_optional_snappy():
    """v2 pages of OPTIONAL columns in a Snappy chunk (levels outside the compressed part), with an all-null page (an empty Snappy
    stream) and a dictionary-encoded column"""
    rng = _rng("v2_optional_snappy")
    rows = [100, 64, 5000, 1, 33333]
    n = sum(rows)
    valid = rng.random(n) > 0.3
    valid[100:164] = False
    composers, hybrids = [], []
    d = rng.integers(-2 ** 62, 2 ** 62, 37)
    cols = [optional_col("i", B.INT64, rng.integers(-2 ** 62, 2 ** 62, n), valid, rows, 2, B.SNAPPY, rng, composers, hybrids),
            optional_col("f", B.DOUBLE, rng.standard_normal(n), ~valid | (rng.random(n) > 0.5), rows, 2, B.SNAPPY, rng, composers, hybrids),
            optional_col("k", B.INT64, rng.integers(0, 37, n), valid, rows, 2, B.SNAPPY, rng, composers, hybrids, dictionary=d),
            optional_col("k1", B.INT64, rng.integers(0, 37, n), valid, rows, 1, B.SNAPPY, rng, composers, hybrids, dictionary=d)]
    return Case("v2_optional_snappy", cols, composers, hybrids)


SNAPPY_CASES = {f.__name__: f for f in (literal_forms, window_straddle, literal_past_window, copy1_full_range, copy2_offsets, copy4_far, noncanonical,
                                        overlap_chains, tile_tail, short_last_tile, dense_windows, page_sizes, random_mix, mixed_codecs,
                                        v2_optional_snappy, dict_snappy_copy4)}
HYBRID_CASES = {"dict_bit_widths": dict_bit_widths, "dict_width_zero": dict_width_zero, "hybrid_runs": hybrid_runs, "booleans": booleans}
for _v in (1, 2):
    for _c in (B.UNCOMPRESSED, B.SNAPPY):
        HYBRID_CASES["levels_v%d_%s" % (_v, "snappy" if _c == B.SNAPPY else "plain")] = functools.partial(definition_levels, _v, _c)
CASES = {**SNAPPY_CASES, **HYBRID_CASES}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


# ================================================================================================ refusals
def _refusal_file(comp, raw_size, declared_raw=None):
    """one REQUIRED INT64 v1 Snappy page whose stream is `comp`"""
    pg = B.Page("v1", raw_size // 8, B.PLAIN, bytes(raw_size), comp, declared_raw=declared_raw)
    return B.build_file([(raw_size // 8, [B.Chunk("v", B.INT64, False, B.SNAPPY, [pg])])])


def snappy_refusals():
    """name -> (file, compressed stream): malformed streams, each of which the reference decoder refuses too"""
    rng = np.random.default_rng(404)
    out = {}

    def put(name, sn, size, announce=None, cut=None, declared_raw=None):
        comp = sn.finish(size if announce is None else announce)[0]
        comp = comp if cut is None else comp[:cut]
        out[name] = (_refusal_file(comp, size, declared_raw), comp)

    lead = lambda n: B.SnappyComposer().literal(rng.bytes(n), 2)  # noqa: E731
    put("copy1_offset_0", lead(64).raw_bytes([1 | (4 << 2), 0]).literal(rng.bytes(56)), 128)
    put("copy2_offset_0", lead(64).raw_bytes([2 | (7 << 2), 0, 0]).literal(rng.bytes(56)), 128)
    put("copy4_offset_0", lead(64).raw_bytes([3 | (7 << 2), 0, 0, 0, 0]).literal(rng.bytes(56)), 128)
    put("offset_past_start_first_element", B.SnappyComposer().raw_bytes([2 | (7 << 2), 1, 0]).literal(rng.bytes(56)), 64)
    put("offset_one_past_produced", lead(64).raw_bytes([2 | (7 << 2), 65, 0]).literal(rng.bytes(56)), 128)
    # the first element of the second window: the leading literal (3 + 4093 bytes) is the first window
    put("offset_one_past_produced_second_window", lead(4093).raw_bytes([2 | (2 << 2)]).raw_bytes(struct.pack("<H", 4094)).literal(rng.bytes(40)), 4136)
    put("offset_one_past_produced_copy4_second_window", lead(4093).raw_bytes([3 | (2 << 2)]).raw_bytes(struct.pack("<I", 4094)).literal(rng.bytes(40)), 4136)
    put("copy4_offset_ffffffff", lead(64).raw_bytes([3 | (7 << 2), 255, 255, 255, 255]).literal(rng.bytes(56)), 128)
    put("output_one_byte_beyond_literal", lead(64).literal(rng.bytes(65)), 128)
    put("output_one_byte_beyond_copy", lead(64).copy2(10, 64).copy1(3, 4).literal(rng.bytes(60)).copy2(1, 1), 192)
    put("output_one_byte_short", lead(64).literal(rng.bytes(63)), 128)
    put("output_one_byte_short_copy", lead(64).copy2(10, 63), 128)
    for kind, hdr in (("copy1", 2), ("copy2", 3), ("copy4", 5), ("lit4", 5)):
        for keep in range(1, hdr):
            sn = lead(100)
            sn.copy(kind, 50, 8) if kind != "lit4" else sn.literal(rng.bytes(8), 4)
            put("cut_%s_header_after_%d" % (kind, keep), sn, 128, cut=1 + 3 + 100 + keep)
    put("cut_inside_literal", lead(128), 128, cut=60)
    put("cut_inside_literal_second_window", lead(4093).literal(rng.bytes(3003), 2), 7096, cut=2 + 4096 + 3 + 1000)
    put("announced_length_larger", lead(128), 128, announce=136)
    put("announced_length_smaller", lead(128), 128, announce=120)
    put("page_header_size_differs", lead(128), 128, declared_raw=136)
    return out


def hybrid_refusals():
    """name -> file"""
    rng = np.random.default_rng(405)
    d = rng.integers(0, 1000, 5)
    out = {}

    def dict_file(name, body, n, dsize=5):
        pages = [B.Page("dict", dsize, B.PLAIN, B.plain_values(B.INT64, d[:dsize])), B.Page("v1", n, B.RLE_DICTIONARY, body)]
        out[name] = B.build_file([(n, [B.Chunk("v", B.INT64, False, B.UNCOMPRESSED, pages)])])

    dict_file("index_equals_dictionary_size_rle", bytes([3]) + B.HybridComposer(3).rle(10, 1).rle(10, 5).finish(), 20)
    dict_file("index_equals_dictionary_size_packed", bytes([3]) + B.HybridComposer(3).packed([0, 1, 2, 3, 4, 5, 0, 1]).finish(), 8)
    dict_file("index_stream_zero_count_run", bytes([3]) + B.HybridComposer(3).rle(10, 1).finish() + bytes([0, 1]) + B.HybridComposer(3).rle(10, 2).finish(), 20)
    dict_file("index_stream_zero_groups_run", bytes([3]) + B.HybridComposer(3).rle(10, 1).finish() + bytes([1]) + B.HybridComposer(3).rle(10, 2).finish(), 20)
    dict_file("index_stream_ends_early", bytes([3]) + B.HybridComposer(3).rle(10, 1).finish(), 20)

    def level_file(name, levels, n, nonnull, version):
        vals = B.plain_values(B.INT64, rng.integers(0, 100, nonnull))
        if version == 1:
            pg = B.Page("v1", n, B.PLAIN, struct.pack("<I", len(levels)) + levels + vals)
        else:
            pg = B.Page("v2", n, B.PLAIN, vals, None, levels, n - nonnull)
        out[name] = B.build_file([(n, [B.Chunk("v", B.INT64, True, B.UNCOMPRESSED, [pg])])])

    for v in (1, 2):
        level_file("levels_v%d_rle_ends_early" % v, B.HybridComposer(1).rle(100, 1).finish(), 200, 100, v)
        # a bit-packed run that announces 25 groups and brings 20 bytes: rows 160..199 have no level (all-ones values follow them)
        level_file("levels_v%d_packed_ends_early" % v, B.HybridComposer(1).packed([1] * 200).finish()[:-5], 200, 200, v)
        level_file("levels_v%d_zero_count_run" % v, B.HybridComposer(1).rle(100, 1).finish() + bytes([0, 1]) + B.HybridComposer(1).rle(100, 1).finish(), 200, 200, v)
    return out
