"""The test-side Parquet builder (tests/_parquet_build.py) and the decoder cases (tests/_parquet_cases.py), judged without a GPU.

* the plain reference decoders return what the composers say their streams hold;
* pyarrow -- Arrow C++ with Google's Snappy decoder, which takes every legal element -- reads every built file back to the source
  values and nulls, bit for bit: a builder bug can neither pass as a kernel bug nor hide one;
* pdx_parquet_open accepts every built file;
* every case holds the shapes it is named for (census assertions: a case cannot degenerate silently);
* deliberately wrong readings of the Snappy format fail on the cases that target them: the cases bite."""
import ctypes as C
import io

import numpy as np
import pytest

import _parquet_build as B
import _parquet_cases as PC


@pytest.fixture(scope="module")
def lib():
    from pandasarrow_amd import _lib as L

    return L


def _check_pyarrow(blob, cols, rows):
    import pyarrow.parquet as pq

    t = pq.read_table(io.BytesIO(blob))
    t.validate(full=True)
    assert t.num_rows == rows and t.schema.names == [c.name for c in cols]
    for c in cols:
        a = t[c.name].combine_chunks()
        valid = np.ones(rows, bool) if c.valid is None else c.valid
        assert a.null_count == int((~valid).sum()), c.name
        assert np.array_equal(np.asarray(a.is_valid()), valid), c.name
        if c.physical == B.BOOLEAN:
            got = np.asarray(a.fill_null(False))
            assert np.array_equal(got[valid], c.values[valid]), c.name
        else:
            import pyarrow as pa

            got = a.fill_null(pa.scalar(0, a.type)).to_numpy(zero_copy_only=False).astype(c.values.dtype)  # (INT32 / FLOAT widen exactly)
            width = np.uint64
            assert np.array_equal(np.ascontiguousarray(got[valid]).view(width), np.ascontiguousarray(c.values[valid]).view(width)), c.name


@pytest.mark.parametrize("name", list(PC.CASES))
def test_reference_decoders_return_the_composed_bytes(name):
    case = PC.case(name)
    for comp, raw in case.streams:
        assert B.snappy_decode(comp) == raw
    for buf, bw, values in case.hybrids:
        assert B.hybrid_decode(buf, bw, len(values)) == values


@pytest.mark.parametrize("name", list(PC.CASES))
def test_pyarrow_reads_every_built_file(name):
    case = PC.case(name)
    _check_pyarrow(case.blob, case.cols, case.rows)


@pytest.mark.parametrize("name", list(PC.CASES))
def test_open_accepts_every_built_file(lib, name):
    case = PC.case(name)
    so, h = lib.load(), C.c_void_p()
    assert so.pdx_parquet_open(case.blob, len(case.blob), C.byref(h)) == 0, so.pdx_last_error()
    try:
        assert so.pdx_parquet_num_rows(h) == case.rows and so.pdx_parquet_num_columns(h) == len(case.cols)
        assert [so.pdx_parquet_column_name(h, i).decode() for i in range(len(case.cols))] == [c.name for c in case.cols]
    finally:
        so.pdx_parquet_destroy(h)


def test_several_row_groups_are_read_by_pyarrow_and_refused_by_name(lib):
    """the builder writes more than one row group; the reader takes one (as DataFrame::readParquet takes one record batch) and says so"""
    rng = np.random.default_rng(3)
    groups, vals = [], []
    for rows in (100, 1, 777):
        x = rng.integers(-2 ** 62, 2 ** 62, rows)
        sn = B.snappy_encode_given(x.tobytes(), rng)
        groups.append((rows, [B.Chunk("v", B.INT64, False, B.SNAPPY, [B.Page("v1", rows, B.PLAIN, x.tobytes(), sn.finish()[0])])]))
        vals.append(x)
    blob = B.build_file(groups)
    _check_pyarrow(blob, [PC.Col("v", B.INT64, [], np.concatenate(vals))], 878)
    so, h = lib.load(), C.c_void_p()
    assert so.pdx_parquet_open(blob, len(blob), C.byref(h)) != 0
    assert b"single record batch" in so.pdx_last_error()


# ------------------------------------------------------------------------------------------------ census: the cases hold their shapes
def test_census_literal_forms():
    c = PC.case("literal_forms").census
    per_nb = [sum(1 for n in PC.LIT_LENGTHS if (nb == 0 and n <= 60) or (nb > 0 and n - 1 < 1 << (8 * nb))) for nb in range(5)]
    assert per_nb == [3, 6, 15, 17, 17]
    for nb in range(5):
        assert c["lit%d" % nb] >= per_nb[nb], (nb, c)
    assert c["noncanonical"] >= 30 and c["direct_literals"] >= 30


def test_census_window_edges():
    c = PC.case("window_straddle").census
    for kind in PC.ALL_KINDS:
        for pos in range(4091, 4096):
            assert c["edge_starts"][(kind, pos)] >= 1, (kind, pos)
    # positions 4096 and 4097 are the next window's first element: the window begins right behind, or one byte behind, the 4096 bytes
    assert c["window_starts_past_0"] >= 8 and c["window_starts_past_1"] >= 8
    c = PC.case("literal_past_window").census
    for d in (63, 64, 65, 127, 128):
        assert c["window_starts_past_%d" % d] >= 1, d
    assert c["max_window_elements"] >= 300


def test_census_copies():
    c = PC.case("copy1_full_range").census
    assert c["copy1"] >= 2047 * 8 and c["max_offset"] == 2047 and c["max_window_elements"] == 2048
    c = PC.case("copy2_offsets").census
    assert c["copy2"] >= 336 and c["max_offset"] == 65535
    c = PC.case("copy4_far").census
    assert c["copy4"] >= 100 and c["max_offset"] > (1 << 20) and c["src_readback"] >= 1
    c = PC.case("noncanonical").census
    assert c["noncanonical"] >= 150 and c["copy4"] >= 12 and c["lit3"] >= 6 and c["lit4"] >= 6
    c = PC.case("overlap_chains").census
    assert c["overlapping"] >= 6 * 300 and c["tiles"] >= 3 * len(PC.OVERLAP_OFFSETS) and c["src_in_tail"] >= 2 * len(PC.OVERLAP_OFFSETS)  # (the chain crosses both tile borders)
    for comp, raw in PC.case("overlap_chains").streams:
        assert len(raw) >= 16384 + 2048


def test_census_tiles_and_tail():
    c = PC.case("tile_tail").census
    assert c["windows"] == 1 and c["tiles"] == 4 and c["direct_literals"] == 0
    for delta in (255, 256, 257):  # sources that begin 255 / 256 / 257 bytes in front of a tile, read by copies inside it
        assert c["tile_src_deltas"][delta] >= 3, (delta, c["tile_src_deltas"])
    assert c["src_straddles_tile"] >= 6 and c["src_in_tail"] >= 12 and c["src_readback"] >= 6
    c = PC.case("short_last_tile").census
    assert c["windows"] == 2 and c["short_tiles"] >= 1 and c["kept_tail_reads"] >= 3 and c["src_readback"] >= 1


def test_census_density_and_sizes():
    case = PC.case("dense_windows")
    c = case.census
    assert [x["max_window_elements"] for x in case.censuses] == [2048, 2048, 2048, 1366]  # literals, copies, both; 3-byte copies
    assert case.censuses[3]["tiles"] >= 4 * 10
    assert c["lit0"] >= 3 * 2048 and c["copy1"] >= 3 * 2048 and c["copy2"] >= 4 * 1365
    assert c["tiles"] >= 40
    case = PC.case("page_sizes")
    sizes = [len(raw) for _, raw in case.streams]
    assert sizes[:len(PC.SIZES)] == list(PC.SIZES)
    assert sorted({len(B.varint(s)) for s in sizes}) == [1, 2, 3, 4]
    comp = case.streams[len(PC.SIZES)][0]
    assert len(comp) - len(B.varint(sizes[len(PC.SIZES)])) == 8192
    assert case.census["copy4"] >= 1 and case.census["lit4"] >= 1
    case = PC.case("random_mix")
    assert len(case.streams) > 4096 + 60  # more Snappy segments than either decoder launches workgroups / waves
    for k in PC.ALL_KINDS:
        assert case.census[k] >= 300, (k, case.census[k])
    assert PC.case("dict_snappy_copy4").census["copy4"] >= 1200 and PC.case("dict_snappy_copy4").census["max_offset"] > 65535


def test_census_hybrid_runs():
    r = PC.case("hybrid_runs").runs
    assert r["rle_header_1"] >= 5 and r["rle_header_2"] >= 5 and r["rle_header_3"] >= 5 and r["rle_header_5"] >= 1
    assert r["packed_header_1"] >= 5 and r["packed_header_2"] >= 4
    assert r["cut"] == 7 and r["overcount_rle"] == 2 and r["overcount_packed"] == 2
    widths = sorted({bw for _, bw, _ in PC.case("dict_bit_widths").hybrids})
    assert widths == list(range(1, 33))
    assert {bw for _, bw, _ in PC.case("dict_width_zero").hybrids} == {0}
    for name in ("levels_v1_plain", "levels_v2_snappy"):
        case = PC.case(name)
        assert case.runs["rle"] >= 100 and case.runs["packed"] >= 100 and case.runs["rle_header_3"] >= 1
        col = case.cols[0]
        assert (~col.valid).sum() > 100000 and col.valid.sum() > 50000


# ------------------------------------------------------------------------------------------------ sensitivity: the cases bite
@pytest.mark.parametrize("flaw,target", [("tag3_short", "copy4_far"), ("nb3_masked", "literal_forms"), ("memmove", "overlap_chains"),
                                         ("copy1_low", "copy1_full_range"), ("tag3_short", "window_straddle"), ("memmove", "dense_windows")])
def test_wrong_readings_fail_on_their_target_case(flaw, target):
    wrong = 0
    streams = PC.case(target).streams
    for comp, raw in streams:
        try:
            wrong += B.snappy_decode(comp, flaw) != raw
        except B.SnappyError:
            wrong += 1
    assert wrong >= 1, (flaw, target)
    if target == "copy4_far":
        assert wrong == len(streams)
    if target == "overlap_chains":
        assert wrong >= 6  # (every offset below the copies' length)


# ------------------------------------------------------------------------------------------------ refusals are refused by the reference too
def test_malformed_streams_are_malformed():
    for name, (blob, comp) in PC.snappy_refusals().items():
        if name == "page_header_size_differs":  # (the stream itself is sound: the page header contradicts it)
            assert len(B.snappy_decode(comp)) == 128
            continue
        with pytest.raises(B.SnappyError):
            B.snappy_decode(comp)
    with pytest.raises(B.HybridError):
        B.hybrid_decode(B.HybridComposer(1).rle(100, 1).finish(), 1, 200)
    with pytest.raises(B.HybridError):
        B.hybrid_decode(B.HybridComposer(1).packed([1] * 200).finish()[:-5], 1, 200)
    with pytest.raises(B.HybridError):
        B.hybrid_decode(B.HybridComposer(3).rle(10, 1).finish() + bytes([0, 1]), 3, 20)
    assert len(PC.hybrid_refusals()) == 11


def test_open_accepts_the_malformed_pages(lib):
    """the damage is in the pages: the footer parser accepts these files, the refusal is the device decoders' (GPU tests)"""
    so = lib.load()
    files = [b for b, _ in PC.snappy_refusals().values()] + list(PC.hybrid_refusals().values())
    for blob in files:
        h = C.c_void_p()
        assert so.pdx_parquet_open(blob, len(blob), C.byref(h)) == 0, so.pdx_last_error()
        so.pdx_parquet_destroy(h)
