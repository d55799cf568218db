"""The Parquet page decoders (pandasarrow_amd/csrc/parquet.hip: k_pq_unsnap, k_pq_unpack, hybrid_decode behind k_pq_levels /
k_pq_values, k_pq_expand) on every legal Snappy and RLE / bit-packed shape, not only on those one encoder emits.

The files come from tests/_parquet_build.py: Snappy streams composed element by element (4-byte offsets, offsets > 64 KB, 3- and
4-byte literal lengths, non-canonical forms, elements placed on the decoder's window / tile / tail edges), hybrid runs composed run by
run (declared bit widths 0..32, over-counting and cut-short last runs), framed by a minimal file writer.  The expected values are the
arrays the builder encoded; tests/test_parquet_build.py proves on the CPU that pyarrow reads the same files to the same arrays.
Every file goes through DataFrame.readParquet under the workgroup decoder, the wave decoder (PDX_PQ_SNAPPY_WAVE=1) and, from 1 MB,
the upload in 1 MB pieces; values, validity and null counts must return bit for bit.  Malformed but bounds-checked inputs must fail
the load with a message under both decoders.

Cases: 16 Snappy files (4690 pages), 8 hybrid files (415 pages: dictionary indices, definition levels v1 / v2, booleans), 28 malformed
Snappy streams, 11 malformed hybrid streams."""
import numpy as np
import pytest

import _parquet_cases as PC

pytestmark = pytest.mark.gpu

SNAPPY_REFUSALS = PC.snappy_refusals()
HYBRID_REFUSALS = PC.hybrid_refusals()
KIND_DTYPE = {np.dtype(np.int64): 0, np.dtype(np.float64): 1, np.dtype(np.bool_): 2}


@pytest.fixture(scope="module")
def px():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from pandasarrow_amd import _lib as L
    from pandasarrow_amd import api, column

    L.check(L.load().pdx_init(0))

    class NS:
        pass

    ns = NS()
    ns.L, ns.K, ns.api = L, column, api
    return ns


def _settings(blob):
    return ("0", "1", "pieces") if len(blob) >= 1 << 20 else ("0", "1")


def _set(monkeypatch, setting):
    monkeypatch.setenv("PDX_PQ_SNAPPY_WAVE", "1" if setting == "1" else "0")
    if setting == "pieces":
        monkeypatch.setenv("PDX_PQ_UPLOAD_PIECE_MB", "1")
    else:
        monkeypatch.delenv("PDX_PQ_UPLOAD_PIECE_MB", raising=False)


def _check(px, case, setting):
    df = px.api.DataFrame.readParquet(case.blob)
    assert df.names == [c.name for c in case.cols] and df.num_rows() == case.rows, (case.name, setting)
    for c in case.cols:
        col = df[c.name].col
        assert col.dtype == KIND_DTYPE[c.values.dtype], (case.name, c.name)
        got, ok = col.to_numpy()
        valid = np.ones(case.rows, bool) if c.valid is None else c.valid
        ok = np.ones(case.rows, bool) if ok is None else ok
        assert np.array_equal(ok, valid), (case.name, c.name, setting, "validity")
        assert col.null_count == int((~valid).sum()), (case.name, c.name, setting, "null_count")
        if c.values.dtype == np.bool_:
            same = np.asarray(got, bool)[valid] == c.values[valid]
        else:
            same = np.ascontiguousarray(got).view(np.uint64)[valid] == np.ascontiguousarray(c.values).view(np.uint64)[valid]
        if not same.all():
            bad = np.flatnonzero(valid)[np.flatnonzero(~same)]
            raise AssertionError(f"{case.name}.{c.name} [{setting}]: {len(bad)} of {case.rows} rows differ, first at row {bad[0]}")


@pytest.mark.parametrize("name", list(PC.SNAPPY_CASES))
def test_snappy_shapes(px, monkeypatch, name):
    case = PC.case(name)
    for setting in _settings(case.blob):
        _set(monkeypatch, setting)
        _check(px, case, setting)


@pytest.mark.parametrize("name", list(PC.HYBRID_CASES))
def test_hybrid_shapes(px, monkeypatch, name):
    case = PC.case(name)
    for setting in _settings(case.blob):
        _set(monkeypatch, setting)
        _check(px, case, setting)


def test_the_pieces_form_is_reached(px):
    """the 1 MB-pieces upload is only taken by files of two pieces or more: the cases must hold some"""
    big = [n for n in PC.CASES if len(PC.case(n).blob) >= 2 << 20]
    assert len(big) >= 4, big


def _refused(px, monkeypatch, blob, what):
    for wave in ("0", "1"):
        _set(monkeypatch, wave)
        pf = px.K.ParquetFile(blob)
        with pytest.raises(RuntimeError, match="pdx_parquet"):
            pf.load()
        h, pf._h = pf._h, None
        assert px.L.load().pdx_parquet_destroy(h) == 0, (what, wave)
    # and the device is as it was: a sound file decodes
    _check(px, PC.case("overlap_chains"), "after " + what)


@pytest.mark.parametrize("name", list(SNAPPY_REFUSALS))
def test_malformed_snappy_is_refused(px, monkeypatch, name):
    _refused(px, monkeypatch, SNAPPY_REFUSALS[name][0], name)


@pytest.mark.parametrize("name", list(HYBRID_REFUSALS))
def test_malformed_hybrid_is_refused(px, monkeypatch, name):
    _refused(px, monkeypatch, HYBRID_REFUSALS[name], name)
