"""The once-through stream paths of the headline group-by chain at their edges, bit-exact against the oracle.

1. The four-rows-per-lane form of the LDS-bitmap dense slot kernel: full tiles of a 16-byte aligned, non-null key column take it, the
   ragged last tile, a key column sliced by one row (8-byte aligned) and nullable keys keep the one-row-per-lane loop.  The pass-0
   histogram the kernel fuses is proven by the aggregates (the sort consumes it).
2. Its `few` peel (few distinct digits per wave step), which runs per sub-row in the wide loop.
3. Sort pass 0 over the 4-byte slots that kernel wrote (non-temporal payload loads): FLAGS pass (nullable values), PDX_SORT_NARROW=0
   (4-byte keys in every pass, keys written), ragged last tile, a sliced value column (8-byte aligned only).
4. The length of the first-row prefix (PDX_DENSE_PREFIX_PER_SLOT) changes speed only.

The shapes are the smallest that take these kernels: the speculative LDS tail needs n >= 2^23, <= 2^20 slots and >= 256 tail tiles; the
narrowing sort n >= 2^22 and three passes (>= 17 slot bits); the fused reducer >= 1024 rows per run (2^23 rows / 2^12 runs = 2048).  The
path is asserted through last_plan() and the profile tags, so a moved threshold fails here instead of testing another kernel.
No tolerances anywhere."""
import functools

import numpy as np
import pytest

import oracle as orc
from conftest import assert_f64_bits

pytestmark = pytest.mark.gpu

SUM, MEAN, COUNT = 0, 1, 4
N0 = 1 << 23
WIDE_KEYS = 150_000  # 18 slot bits: 6 + 6 narrowing passes + the fused 6-bit digit


@pytest.fixture(scope="module")
def px():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from pandasarrow_amd import _lib as L
    from pandasarrow_amd import column

    L.check(L.load().pdx_init(0))

    class NS:
        pass

    ns = NS()
    ns.L, ns.K, ns.Column, ns.torch = L, column, column.Column, torch
    return ns


def _profile(px, fn):
    """run fn() with the library's per-kernel timing on -> ({tag: launches}, fn's result)"""
    import ctypes as C

    lib = px.L.load()
    px.L.check(lib.pdx_profile_reset())
    px.L.check(lib.pdx_profile_enable(1))
    try:
        res = fn()
    finally:
        buf = C.create_string_buffer(1 << 16)
        px.L.check(lib.pdx_profile_report(buf, 1 << 16))
        lib.pdx_profile_enable(0)
        lib.pdx_profile_reset()
    tags = {}
    for line in buf.value.decode().splitlines():
        tag, count, _ms = line.split()
        tags[tag] = int(count)
    return tags, res


@functools.lru_cache(maxsize=None)
def _keys(kind, n):
    """host keys of one named input (shared, never written)"""
    if kind == "wide":
        k = orc.synth_keys(0, n, WIDE_KEYS)
    elif kind == "k1000":
        k = orc.synth_keys(0, n, 1000)
    elif kind == "equal":
        k = np.full(n, 42, np.int64)
    elif kind == "three":
        k = np.random.default_rng(5).integers(0, 3, n).astype(np.int64) * 7 + 100
    elif kind == "hot":  # 30 % of the rows on one key
        k = orc.synth_keys(0, n, WIDE_KEYS).copy()
        k[np.random.default_rng(6).random(n) < 0.30] = 77_777
    else:
        raise KeyError(kind)
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def _vals(n):
    v = orc.synth_vals(0, n) - 0.25
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def _key_valid(n):
    m = np.random.default_rng(7).random(n) > 0.05
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _val_valid(n):
    m = np.random.default_rng(8).random(n) > 0.05
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _groups(kind, n, null_keys):
    """oracle (ids, uniques, unique_is_null, first rows) of one named input"""
    return orc.group_ids(_keys(kind, n), _key_valid(n) if null_keys else None)


@functools.lru_cache(maxsize=None)
def _expected(kind, n, null_keys, null_vals):
    ids, uniq, _, _ = _groups(kind, n, null_keys)
    vv = _val_valid(n) if null_vals else None
    return [orc.groupby_agg(k, ids, len(uniq), _vals(n), vv, nthreads=8) for k in (SUM, MEAN, COUNT)]


def _run_and_check(px, kind, n, *, key_offset=0, val_offset=0, null_keys=False, null_vals=False, chain="narrow", what=""):
    """create + agg(sum, mean, count) with the profile on; ids, uniques, first rows and the three aggregates against the oracle.
    chain: "narrow" = the headline chain (dense slots, narrowing sort, fused last digit); "wide_keys" = 4-byte keys in every sort pass;
    "dense" = only the dense slot kernels are pinned (few slot bits or one hot key: the sort / reducer behind them is another one)."""
    keys, vals = _keys(kind, n), _vals(n)
    kcol = px.Column.from_numpy(keys, _key_valid(n) if null_keys else None, offset=key_offset)
    vcol = px.Column.from_numpy(vals, _val_valid(n) if null_vals else None, offset=val_offset)

    def run():
        gb = px.K.GroupByHandle.create(kcol)
        return gb, gb.agg(vcol, [SUM, MEAN, COUNT])

    tags, (gb, outs) = _profile(px, run)
    plan = gb.last_plan()
    assert plan["slots"] == "dense" and "dense_slots" in tags, (what, plan, tags)
    if chain == "narrow":
        assert plan["sort"].startswith("narrow:") and plan["layout"] == "fused", (what, plan)
        assert tags.get("radix_scatter") == 2 and tags.get("fused_last_digit_reduce") == 1, (what, tags)
    elif chain == "wide_keys":
        assert not plan["sort"].startswith("narrow:"), (what, plan)
        assert tags.get("radix_scatter", 0) >= 2, (what, tags)
    ids, uniq, isnull, first = _groups(kind, n, null_keys)
    assert gb.num_groups == len(uniq), what
    assert np.array_equal(gb.unique_keys().to_numpy()[0][~isnull], uniq[~isnull]), what
    assert np.array_equal(gb.first_rows().cpu().numpy(), first), what
    assert np.array_equal(gb.group_ids().cpu().numpy().astype(np.uint32), ids), what
    for k, out, (exp, eok) in zip((SUM, MEAN, COUNT), outs, _expected(kind, n, null_keys, null_vals)):
        got, ok = out.to_numpy()
        assert ok is None or np.array_equal(ok, eok), (what, k)
        if exp.dtype == np.float64:
            assert_f64_bits(got, exp, valid=eok, what=f"{what} kind={k}")
        else:
            assert np.array_equal(got[eok], exp[eok]), (what, k)
    return gb


# n % 4 and n % 4096 both hit; the key column as allocated (16-byte aligned: wide loop + ragged last tile) and sliced by one row
# (8-byte aligned pointer: the one-row-per-lane loop everywhere)
@pytest.mark.parametrize("sliced", [0, 1], ids=["aligned", "sliced"])
@pytest.mark.parametrize("r", [0, 1, 3, 4095])
def test_wide_dense_kernel_edges(px, r, sliced):
    _run_and_check(px, "wide", N0 + r, key_offset=sliced, what=f"r={r} sliced={sliced}")


def test_wide_dense_kernel_null_keys(px):
    """5 % null keys: the validity bitmap keeps the one-row-per-lane loop; the null slot is its own group"""
    _run_and_check(px, "wide", N0 + 3, null_keys=True, what="null keys")


def test_wide_dense_kernel_few_slot_bits(px):
    """1000 keys = 10 slot bits: the LDS tail (wide loop) in front of the classic sort"""
    _run_and_check(px, "k1000", N0 + 3, chain="dense", what="1000 keys")


@pytest.mark.parametrize("kind", ["equal", "three", "hot"])
def test_wide_dense_kernel_few_peel(px, kind, monkeypatch):
    """one digit, three digits (the peel stays on) and 30 % of the rows on one key among 150 000 (the peel is dropped at once).
    Only the slot kernels are pinned: what sorts and reduces behind them depends on the skew."""
    if kind == "equal":
        monkeypatch.setenv("PDX_GROUPBY_SORTED", "0")  # (equal keys arrive grouped: keep them off the run-label path)
    _run_and_check(px, kind, N0 + 3, chain="dense", what=kind)


@pytest.mark.parametrize("case", ["sliced_values", "null_values", "no_narrowing"])
def test_pass0_key_and_payload_paths(px, case, monkeypatch):
    """pass 0 over 4-byte slots in its three key forms, the value column sliced by one row; n has a ragged last tile"""
    n = N0 + 4095
    if case == "no_narrowing":
        monkeypatch.setenv("PDX_SORT_NARROW", "0")
    _run_and_check(px, "wide", n, val_offset=1, null_vals=case == "null_values", chain="wide_keys" if case == "no_narrowing" else "narrow", what=case)


@pytest.mark.parametrize("per_slot", ["1", "16"])
def test_prefix_length_is_speed_only(px, per_slot, monkeypatch):
    monkeypatch.setenv("PDX_DENSE_PREFIX_PER_SLOT", per_slot)
    _run_and_check(px, "hot", N0 + 3, chain="dense", what=f"prefix per slot {per_slot}")
