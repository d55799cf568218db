"""GPU tests of csrc/elementwise.hip: pdx_binary, pdx_compare, pdx_if_else, pdx_unary, pdx_power, pdx_cast, pdx_cast_f64, pdx_logical and
pdx_invert on every dtype pair, scalar side, path (four rows per lane / a row per lane) and size edge, through the C ABI, against the
numpy reference (tests/_elementwise_ref.py) bit for bit and against Arrow's recorded digest or message
(tests/golden/elementwise_golden.npz, oracle/gen_golden_elementwise.py).

Every operand is a slice of a poisoned frame (tests/_elementwise_cases.py), all frames of a test in one upload.  The test owns the output:
capacity n + 130 rows, every byte pre-filled, so a row left unwritten or a row written behind n shows.  DESIGN section 20 has the edges."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _elementwise_cases as EC
import _elementwise_ref as R
from conftest import ROOT
from test_gpu_round2 import LIBM_TOL_ULP

pytestmark = pytest.mark.gpu

Z = np.load(os.path.join(ROOT, "tests", "golden", "elementwise_golden.npz"))
MANIFEST = json.loads(str(Z["manifest"]))


def _recipes():
    t, f, k = MANIFEST["types"], MANIFEST["families"], MANIFEST["kinds"]
    cols = [Z[x].tolist() for x in ("family", "op", "ta", "tb", "side", "n", "oi", "seed", "kind", "digest", "error")]
    return [((f[a], b, t[c], t[d], e, n, oi, s, k[kd]), dg, er) for a, b, c, d, e, n, oi, s, kd, dg, er in zip(*cols)]


RECIPES = _recipes()
GROUPS = EC.groups()
BIG = 100_000


def _of_group(group, big):
    return [r for r in RECIPES if (r[0][0], r[0][2], r[0][3], r[0][4]) == group and r[0][8] != "large" and (r[0][5] > BIG) == big]


LARGE = [r for r in RECIPES if r[0][8] == "large"]
BIG_ERROR_GROUPS = [g for g in GROUPS if _of_group(g, True)]


@pytest.fixture(scope="module")
def env():
    import torch

    from pandasarrow_amd import _lib as L

    assert torch.cuda.is_available()
    L.check(L.load().pdx_init(0))
    yield L, torch
    torch.cuda.empty_cache()  # (the large recipes leave gigabytes in torch's cache)


def _code(L, t):
    return {"i32": L.INT32, "i64": L.INT64, "f32": L.FLOAT32, "f64": L.FLOAT64, "u64": L.UINT64, "bool": L.BOOL}[t]


class Arena:
    """the frames of one operand role, one after the other (each starts on a multiple of 64 rows, which keeps its alignment and bit
    phase), uploaded once; the validity bitmap is addressed with the same row numbers as the values"""

    def __init__(self, t):
        self.t, self.vals, self.valid, self.pos, self.index = t, [], [], 0, {}

    def add(self, key, x):
        if key in self.index:
            return
        pad = -len(x.buf) % 64
        self.vals += [x.buf, np.zeros(pad, x.buf.dtype)]
        self.valid += [np.ones(len(x.buf), bool) if x.vbuf is None else x.vbuf, np.ones(pad, bool)]
        self.index[key] = (self.pos, x)
        self.pos += len(x.buf) + pad

    def upload(self, torch):
        pack = lambda parts: np.concatenate([np.packbits(np.concatenate(parts), bitorder="little"), np.zeros(16, np.uint8)])
        vals = np.concatenate(self.vals)
        host = pack(self.vals) if self.t == "bool" else vals.view(np.uint8)
        self.dvals = torch.from_numpy(host.copy()).cuda()
        self.dvalid = torch.from_numpy(pack(self.valid)).cuda()
        self.vals = self.valid = None

    def column(self, L, key):
        base, x = self.index[key]
        return L.PdxColumn(_code(L, self.t), 0, x.n, base + x.off, 0 if x.vbuf is None else -1, None if x.vbuf is None else self.dvalid.data_ptr(),
                           self.dvals.data_ptr())


class Output:
    """a values buffer and a validity buffer owned by the test, pre-filled before every call"""

    def __init__(self, torch, max_rows):
        self.torch = torch
        self.vals = torch.empty((max_rows + EC.TAIL + 4) * 8 + 64, dtype=torch.uint8, device="cuda")
        self.valid = torch.empty((max_rows + EC.TAIL) // 8 + 64, dtype=torch.uint8, device="cuda")

    def prepare(self, L, tname, n, with_validity, vbyte, fill, shift):
        """-> pdx_mut_column of capacity n + TAIL; shift: the values pointer advanced by one element (16-byte misaligned)"""
        self.w = 1 if tname == "bool" else R.NP[tname].itemsize
        self.nbytes = ((n + EC.TAIL + 7) // 8 + 8) if tname == "bool" else (n + EC.TAIL + 1) * self.w
        self.vbytes = (n + EC.TAIL + 7) // 8 + 8
        self.shift = shift * self.w
        self.vals[:self.nbytes + 8].fill_(fill)
        self.valid[:self.vbytes].fill_(vbyte)
        return L.PdxMutColumn(_code(L, tname), 0, n + EC.TAIL, -7, self.valid.data_ptr() if with_validity else None, self.vals.data_ptr() + self.shift)

    def read(self):
        self.torch.cuda.current_stream().synchronize()
        return self.vals[self.shift:self.shift + self.nbytes].cpu().numpy(), self.valid[:self.vbytes].cpu().numpy()


def _call(L, lib, rec, cols, m, st):
    family, op, ta, tb, side = rec[:5]
    a = C.byref(cols["a"])
    if family == "binary":
        return lib.pdx_binary(op, a, C.byref(cols["b"]), side, C.byref(m), st)
    if family == "compare":
        return lib.pdx_compare(op, a, C.byref(cols["b"]), side, C.byref(m), st)
    if family == "if_else":
        return lib.pdx_if_else(C.byref(cols["cond"]), a, C.byref(cols["b"]), side, C.byref(m), st)
    if family == "unary":
        return lib.pdx_unary(op, a, C.byref(m), st)
    if family == "power":
        return lib.pdx_power(a, EC.EXPONENTS[op], C.byref(m), st)
    if family == "cast":
        return lib.pdx_cast(a, C.byref(m), st)
    if family == "cast_f64":
        return lib.pdx_cast_f64(a, op, C.byref(m), st)
    if family == "logical":
        return lib.pdx_logical(op, a, C.byref(cols["b"]), C.byref(m), st)
    return lib.pdx_invert(a, C.byref(m), st)


def _first(bad):
    return np.flatnonzero(bad)[:5].tolist()


def _check_ok(rec, digest, ops, m, raw, vraw, with_validity, vbyte, fill):
    """the output of a call that returned PDX_OK against the reference, the recorded digest and the prefill"""
    family, op, ta, tb, side, n = rec[:6]
    want, ok, tname, libm = EC.reference(rec, ops)
    has_nulls = any(x.vbuf is not None for x in ops.values())
    assert m.length == n, (rec, m.length)
    assert m.null_count == (-1 if has_nulls else 0), (rec, m.null_count)
    if with_validity:
        got_ok = np.unpackbits(vraw, bitorder="little")[:n].astype(bool)
        assert np.array_equal(got_ok, ok), (rec, "validity, first rows", _first(got_ok != ok))
        behind = vraw[(n + 7) // 8:]
        assert (behind == vbyte).all(), (rec, "validity bytes behind the result were written", _first(behind != vbyte))
    else:
        assert ok.all(), rec
        assert (vraw == vbyte).all(), (rec, "a validity buffer that was not handed over was written")
    if tname == "bool":
        got = np.unpackbits(raw, bitorder="little")[:n].astype(bool)
        diff = (got != want) & ok
        behind = raw[(n + 7) // 8:]
    else:
        dt = R.NP[tname]
        allrows = raw.view(dt)
        got, behind = allrows[:n], allrows[n:].view(np.uint8)
        if libm:
            gc, wc = R.float_class(got), R.float_class(want)
            fin = ok & (wc < 2) & (gc < 2)
            diff = ((gc != wc) & ok)
            diff[fin] |= R.ulp_distance(got[fin], want[fin]) > LIBM_TOL_ULP
        else:
            diff = (EC._raw(got) != EC._raw(want)) & ok
    assert not diff.any(), f"{rec}: values, first rows {_first(diff)}: got {EC._raw(got[diff][:5])} want {EC._raw(want[diff][:5])}"
    assert (behind == fill).all(), (rec, "rows behind the result were written", _first(behind != fill))
    assert R.digest(got, ok, tname, libm) == digest, f"{rec}: Arrow's digest"


CHUNK = 1 << 22  # rows of a large recipe compared at a time


def _check_large(rec, digest, ops, m, raw, vraw, with_validity, vbyte, fill):
    """as _check_ok, in chunks of CHUNK rows: beside the inputs the host holds the output it read back and one chunk of the reference"""
    n = rec[5]
    tname, libm = EC.result_type(rec)
    assert m.length == n and m.null_count == (-1 if any(x.vbuf is not None for x in ops.values()) else 0), (rec, m.length, m.null_count)
    got_ok = np.unpackbits(vraw, bitorder="little")[:n].astype(bool) if with_validity else np.ones(n, bool)
    behind = vraw[(n + 7) // 8:] if with_validity else vraw
    assert (behind == vbyte).all(), (rec, "validity bytes behind the result were written", _first(behind != vbyte))
    if tname == "bool":
        got, tail = np.unpackbits(raw, bitorder="little")[:n].astype(bool), raw[(n + 7) // 8:]
    else:
        allrows = raw.view(R.NP[tname])
        got, tail = allrows[:n], allrows[n:].view(np.uint8)
    assert (tail == fill).all(), (rec, "rows behind the result were written", _first(tail != fill))
    d = R.StreamDigest(tname, libm)
    d.valid(got_ok)
    for s in range(0, n, CHUNK):
        e = min(n, s + CHUNK)
        want, ok, _, _ = EC.reference(rec, EC.rows(ops, s, e, n))
        assert np.array_equal(got_ok[s:e], ok), (rec, "validity, first rows", s + np.flatnonzero(got_ok[s:e] != ok)[:5])
        g = got[s:e]
        diff = ((g != want) if tname == "bool" else (EC._raw(g) != EC._raw(want))) & ok
        assert not diff.any(), f"{rec}: values, first rows {s + np.flatnonzero(diff)[:5]}: got {EC._raw(g[diff][:5])} want {EC._raw(want[diff][:5])}"
        if tname != "bool":
            assert not ((EC._raw(want) == EC._raw(EC.prefill_values(want.dtype, 1))[0]) & ok).any(), (rec, "an expected row equals the prefill")
        d.values(g, ok)
    assert d.value() == digest, f"{rec}: Arrow's digest"


def _large_prefills(rec, ops):
    """the prefill bytes of a large recipe from its last partial 64-row word alone"""
    n = rec[5]
    if not n & 63:
        return EC.PREFILL, EC.PREFILL
    want, ok, tname, _ = EC.reference(rec, EC.rows(ops, n & ~63, n, n))
    k = len(ok)
    return EC.bitmap_prefill(ok, np.ones(k, bool), k), (EC.bitmap_prefill(want, ok, k) if tname == "bool" else EC.PREFILL)


def _prefills(rec, ops):
    """-> (validity prefill byte, values prefill byte | None when the call must fail): chosen on the CPU so that no expected row equals it"""
    try:
        want, ok, tname, libm = EC.reference(rec, ops)
    except R.RefError:
        return EC.PREFILL, EC.PREFILL
    n = rec[5]
    vbyte = EC.bitmap_prefill(ok, np.ones(n, bool), n)
    if tname == "bool":
        return vbyte, EC.bitmap_prefill(want, ok, n)
    assert not ((EC._raw(want) == EC._raw(EC.prefill_values(want.dtype, 1))[0]) & ok).any(), (rec, "an expected row equals the prefill")
    return vbyte, EC.PREFILL


def _run(env, recipes):
    L, torch = env
    lib = L.load()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    inputs, arenas = {}, {}
    for rec, _, _ in recipes:
        key = EC.input_key(rec)
        if key not in inputs:
            inputs[key] = EC.inputs(rec)
            for name, x in inputs[key].items():
                arenas.setdefault(name, Arena(x.t)).add(key, x)
    for a in arenas.values():
        a.upload(torch)
    out = Output(torch, max(r[0][5] for r in recipes))
    ran = 0
    for rec, digest, err in recipes:
        family, op, ta, tb, side, n, oi = rec[:7]
        key = EC.input_key(rec)
        ops = inputs[key]
        cols = {name: arenas[name].column(L, key) for name in ops}
        tname = EC.result_type(rec)[0]
        large = rec[8] == "large"
        vbyte, fill = _large_prefills(rec, ops) if large else _prefills(rec, ops)
        has_nulls = any(x.vbuf is not None for x in ops.values())
        forms = [(True, 0)] + ([] if has_nulls else [(False, 0)])
        if oi == 0 and tname != "bool":
            forms.append((True, 1))  # the output 16-byte misaligned: the row-per-lane form although every input is aligned
        for with_validity, shift in forms:
            m = out.prepare(L, tname, n, with_validity, vbyte, fill, shift)
            rc = _call(L, lib, rec, cols, m, st)
            ran += 1
            if err >= 0:
                message = MANIFEST["messages"][err]
                assert rc == (L.NOT_IMPLEMENTED if message.startswith("Function '") else L.INVALID), (rec, rc)
                assert lib.pdx_last_error().decode() == message, rec
                continue  # (the next recipe is the check that a failed call leaves the library usable)
            assert rc == L.OK, f"{rec}: {rc} {lib.pdx_last_error().decode()}"
            raw, vraw = out.read()
            (_check_large if large else _check_ok)(rec, digest, ops, m, raw, vraw, with_validity, vbyte, fill)
    return ran


@pytest.mark.parametrize("group", GROUPS, ids=["-".join(map(str, g)).rstrip("-0") or "x" for g in GROUPS])
def test_small(env, group):
    """every op of the group at the 31 sizes x 5 offset pairs, and its error recipes at 5, 1027 and 4097 rows"""
    recipes = _of_group(group, False)
    assert len(recipes) >= len(EC.SIZES) * len(EC.OFFSETS) * 0.98
    assert _run(env, recipes) >= len(recipes)


def test_bit_not_on_floats_is_refused_by_name(env):
    L, torch = env
    for t, name in (("f32", "float"), ("f64", "double")):
        rec = ("unary", R.BIT_NOT, t, "", 0, 5, 0, 1, "small")
        ops = EC.inputs(rec)
        ar = Arena(t)
        ar.add(0, ops["a"])
        ar.upload(torch)
        out = Output(torch, 5)
        m = out.prepare(L, t, 5, True, EC.PREFILL, EC.PREFILL, 0)
        col = ar.column(L, 0)
        rc = L.load().pdx_unary(R.BIT_NOT, C.byref(col), C.byref(m), None)
        assert rc == L.NOT_IMPLEMENTED
        assert L.load().pdx_last_error().decode() == f"Function 'bit_wise_not' has no kernel matching input types ({name})"


@pytest.mark.parametrize("group", BIG_ERROR_GROUPS, ids=["-".join(map(str, g)).rstrip("-0") for g in BIG_ERROR_GROUPS])
def test_first_bad_row_past_the_grid_cap(env, group):
    """2,097,157 rows: out-of-range values in the first round, in the second round and in the n & 3 tail, in the vector and the row form"""
    _run(env, _of_group(group, True))


@pytest.mark.parametrize("k", range(len(LARGE)), ids=[f"{r[0][0]}-{r[0][2]}-{r[0][3]}-s{r[0][4]}-{r[0][5]}-o{r[0][6]}" for r in LARGE])
def test_large(env, k):
    """one op past a launch boundary of its kernel (the grid caps at 2,097,152 and 33,554,432 rows; the second trip of the 4x unrolled row
    loop of a misaligned 8-byte pair at 3,670,019 rows, and at 4,194,309 every lane's second trip with the plain loop behind it)"""
    _run(env, [LARGE[k]])
