"""numpy restatement of the join contract of include/pdx/abi.h ("join"), and the reader of tests/golden/join_golden.npz.

TEST INFRASTRUCTURE: the product never imports this.  join_ref states the contract in the plainest way numpy allows -- stable sort of the
valid right keys, searchsorted, repeat -- and is itself held against Arrow's hash join by tests/test_join_golden.py (the multiset of
(left row, right row) pairs; Arrow's row ORDER is unspecified, this backend's is defined):
  - keys match by value; a null key matches nothing
  - inner: ordered by left row, the matches of one left row by ascending right row
  - left : the same, a left row without a match once, with a null right index
  - outer: left, then the right rows that no left row matched (null-key rows among them) in right row order, each with a null left index
  - semi / anti: the left rows with / without a match, each once, in left order; no right output
Value slots under a null index are 0.
"""
import json
import os

import numpy as np

HOWS = ("inner", "left", "outer", "semi", "anti")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "join_golden.npz")


def join_ref(lk, lv, rk, rv, how):
    """lk / rk: 1-d integer key arrays of one dtype; lv / rv: bool validity or None.  -> (left_idx, left_ok, right_idx, right_ok), int64 and
    bool arrays of the result's length; right_idx / right_ok are None for semi / anti."""
    lk, rk = np.asarray(lk), np.asarray(rk)
    nl, nr = len(lk), len(rk)
    lv = np.ones(nl, bool) if lv is None else np.asarray(lv, bool)
    rv = np.ones(nr, bool) if rv is None else np.asarray(rv, bool)
    rrows = np.flatnonzero(rv)
    order = rrows[np.argsort(rk[rrows], kind="stable")]  # the valid right rows by key, equal keys in row order
    sk = rk[order]
    lo = np.searchsorted(sk, lk, "left").astype(np.int64)
    cnt = (np.searchsorted(sk, lk, "right") - lo).astype(np.int64)
    cnt[~lv] = 0
    if how == "semi" or how == "anti":
        li = np.flatnonzero(cnt > 0 if how == "semi" else cnt == 0).astype(np.int64)
        return li, np.ones(len(li), bool), None, None
    outc = cnt if how == "inner" else np.maximum(cnt, 1)
    total = int(outc.sum())
    li = np.repeat(np.arange(nl, dtype=np.int64), outc)
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(outc) - outc, outc)
    rok = np.repeat(cnt > 0, outc)
    ri = np.zeros(total, np.int64)
    ri[rok] = order[(np.repeat(lo, outc) + within)[rok]]
    lok = np.ones(total, bool)
    if how == "outer":
        hit = np.zeros(nr, bool)
        hit[ri[rok]] = True
        tail = np.flatnonzero(~hit).astype(np.int64)
        li = np.concatenate([li, np.zeros(len(tail), np.int64)])
        lok = np.concatenate([lok, np.zeros(len(tail), bool)])
        ri = np.concatenate([ri, tail])
        rok = np.concatenate([rok, np.ones(len(tail), bool)])
    return li, lok, ri, rok


def pair_multiset(li, lok, ri, rok):
    """the result as sorted (left row | -1, right row | -1) pairs: what can be compared with an engine whose row order is unspecified"""
    a = np.where(lok, li, -1).astype(np.int64)
    b = np.full(len(a), -1, np.int64) if ri is None else np.where(rok, ri, -1).astype(np.int64)
    p = np.stack([a, b], axis=1) if len(a) else np.zeros((0, 2), np.int64)
    return p[np.lexsort((p[:, 1], p[:, 0]))]


NP_KEY = {"i64": np.int64, "u64": np.uint64, "ts": np.int64, "i32": np.int32}


def load_golden():
    """-> (manifest dict, get(name) -> ndarray).  Every array is stored as int64 in one blob (uint64 keys as their bits)."""
    z = np.load(GOLDEN)
    man = json.loads(bytes(z["manifest"]).decode())
    blob = z["blob"]

    def get(name):
        first, count = man["arrays"][name]
        return blob[first:first + count]

    return man, get


def golden_inputs(case, get):
    """-> (lk, lv, rk, rv) of a manifest case, keys in their own dtype"""
    dt = NP_KEY[case["dtype"]]
    name = case["name"]

    def key(side):
        raw = get(f"{name}/{side}k")
        return raw.view(np.uint64) if dt is np.uint64 else raw.astype(dt)

    return key("l"), get(f"{name}/lv").astype(bool), key("r"), get(f"{name}/rv").astype(bool)
