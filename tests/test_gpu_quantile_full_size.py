"""GPU: pdx_quantile beyond 2^32 rows, with ONE histogram bin holding more than 2^32 of them (every count and rank inside is 64 bits wide).
The expected values are known in closed form; no host copy of the column is made."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_more_than_2_to_32_rows_in_one_bin():
    import torch

    from pandasarrow_amd import _lib as L
    from pandasarrow_amd import column as K

    L.check(L.load().pdx_init(0))
    n = 2**32 + 2**20 + 7
    # int32 values i % 1000 for the first 2^32 + 7 rows: all of them share the key's top 11 bits (one bin of 2^32 + 7 rows); the last 2^20
    # rows are -5 (another bin, in front of it)
    t = torch.empty(n, dtype=torch.int32, device="cuda")
    step = 2**28
    for lo in range(0, n, step):
        hi = min(lo + step, n)
        t[lo:hi] = (torch.arange(lo, hi, device="cuda", dtype=torch.int64) % 1000).to(torch.int32)
    m = 2**32 + 7
    t[m:] = -5
    col = K.Column(L.INT32, n, t, None)
    qs = [0.0, 2.0**20 / (n - 1), 0.5, 1.0]
    got = K.quantile(col, qs, L.INTERP_LOWER)
    assert all(c == n for _, c in got)
    # sorted: 2^20 times -5, then every v in 0..999 either ceil or floor of m / 1000 times: v occurs m // 1000 + (v < m % 1000) times
    def at(rank):
        if rank < 2**20:
            return -5
        r = rank - 2**20
        per, extra = divmod(m, 1000)
        head = extra * (per + 1)
        return r // (per + 1) if r < head else extra + (r - head) // per

    want = [at(int(np.float64(n - 1) * np.float64(q))) for q in qs]
    assert [v for v, _ in got] == want
    assert want[0] == -5 and want[1] in (-5, 0) and want[2] in (499, 500) and want[3] == 999
    lin = K.quantile(col, [0.5])[0][0]
    assert lin == float(want[2])  # both neighbours of the middle rank are equal
    del t, col
    L.load().pdx_trim_pool()
