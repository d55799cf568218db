"""The key->slot path that every environment-steered group-by test reached on the commit before pdx_groupby_create was split into
one builder per path: the `slots` word of GroupByHandle.last_plan(), recorded per parameter set on an MI355X
(tests/golden/create_slots.json).  These tests check results only; a case that quietly took another path would still pass them."""
import json
import os

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "create_slots.json")) as fh:
    _PINNED = json.load(fh)


def pinned_slots(test, *params):
    """expected last_plan()["slots"] of `test` (the test's name without `test_`) for one parameter set"""
    return _PINNED[test]["-".join(str(p) for p in params)]
