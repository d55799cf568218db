"""The path that every environment-steered group-by test reached before the host code behind it was split into one function per path.
These tests check results only; a case that quietly took another path would still pass them.

pinned_slots: the key->slot path, the `slots` word of GroupByHandle.last_plan() on the commit before pdx_groupby_create was split
(tests/golden/create_slots.json).  pinned_plan: the whole last_plan() -- slots, sort, layout, skew, side, reducer, bound, cache -- on the
commit before pdx_groupby_agg and build_layout were split (tests/golden/agg_plans.json).  Both recorded per parameter set on an MI355X;
the plans were identical in two runs.

One pinned case per function of gb_layout.hpp / gb_agg.hpp (ids are [seed-mode] of test_gpu_fuzz.py, bound = test_groupby_fuzz_bound_columns
with the kind of the call after the colon, else test_groupby_fuzz); the drivers, parse_agg_request, choose_reducer, reduce_std,
agg_std_unbound, pack_validity and compose_plan are entered by every case:
  layout_segments                          103-default (slots=runs)
  layout_single_group, with nulls          22-default (sort=none, seg_reduce_nullable)
  layout_full_sort, finish_sorted_slots    0-default
  sort_narrow_to_runs -> seal_fused        129-fused_dense (narrow), 131-fused_hash (narrow_part)
  ... -> build_side<uint8_t>               bound 19-bound_fused:5 (side=)
  ... -> finish_narrow_skewed              129-fused_side (nulls), 143-fused_hash (no nulls; narrow_part)
  sort_lsd_to_runs -> seal_fused           114-fused_dense (lsd:skip)
  ... -> build_side<uint32_t>              38-fused_side
  ... -> finish_partial_lsd                143-fused_dense (+finish)
  agg_std_bound, cache_alloc               bound 26-bound:3 (lds_acc fill), 0-bound:1 (sorted fill), 17-bound:1 (cache=hit)
  agg_variance                             bound 34-bound_fused:5 (fused form), 0-bound:5 (full form)
  agg_product_first_last                   bound 19-bound_fused:7 (the column already has a fused layout, from :5)
  reduce_fused (with_fused_rows, with_flag)  114-fused_dense (flr_reduce_dense), 129-fused_dense (flr_wave)"""
import json
import os

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(_GOLDEN, "create_slots.json")) as fh:
    _PINNED = json.load(fh)
with open(os.path.join(_GOLDEN, "agg_plans.json")) as fh:
    _PLANS = json.load(fh)


def pinned_slots(test, *params):
    """expected last_plan()["slots"] of `test` (the test's name without `test_`) for one parameter set"""
    return _PINNED[test]["-".join(str(p) for p in params)]


def pinned_plan(test, *params):
    """expected last_plan() of `test` for one parameter set (a test that aggregates more than once per set names the call last:
    the column, or the kind)"""
    return _PLANS[test]["-".join(str(p) for p in params)]
