// test_facade_mode.cpp -- the value-frequency calls through the C++ facade (pandasarrow_amd/cpp/pdx.hpp -> pdx_mode, pdx_groupby_mode,
// pdx_groupby_create + pdx_groupby_unique_keys + pdx_groupby_sizes -> HIP kernels): Series::mode / value_counts / is_unique and
// GroupBy::mode on hand-checked cases (Arrow 25's rules: count descending, ties by value ascending, nulls take no part, a null is one
// value_counts entry).  Built with g++ (host code only) and run on the GPU box by tests/test_gpu_cpp_mode.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>

#include "pdx.hpp"

static int g_checks = 0, g_failed = 0;
#define REQUIRE(cond)                                                              \
  do {                                                                             \
    ++g_checks;                                                                    \
    if (!(cond)) {                                                                 \
      ++g_failed;                                                                  \
      std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond);                \
    }                                                                              \
  } while (0)
#define REQUIRE_THROWS(expr)                                                       \
  do {                                                                             \
    ++g_checks;                                                                    \
    bool threw = false;                                                            \
    try { (void)(expr); } catch (const std::runtime_error&) { threw = true; }      \
    if (!threw) {                                                                  \
      ++g_failed;                                                                  \
      std::printf("FAILED %s:%d  expected std::runtime_error: %s\n", __FILE__, __LINE__, #expr); \
    }                                                                              \
  } while (0)
using namespace pd;
using Flags = std::vector<bool>;
using Ints = std::vector<int64_t>;
using Doubles = std::vector<double>;

static void test_series_mode() {
  // 3 holds three rows; 2 and 5 tie with two: the smaller one first
  Series s(Ints{5, 3, 2, 3, 5, 2, 3, 9});
  auto one = s.mode();
  REQUIRE(one.size() == 1);
  REQUIRE(one[0].mode == 3.0);
  REQUIRE(one[0].count == 3);
  auto three = s.mode(3);
  REQUIRE(three.size() == 3);
  REQUIRE(three[1].mode == 2.0 && three[1].count == 2);
  REQUIRE(three[2].mode == 5.0 && three[2].count == 2);
  REQUIRE(s.mode(100).size() == 4);  // n beyond the number of distinct values
  REQUIRE_THROWS(s.mode(0));
  REQUIRE_THROWS(s.mode(-1));
  // nulls take no part; skip_nulls = false with a null, and min_count above the valid rows, give an empty result
  Series holes(Ints{7, 7, 7, 1, 1}, Flags{false, false, true, true, true});
  auto h = holes.mode(2);
  REQUIRE(h.size() == 2);
  REQUIRE(h[0].mode == 1.0 && h[0].count == 2);
  REQUIRE(h[1].mode == 7.0 && h[1].count == 1);
  REQUIRE(holes.mode(1, false).empty());
  REQUIRE(holes.mode(1, true, 4).empty());
  REQUIRE(holes.mode(1, true, 3).size() == 1);
  REQUIRE(Series(Ints{}).mode().empty());
  // values spread over the 64-bit range (the sort path) and doubles
  Series wide(Ints{INT64_MIN, INT64_MAX, 0, INT64_MAX, INT64_MIN, 5});
  auto w = wide.mode(2);
  REQUIRE(w.size() == 2);
  REQUIRE(w[0].mode.as<int64_t>() == INT64_MIN && w[0].count == 2);
  REQUIRE(w[1].mode.as<int64_t>() == INT64_MAX && w[1].count == 2);
  Series d(Doubles{2.5, -1.5, 2.5, 1e300, -1.5, 2.5});
  auto dm = d.mode(2);
  REQUIRE(dm.size() == 2);
  REQUIRE(dm[0].mode == 2.5 && dm[0].count == 3);
  REQUIRE(dm[1].mode == -1.5 && dm[1].count == 2);
  // bool: false < true on a tie
  auto b = Series(Flags{true, false, false, true}).mode(2);
  REQUIRE(b.size() == 2);
  REQUIRE(b[0].mode.as<int64_t>() == 0 && b[0].count == 2);
  REQUIRE(b[1].mode.as<int64_t>() == 1 && b[1].count == 2);
}

static void test_value_counts_and_is_unique() {
  Series s(Ints{5, 3, 5, 5, 9, 3});
  DataFrame vc = s.value_counts();
  REQUIRE(vc.num_rows() == 3);
  REQUIRE((vc["values"].values<int64_t>() == Ints{5, 3, 9}));  // first-occurrence order
  REQUIRE((vc["counts"].values<int64_t>() == Ints{3, 2, 1}));
  REQUIRE(!s.is_unique());
  REQUIRE(Series(Ints{5, 3, 9}).is_unique());
  // a null is one entry, where the first null is; two nulls are not unique
  Series holes(Ints{4, 0, 4, 0, 6}, Flags{true, false, true, false, true});
  DataFrame hv = holes.value_counts();
  REQUIRE((hv["values"].m_array.valid_flags() == Flags{true, false, true}));
  REQUIRE((hv["counts"].values<int64_t>() == Ints{2, 2, 1}));
  REQUIRE(hv["values"].at(2) == 6.0);
  REQUIRE(!holes.is_unique());
  REQUIRE(Series(Ints{4, 0, 6}, Flags{true, false, true}).is_unique());
  // doubles: distinct bit patterns (0.0 and -0.0 are two entries)
  DataFrame dv = Series(Doubles{0.0, -0.0, 1.5, 0.0}).value_counts();
  REQUIRE(dv["values"].dtype() == PDX_FLOAT64);
  REQUIRE((dv["counts"].values<int64_t>() == Ints{2, 1, 1}));
  REQUIRE(std::signbit(dv["values"].values<double>()[1]));
  // bool
  DataFrame bv = Series(Flags{false, true, true, false, true}).value_counts();
  REQUIRE(bv["values"].dtype() == PDX_BOOL);
  REQUIRE((bv["values"].values<int64_t>() == Ints{0, 1}));
  REQUIRE((bv["counts"].values<int64_t>() == Ints{2, 3}));
  REQUIRE(Series(Ints{}).value_counts().num_rows() == 0);
  REQUIRE(Series(Ints{}).is_unique());
}

static void test_groupby_mode() {
  Flags vb{true, true, true, true, true, false, false};
  DataFrame df({"k", "a", "b"}, {Array::Make(Ints{1, 2, 1, 2, 1, 3, 3}), Array::Make(Ints{4, 8, 4, 6, 5, 7, 7}), Array::Make(Doubles{0.5, 2.5, 1.5, 2.5, 0.5, 9.0, 9.0}, &vb)});
  GroupBy gb = df.group_by("k");
  Series a = gb.mode("a");
  REQUIRE((a.values<int64_t>() == Ints{4, 6, 7}));  // group 2: 8 and 6 tie, the smaller one
  REQUIRE((a.m_index->values_as<int64_t>() == Ints{1, 2, 3}));
  REQUIRE(a.name() == "a");
  DataFrame both = gb.mode(std::vector<std::string>{"a", "b"});
  REQUIRE((both["b"].m_array.valid_flags() == Flags{true, true, false}));  // group 3 has no valid value of b
  REQUIRE(both["b"].m_array.null_count == 1);
  REQUIRE(both["b"].at(0) == 0.5);
  REQUIRE(both["b"].at(1) == 2.5);
  REQUIRE((both["a"].values<int64_t>() == Ints{4, 6, 7}));
  REQUIRE_THROWS(gb.mode("nope"));
}

int main() {
  ThrowOnFailure(pdx_init(0));
  try {
    test_series_mode();
    test_value_counts_and_is_unique();
    test_groupby_mode();
  } catch (const std::exception& e) {
    std::printf("FAILED with an exception: %s\n", e.what());
    return 2;
  }
  std::printf("test_facade_mode: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
