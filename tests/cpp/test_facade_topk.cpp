// test_facade_topk.cpp -- top-k and partition through the C++ facade (pandasarrow_amd/cpp/pdx.hpp -> pdx_select_k, pdx_partition_nth -> HIP
// kernels): Series::n_largest / n_smallest / nth_element on hand-checked cases (Arrow 25's array_sort_indices rules: stable in both orders,
// -0.0 == 0.0, NaN behind the numbers, nulls last; nth_element in pdx_partition_nth's deterministic layout).  Built with g++ (host code only)
// and run on the GPU box by tests/test_gpu_cpp_topk.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static const int64_t kT0 = 1700000000000000000LL, kMinute = 60000000000LL;

static std::string plan() {
  char buf[256];
  ThrowOnFailure(pdx_select_k_last_plan(buf, sizeof(buf)));
  return buf;
}

static void test_top_of_a_small_series() {
  // ties keep their row order in BOTH orders; the index travels with the values
  Series s(Array::Make(Ints{5, 9, 1, 9, 5, 1, 7}), date_range(kT0, 7), "v");
  Series top = s.n_largest(3);
  REQUIRE(top.size() == 3 && top.m_name == "v");
  REQUIRE((top.values<int64_t>() == Ints{9, 9, 7}));
  REQUIRE((top.m_index->values_as<int64_t>() == Ints{kT0 + kMinute, kT0 + 3 * kMinute, kT0 + 6 * kMinute}));
  REQUIRE(plan().rfind("plan=", 0) == 0 && plan().find(" k=3 rows=7 ") != std::string::npos);
  Series low = s.n_smallest(4);
  REQUIRE((low.values<int64_t>() == Ints{1, 1, 5, 5}));
  REQUIRE((low.m_index->values_as<int64_t>() == Ints{kT0 + 2 * kMinute, kT0 + 5 * kMinute, kT0, kT0 + 4 * kMinute}));
  // the same rows as sort(order).head(n), and all of them when the Series is shorter than n
  for (int n : {0, 1, 6, 7, 12}) {
    REQUIRE((s.n_largest(n).values<int64_t>() == s.sort(false).head(n).values<int64_t>()));
    REQUIRE((s.n_smallest(n).values<int64_t>() == s.sort(true).head(n).values<int64_t>()));
    REQUIRE(s.n_smallest(n).size() == std::min<int64_t>(n, 7));
  }
  REQUIRE(plan().find("plan=sort") == 0);  // (12 rows asked of 7)
  // without an index the labels are the rows
  Series bare(Ints{5, 9, 1, 9});
  REQUIRE((bare.n_largest(2).m_index->values_as<int64_t>() == Ints{1, 3}));
  REQUIRE_THROWS(bare.n_largest(-1));
  REQUIRE(Series(Ints{}).n_largest(3).size() == 0);
}

static void test_zeros_nan_and_nulls() {
  // -0.0 == 0.0 (row order decides); a null row comes last in both orders
  Series z(Doubles{0.0, -0.0, 2.0, -0.0, -1.0, 0.0}, Flags{true, true, true, true, true, false});
  REQUIRE((z.n_smallest(3).m_index->values_as<int64_t>() == Ints{4, 0, 1}));
  REQUIRE((z.n_largest(4).m_index->values_as<int64_t>() == Ints{2, 0, 1, 3}));
  Series all = z.n_largest(6);
  REQUIRE((all.m_index->values_as<int64_t>() == Ints{2, 0, 1, 3, 4, 5}));
  REQUIRE((all.m_array.valid_flags() == Flags{true, true, true, true, true, false}));
  // more rows asked than there are numbers: the null rows follow in row order
  Series holes(Ints{4, 8, 6, 2, 9}, Flags{false, true, true, false, true});
  REQUIRE((holes.n_smallest(4).m_index->values_as<int64_t>() == Ints{2, 1, 4, 0}));
  REQUIRE((holes.n_largest(5).m_index->values_as<int64_t>() == Ints{4, 1, 2, 0, 3}));
}

static void test_nth_element() {
  Series s(Array::Make(Ints{5, 1, 4, 1, 9, 3}), date_range(kT0, 6), "v");
  // rank 2 of {1, 1, 3, 4, 5, 9} is 3: smaller rows, the equal row, larger rows, each in row order
  Series r = s.nth_element(2);
  REQUIRE(r.dtype() == PDX_UINT64 && r.size() == 6 && r.m_index && r.m_index->length == 6);
  REQUIRE((r.values<int64_t>() == Ints{1, 3, 5, 0, 2, 4}));
  REQUIRE((s.nth_element().values<int64_t>() == Ints{1, 3, 0, 2, 4, 5}));  // n = 0: the smallest value leads, its ties with it
  REQUIRE((s.nth_element(6).values<int64_t>() == Ints{0, 1, 2, 3, 5, 4}));  // n = size(): the largest value is the threshold
  REQUIRE_THROWS(s.nth_element(7));
  REQUIRE_THROWS(s.nth_element(-1));
  Series holes(Doubles{2.5, 0.0, 7.0, -0.0, 1.0}, Flags{true, true, false, true, true});
  REQUIRE((holes.nth_element(1).values<int64_t>() == Ints{1, 3, 0, 4, 2}));  // both zeros are the threshold; the null row is last
  REQUIRE(Series(Ints{}).nth_element().size() == 0);
}

static void test_four_byte_values() {
  // int32 codes of dictionary_encode: a 4-byte Series the 8-byte-only argsort refuses
  Series codes = Series(Ints{70, 80, 70, 90, 80, 60}).dictionary_encode().first;
  REQUIRE(codes.dtype() == PDX_INT32);
  REQUIRE((codes.values_i32() == std::vector<int32_t>{0, 1, 0, 2, 1, 3}));
  REQUIRE_THROWS(codes.argsort());
  Series top = codes.n_largest(3);
  REQUIRE(top.dtype() == PDX_INT32);
  REQUIRE((top.values_i32() == std::vector<int32_t>{3, 2, 1}));
  REQUIRE((top.m_index->values_as<int64_t>() == Ints{5, 3, 1}));
  REQUIRE((codes.n_smallest(3).m_index->values_as<int64_t>() == Ints{0, 2, 1}));
  REQUIRE((codes.nth_element(3).values<int64_t>() == Ints{0, 2, 1, 4, 3, 5}));
}

int main() {
  ThrowOnFailure(pdx_init(0));
  try {
    test_top_of_a_small_series();
    test_zeros_nan_and_nulls();
    test_nth_element();
    test_four_byte_values();
  } catch (const std::exception& e) {
    std::printf("FAILED with an exception: %s\n", e.what());
    return 2;
  }
  std::printf("test_facade_topk: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
