// test_facade_multisort.cpp -- DataFrame::argsort / sort_values through the C++ facade (pandasarrow_amd/cpp/pdx.hpp -> C ABI -> HIP kernels):
// Arrow C++ 25.0.0's sort_indices on hand-checked frames (stable, lexicographic; per key numbers < NaN < null in both orders; -0.0 == 0.0).
// Built with g++ (host code only) and run on the GPU box by tests/test_gpu_cpp_multisort.py.
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
#define REQUIRE_THROWS_WITH(expr, text)                                            \
  do {                                                                             \
    ++g_checks;                                                                    \
    bool threw = false;                                                            \
    try { (void)(expr); } catch (const std::runtime_error& e) { threw = std::string(e.what()).find(text) != std::string::npos; } \
    if (!threw) {                                                                  \
      ++g_failed;                                                                  \
      std::printf("FAILED %s:%d  expected std::runtime_error with '%s': %s\n", __FILE__, __LINE__, text, #expr); \
    }                                                                              \
  } while (0)
using namespace pd;
using Flags = std::vector<bool>;
using Rows = std::vector<uint64_t>;
using Names = std::vector<std::string>;

static void test_argsort() {
  const double nan = std::nan("");
  //                        row:   0    1     2    3    4    5
  const std::vector<double> a{0.0, nan, -0.0, 1.0, 5.0, 1.0};
  const Flags a_valid{true, true, true, true, false, true};  // row 4 is null, row 1 stays a NaN
  const std::vector<int64_t> b{2, 0, 1, 7, 0, 7};
  DataFrame df({"a", "b"}, {Array::Make(a, &a_valid), Array::Make(b)});
  Series asc = df.argsort(Names{"a", "b"}, true);
  REQUIRE(asc.dtype() == PDX_UINT64 && !asc.m_index && !asc.m_is_index);
  REQUIRE((asc.values<uint64_t>() == Rows{2, 0, 3, 5, 1, 4}));  // the zeros tie: b decides; the ones tie on b too: row order
  REQUIRE((df.argsort(Names{"a", "b"}, false).values<uint64_t>() == Rows{3, 5, 0, 2, 1, 4}));  // NaN and null stay behind
  REQUIRE((df.argsort(Names{"a", "b"}, Flags{false, true}).values<uint64_t>() == Rows{3, 5, 2, 0, 1, 4}));
  REQUIRE((df.argsort(Names{"a", "b"}, Flags{true, false}).values<uint64_t>() == Rows{0, 2, 3, 5, 1, 4}));
  REQUIRE((df.argsort(Names{"b", "a"}, true).values<uint64_t>() == Rows{1, 4, 2, 0, 3, 5}));
  REQUIRE((df.argsort(Names{"b"}, true).values<uint64_t>() == Rows{1, 4, 2, 0, 3, 5}));
  REQUIRE_THROWS_WITH(df.argsort(Names{"a", "zz"}, true), "zz not in schema");
  REQUIRE_THROWS_WITH(df.argsort(Names{}, true), "sort keys");
  REQUIRE_THROWS_WITH(df.argsort(Names{"a", "b"}, Flags{true}), "one sort order");
  // full-range keys: more bits than one 64-bit round holds
  const int64_t lo = INT64_MIN, hi = INT64_MAX;
  DataFrame wide({"x", "y"}, {Array::Make(std::vector<int64_t>{hi, lo, hi, lo, 0}), Array::Make(std::vector<int64_t>{lo, hi, hi, lo, 0})});
  REQUIRE((wide.argsort(Names{"x", "y"}, true).values<uint64_t>() == Rows{3, 1, 4, 0, 2}));
  REQUIRE((wide.argsort(Names{"x", "y"}, Flags{true, false}).values<uint64_t>() == Rows{1, 3, 4, 2, 0}));
}

static void test_sort_values() {
  DataFrame df({"sym", "t", "v"}, {Array::Make(std::vector<int64_t>{2, 1, 2, 1, 3}), Array::Make(std::vector<int64_t>{50, 40, 10, 40, 5}),
                                   Array::Make(std::vector<double>{0.5, 1.5, 2.5, 3.5, 4.5})},
               Array::Make(std::vector<int64_t>{100, 101, 102, 103, 104}));
  DataFrame s = df.sort_values(Names{"sym", "t"});
  REQUIRE((s["sym"].values<int64_t>() == std::vector<int64_t>{1, 1, 2, 2, 3}));
  REQUIRE((s["t"].values<int64_t>() == std::vector<int64_t>{40, 40, 10, 50, 5}));
  REQUIRE((s["v"].values<double>() == std::vector<double>{1.5, 3.5, 2.5, 0.5, 4.5}));  // the rows stay together
  REQUIRE(s.m_index && (s.m_index->values_as<int64_t>() == std::vector<int64_t>{101, 103, 102, 100, 104}));  // and so does the index
  DataFrame d = df.sort_values(Names{"sym", "t"}, Flags{false, true});
  REQUIRE(d.m_index && (d.m_index->values_as<int64_t>() == std::vector<int64_t>{104, 102, 100, 101, 103}));
  DataFrame plain({"sym", "t"}, {Array::Make(std::vector<int64_t>{2, 1, 2}), Array::Make(std::vector<int64_t>{5, 9, 4})});
  DataFrame p = plain.sort_values(Names{"sym", "t"}, false);
  REQUIRE((p["t"].values<int64_t>() == std::vector<int64_t>{5, 4, 9}));
  REQUIRE(p.m_index && (p.m_index->values_as<int64_t>() == std::vector<int64_t>{0, 2, 1}));  // the implicit index, taken along
  REQUIRE_THROWS_WITH(df.sort_values(Names{"nope"}), "nope not in schema");
  // 17 columns + the index: more than one pdx_take serves
  Names many;
  std::vector<Array> cols;
  for (int c = 0; c < 17; ++c) {
    many.push_back("c" + std::to_string(c));
    cols.push_back(Array::Make(std::vector<int64_t>{3 + c, 1 + c, 2 + c}));
  }
  DataFrame w = DataFrame(many, cols, Array::Make(std::vector<int64_t>{7, 8, 9})).sort_values(Names{"c16", "c0"});
  REQUIRE(w.num_columns() == 17 && (w["c0"].values<int64_t>() == std::vector<int64_t>{1, 2, 3}));
  REQUIRE((w["c16"].values<int64_t>() == std::vector<int64_t>{17, 18, 19}));
  REQUIRE(w.m_index && (w.m_index->values_as<int64_t>() == std::vector<int64_t>{8, 9, 7}));
}

int main() {
  ThrowOnFailure(pdx_init(0));
  test_argsort();
  test_sort_values();
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
