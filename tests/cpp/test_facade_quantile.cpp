// test_facade_quantile.cpp -- Series / DataFrame / GroupBy::quantile through the C++ facade (pandasarrow_amd/cpp/pdx.hpp -> C ABI -> HIP
// kernels): Arrow C++ 25.0.0's exact `quantile` on the corner values include/pdx/abi.h documents (tests/golden/quantile_golden.npz holds
// the same ones as pyarrow returned them).  Built with g++ (host code only) and run on the GPU box by tests/test_gpu_cpp_quantile.py.
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

static void test_series() {
  Series s(std::vector<int64_t>{4, 1, 3, 2});
  REQUIRE(s.quantile().s.dtype == PDX_FLOAT64 && s.quantile().as<double>() == 2.5);
  REQUIRE(s.quantile(0.5, Interpolation::LOWER).s.dtype == PDX_INT64 && s.quantile(0.5, Interpolation::LOWER).as<int64_t>() == 2);
  REQUIRE(s.quantile(0.5, Interpolation::HIGHER).as<int64_t>() == 3);
  REQUIRE(s.quantile(0.5, Interpolation::NEAREST).as<int64_t>() == 3);  // a tie goes to the even index
  REQUIRE(s.quantile(0.5, Interpolation::MIDPOINT).as<double>() == 2.5);
  REQUIRE(s.quantile(0.0).as<double>() == 1.0 && s.quantile(1.0).as<double>() == 4.0);
  auto many = s.quantiles({0.0, 0.25, 1.0});
  REQUIRE(many.size() == 3 && many[1].as<double>() == 1.75 && many[1].s.count == 4);
  Series big(std::vector<int64_t>{(int64_t)1 << 62, ((int64_t)1 << 62) + 1});
  REQUIRE(big.quantile().as<double>() == 4.611686018427388e+18);
  Series huge(std::vector<double>{1e308, 1.7e308});
  REQUIRE(huge.quantile(0.5, Interpolation::MIDPOINT).as<double>() == 1.35e308);  // halves first
  Series inf(std::vector<double>{1.0, HUGE_VAL});
  REQUIRE(inf.quantile(0.0).as<double>() == 1.0);  // f == 0 returns v[lo] alone
  Series gaps(Array::Make(std::vector<int64_t>{5, 0, 7}, nullptr), std::nullopt, "g");
  Flags valid{true, false, true};
  Series nulls(Array::Make(std::vector<int64_t>{5, 0, 7}, &valid));
  REQUIRE(nulls.quantile().as<double>() == 6.0 && nulls.quantile().s.count == 2);
  REQUIRE(!nulls.quantile(0.5, Interpolation::LINEAR, false).isValid());  // skip_nulls = false
  REQUIRE(!nulls.quantile(0.5, Interpolation::LINEAR, true, 3).isValid());  // min_count
  REQUIRE(gaps.quantile().as<double>() == 5.0);
  REQUIRE_THROWS(s.quantile(1.5));   // Quantile must be between 0 and 1
  REQUIRE_THROWS(s.quantiles({}));   // Requires quantile argument
  DataFrame df({"a", "b"}, {Array::Make(std::vector<int64_t>{1, 2, 3, 4, 5}), Array::Make(std::vector<double>{4, 5, 6, 7, 8})});
  auto r = df.quantile(0.5);
  REQUIRE(r.size() == 2 && r["a"].as<double>() == 3.0 && r["b"].as<double>() == 6.0);
}

static void test_groups() {
  DataFrame df({"k", "v", "w"}, {Array::Make(std::vector<int64_t>{7, 3, 7, 3, 7, 9}), Array::Make(std::vector<double>{4.0, 10.0, 1.0, 20.0, 2.0, 5.5}),
                                 Array::Make(std::vector<int64_t>{40, 100, 10, 200, 20, 55})});
  GroupBy g = df.group_by("k");
  Series m = g.quantile("v", 0.5);
  REQUIRE((m.values<double>() == std::vector<double>{2.0, 15.0, 5.5}));  // groups 7, 3, 9 in first-occurrence order
  REQUIRE(m.name() == "v" && m.m_index && (m.m_index->values_as<int64_t>() == std::vector<int64_t>{7, 3, 9}));
  DataFrame f = g.quantile({"v", "w"}, {1.0, 0.5}, Interpolation::LOWER);
  REQUIRE((f["v"].values<double>() == std::vector<double>{4.0, 20.0, 5.5}));
  REQUIRE((f["w"].values<int64_t>() == std::vector<int64_t>{20, 100, 55}));
  Series few = g.quantile("v", 0.5, Interpolation::LINEAR, true, 2);  // min_count = 2: the single-row group is null
  REQUIRE((few.m_array.valid_flags() == Flags{true, true, false}) && few.m_array.null_count == 1);
  REQUIRE_THROWS(g.quantile({"v", "w"}, {0.5}));
  REQUIRE_THROWS(g.quantile("v", -0.5));
}

int main() {
  ThrowOnFailure(pdx_init(0));
  test_series();
  test_groups();
  std::printf("%d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
