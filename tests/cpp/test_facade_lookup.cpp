// test_facade_lookup.cpp -- the lookup calls through the C++ facade (pandasarrow_amd/cpp/pdx.hpp -> pdx_is_in, pdx_index_in, pdx_index,
// pdx_arg_extreme, pdx_dictionary_encode -> HIP kernels): Series::is_in / index_in / index / argmin / argmax / idxMin / idxMax /
// dictionary_encode / unique and DataFrame::idxMin / idxMax on hand-checked cases (Arrow 25's rules: values match by bit pattern, the first
// position in the value set, the first row of an extreme).  Built with g++ (host code only) and run on the GPU box by
// tests/test_gpu_cpp_lookup.py.
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

static uint64_t bits_of(double x) {
  uint64_t b;
  std::memcpy(&b, &x, 8);
  return b;
}
static double from_bits(uint64_t b) {
  double x;
  std::memcpy(&x, &b, 8);
  return x;
}

static void test_idx_min_max() {
  // a timestamp index: the label at the first row of the extreme
  Series s(Array::Make(Doubles{3.5, -1.0, 7.0, -1.0, 7.0}), date_range(kT0, 5), "v");
  REQUIRE(s.argmin() == 1 && s.argmax() == 2);
  REQUIRE(s.idxMin().as<int64_t>() == kT0 + kMinute);
  REQUIRE(s.idxMax().as<int64_t>() == kT0 + 2 * kMinute);
  REQUIRE(s.index(Scalar(7.0)) == 2 && s.index(Scalar(8.0)) == -1 && s.index(Scalar()) == -1);
  // nulls take no part; without an index the label is the row
  Series holes(Ints{1, 9, 4, 9}, Flags{false, true, true, false});
  REQUIRE(holes.argmin() == 2 && holes.argmax() == 1);
  REQUIRE(holes.idxMin().as<int64_t>() == 2);
  REQUIRE(holes.index(Scalar((int64_t)9)) == 1 && holes.index(Scalar((int64_t)1)) == -1);
  // zeros of both signs tie: the first row
  Series z(Doubles{2.0, -0.0, 0.0, 2.0});
  REQUIRE(z.argmin() == 1 && z.index(Scalar(0.0)) == 1);
  // an all-null Series has no extreme: idxMin throws as GetScalar(-1) does
  Series nothing(Ints{1, 2}, Flags{false, false});
  REQUIRE(nothing.argmin() == -1 && nothing.argmax() == -1);
  REQUIRE_THROWS(nothing.idxMin());
  REQUIRE_THROWS(nothing.idxMax());
  REQUIRE(Series(Ints{}).argmin() == -1);
}

static void test_frame_idx_min() {
  DataFrame df({"a", "b"}, {Array::Make(Ints{5, 1, 9, 1}), Array::Make(Doubles{2.5, 8.0, -1.0, 8.0})}, date_range(kT0, 4));
  auto lo = df.idxMin(), hi = df.idxMax();
  REQUIRE(lo["a"].as<int64_t>() == kT0 + kMinute && lo["b"].as<int64_t>() == kT0 + 2 * kMinute);
  REQUIRE(hi["a"].as<int64_t>() == kT0 + 2 * kMinute && hi["b"].as<int64_t>() == kT0 + kMinute);
  Flags none{false, false, false, false};
  DataFrame bad({"a", "n"}, {Array::Make(Ints{5, 1, 9, 1}), Array::Make(Ints{0, 0, 0, 0}, &none)});
  REQUIRE_THROWS(bad.idxMin());
}

static void test_is_in_as_a_filter() {
  DataFrame df({"id", "x"}, {Array::Make(Ints{10, 20, 30, 20, 40}), Array::Make(Doubles{0.5, 1.5, 2.5, 3.5, 4.5})}, date_range(kT0, 5));
  Series ids = df["id"];
  Series mask = ids.is_in(Series(Ints{20, 40, 99, 20}));
  REQUIRE(mask.dtype() == PDX_BOOL && mask.m_array.null_count == 0);
  REQUIRE((mask.values<int64_t>() == Ints{0, 1, 0, 1, 1}));
  REQUIRE(mask.m_index && mask.m_index->length == 5);  // the result keeps the index
  DataFrame kept = df[mask];
  REQUIRE(kept.num_rows() == 3);
  REQUIRE((kept["id"].values<int64_t>() == Ints{20, 20, 40}));
  REQUIRE((kept["x"].values<double>() == Doubles{1.5, 3.5, 4.5}));
  // index_in: the first position in the set, null without a match; a null row finds the set's null unless skip_nulls
  Series in(Ints{20, 7, 40, 0}, Flags{true, true, true, false});
  Series set(Ints{40, 0, 20, 40}, Flags{true, false, true, true});
  Series pos = in.index_in(set);
  REQUIRE(pos.dtype() == PDX_INT32);
  REQUIRE((pos.values_i32() == std::vector<int32_t>{2, 0, 0, 1}));
  REQUIRE((pos.m_array.valid_flags() == Flags{true, false, true, true}));
  REQUIRE((in.index_in(set, true).m_array.valid_flags() == Flags{true, false, true, false}));
  REQUIRE((in.is_in(set).values<int64_t>() == Ints{1, 0, 1, 1}));
  REQUIRE((in.is_in(set, true).values<int64_t>() == Ints{1, 0, 1, 0}));
  // doubles match by bit pattern; an int64 set is cast (exactly) for a float64 Series
  Series d(Doubles{0.0, -0.0, 5.0}, Flags{true, true, true});
  REQUIRE((d.is_in(Series(Doubles{-0.0}, Flags{true})).values<int64_t>() == Ints{0, 1, 0}));
  REQUIRE((d.is_in(Series(Ints{5, 0})).values<int64_t>() == Ints{1, 0, 1}));
  REQUIRE_THROWS(Series(Ints{1}).is_in(Series(Doubles{1.0})));
  REQUIRE((Series(Ints{1, 2}).is_in(Series(Ints{})).values<int64_t>() == Ints{0, 0}));
}

static void test_unique_and_dictionary_encode() {
  // 0.0 and -0.0 are two values, and so are two NaNs of different payload
  const double nan1 = from_bits(0x7ff8000000000000ull), nan2 = from_bits(0x7ff8000000000005ull);
  Doubles v{1.0, nan1, nan2, 0.0, -0.0, 0.0, 5.0, nan2};
  Series s(v, Flags(v.size(), true));
  Series u = s.unique();
  REQUIRE(u.dtype() == PDX_FLOAT64 && u.size() == 6);
  const Doubles uv = u.values<double>();
  const std::vector<uint64_t> want{bits_of(1.0), bits_of(nan1), bits_of(nan2), bits_of(0.0), bits_of(-0.0), bits_of(5.0)};
  for (size_t i = 0; i < want.size() && i < uv.size(); ++i) REQUIRE(bits_of(uv[i]) == want[i]);
  REQUIRE(s.nunique() == 6);
  auto enc = s.dictionary_encode();
  REQUIRE((enc.first.values_i32() == std::vector<int32_t>{0, 1, 2, 3, 4, 3, 5, 2}));
  REQUIRE(enc.second.size() == 6);
  const Doubles dv = enc.second.values<double>();
  for (size_t i = 0; i < want.size() && i < dv.size(); ++i) REQUIRE(bits_of(dv[i]) == want[i]);
  // a null row gets a null code and takes no dictionary slot; the codes keep the index
  Flags ok{true, true, false, true, true};
  Series holes(Array::Make(Ints{7, 8, 0, 7, 9}, &ok), date_range(kT0, 5));
  auto he = holes.dictionary_encode();
  REQUIRE((he.first.values_i32() == std::vector<int32_t>{0, 1, 0, 0, 2}));
  REQUIRE((he.first.m_array.valid_flags() == ok) && he.first.m_array.null_count == 1);
  REQUIRE(he.first.m_index && he.first.m_index->length == 5);
  REQUIRE((he.second.values<int64_t>() == Ints{7, 8, 9}));
  // bool unique: at most three entries, the null in its place; the integer path is unchanged
  Series b(Flags{true, false, true, true}, Flags{true, true, false, true});
  REQUIRE(b.unique().size() == 3 && b.nunique() == 2);
  REQUIRE((Series(Ints{4, 4, 2}).unique().values<int64_t>() == Ints{4, 2}));
}

int main() {
  ThrowOnFailure(pdx_init(0));
  try {
    test_idx_min_max();
    test_frame_idx_min();
    test_is_in_as_a_filter();
    test_unique_and_dictionary_encode();
  } catch (const std::exception& e) {
    std::printf("FAILED with an exception: %s\n", e.what());
    return 2;
  }
  std::printf("test_facade_lookup: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
