// test_facade_join.cpp -- merge / join through the C++ facade (pandasarrow_amd/cpp/pdx.hpp -> pdx_join_create, pdx_join_indices, pdx_take ->
// HIP kernels): DataFrame::merge with every `how`, suffixes, the single key column and its coalesce for "outer", 4-byte value columns,
// null cells and null keys (a null key matches nothing), DataFrame::join on int64 and timestamp indexes -- all on hand-checked cases.
// Built with g++ (host code only) and run on the GPU box by tests/test_gpu_cpp_join.py.
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
using Names = std::vector<std::string>;

static const int64_t kT0 = 1700000000000000000LL, kMinute = 60000000000LL;

static Ints ints(const DataFrame& f, const std::string& nm) { return f[nm].m_array.values_as<int64_t>(); }
static Doubles doubles(const DataFrame& f, const std::string& nm) { return f[nm].m_array.values_as<double>(); }
static Flags flags(const DataFrame& f, const std::string& nm) { return f[nm].m_array.valid_flags(); }
// the values with -1 at the null cells
static Ints cells(const DataFrame& f, const std::string& nm) {
  Ints v = ints(f, nm);
  const Flags ok = flags(f, nm);
  for (size_t i = 0; i < v.size(); ++i)
    if (!ok[i]) v[i] = -1;
  return v;
}

// left: k = 2, null, 1, 2 (a = 10, 11, 12, 13); right: k = 2, 1, 2, null, 3 (b = 20 .. 24; v clashes with the left's v)
static DataFrame left_frame() {
  const Flags kv{true, false, true, true};
  return DataFrame(Names{"k", "a", "v"}, {Array::Make(Ints{2, 0, 1, 2}, &kv), Array::Make(Ints{10, 11, 12, 13}), Array::Make(Doubles{0.5, 1.5, 2.5, 3.5})});
}
static DataFrame right_frame() {
  const Flags kv{true, true, true, false, true}, bv{true, true, false, true, true};
  return DataFrame(Names{"k", "b", "v"}, {Array::Make(Ints{2, 1, 2, 0, 3}, &kv), Array::Make(Ints{20, 21, 22, 23, 24}, &bv), Array::Make(Ints{7, 8, 9, 10, 11})});
}

static void test_merge_every_how() {
  const DataFrame l = left_frame(), r = right_frame();
  DataFrame in = l.merge(r, "k");
  REQUIRE((in.m_names == Names{"k", "a", "v_x", "b", "v_y"}) && !in.m_index);
  REQUIRE((ints(in, "k") == Ints{2, 2, 1, 2, 2}));
  REQUIRE((ints(in, "a") == Ints{10, 10, 12, 13, 13}));
  REQUIRE((cells(in, "b") == Ints{20, -1, 21, 20, -1}));  // (the right frame's null cell travels)
  REQUIRE((ints(in, "v_y") == Ints{7, 9, 8, 7, 9}));
  REQUIRE((doubles(in, "v_x") == Doubles{0.5, 0.5, 2.5, 3.5, 3.5}));

  DataFrame lf = l.merge(r, "k", "left");
  REQUIRE((ints(lf, "a") == Ints{10, 10, 11, 12, 13, 13}));
  REQUIRE((cells(lf, "k") == Ints{2, 2, -1, 1, 2, 2}));  // the null key keeps its row and matches nothing
  REQUIRE((cells(lf, "v_y") == Ints{7, 9, -1, 8, 7, 9}));

  DataFrame out = l.merge(r, "k", "outer");
  REQUIRE(out.num_rows() == 8);
  REQUIRE((cells(out, "k") == Ints{2, 2, -1, 1, 2, 2, -1, 3}));  // coalesce(left key, right key): the unmatched right key 3 shows
  REQUIRE((cells(out, "a") == Ints{10, 10, 11, 12, 13, 13, -1, -1}));
  REQUIRE((cells(out, "v_y") == Ints{7, 9, -1, 8, 7, 9, 10, 11}));

  DataFrame rt = l.merge(r, "k", "right");  // ordered by right row; the columns stay left-then-right
  REQUIRE((rt.m_names == Names{"k", "a", "v_x", "b", "v_y"}));
  REQUIRE((cells(rt, "k") == Ints{2, 2, 1, 2, 2, -1, 3}));
  REQUIRE((cells(rt, "a") == Ints{10, 13, 12, 10, 13, -1, -1}));
  REQUIRE((ints(rt, "v_y") == Ints{7, 7, 8, 9, 9, 10, 11}));

  DataFrame semi = l.merge(r, "k", "semi"), anti = l.merge(r, "k", "anti");
  REQUIRE((semi.m_names == Names{"k", "a", "v"}) && (ints(semi, "a") == Ints{10, 12, 13}));
  REQUIRE((ints(anti, "a") == Ints{11}) && (flags(anti, "k") == Flags{false}));
  REQUIRE_THROWS(l.merge(r, "k", "cross"));
  REQUIRE_THROWS(l.merge(r, "nope"));
}

static void test_left_on_right_on_and_suffixes() {
  const DataFrame l = left_frame();
  DataFrame r = right_frame();
  r.m_names = Names{"rk", "b", "v"};
  DataFrame m = l.merge(r, "k", "rk", "inner", {"_l", "_r"});
  REQUIRE((m.m_names == Names{"k", "a", "v_l", "rk", "b", "v_r"}));  // two key names: both columns stay
  REQUIRE((ints(m, "k") == ints(m, "rk")) && (ints(m, "v_r") == Ints{7, 9, 8, 7, 9}));
  // a suffix that collides with an existing name is refused
  DataFrame l2(Names{"k", "v", "v_y"}, {Array::Make(Ints{1}), Array::Make(Ints{2}), Array::Make(Ints{3})});
  DataFrame r2(Names{"k", "v"}, {Array::Make(Ints{1}), Array::Make(Ints{4})});
  REQUIRE_THROWS(l2.merge(r2, "k"));
  // a float key has no equality rule here; a dtype mismatch is refused
  REQUIRE_THROWS(l.merge(r, "v", "rk", "inner"));
  REQUIRE_THROWS(DataFrame(Names{"k"}, {Array::Make(Doubles{1.0})}).merge(DataFrame(Names{"k"}, {Array::Make(Doubles{1.0})}), "k"));
}

static void test_four_byte_values_and_empty_sides() {
  // int32 codes of dictionary_encode as a 4-byte VALUE column on the right
  Series codes = Series(Ints{70, 80, 70, 90}).dictionary_encode().first;
  REQUIRE(codes.dtype() == PDX_INT32);
  DataFrame l(Names{"k", "x"}, {Array::Make(Ints{3, 1, 0, 9}), Array::Make(Doubles{0.25, 0.5, 0.75, 1.0})});
  DataFrame r(Names{"k", "code"}, {Array::Make(Ints{0, 1, 2, 3}), codes.m_array});
  DataFrame m = l.merge(r, "k", "left");
  REQUIRE(m["code"].dtype() == PDX_INT32);
  REQUIRE((m["code"].values_i32() == std::vector<int32_t>{2, 1, 0, 0}));
  REQUIRE((flags(m, "code") == Flags{true, true, true, false}));
  // the int32 codes as KEYS on both sides
  DataFrame lc(Names{"c", "x"}, {codes.m_array, Array::Make(Ints{1, 2, 3, 4})});
  DataFrame rc(Names{"c", "y"}, {Series(Ints{80, 70, 60}).dictionary_encode().first.m_array, Array::Make(Ints{5, 6, 7})});  // codes 0, 1, 2
  DataFrame mc = lc.merge(rc, "c");
  REQUIRE((ints(mc, "x") == Ints{1, 2, 3, 4}) && (ints(mc, "y") == Ints{5, 6, 5, 7}));
  // empty sides
  DataFrame none(Names{"k", "code"}, {Array::Make(Ints{}), Array::Make(Ints{})});
  REQUIRE(l.merge(none, "k").num_rows() == 0);
  REQUIRE(l.merge(none, "k", "left").num_rows() == 4 && (flags(l.merge(none, "k", "left"), "code") == Flags{false, false, false, false}));
  REQUIRE(none.merge(l, "k", "outer").num_rows() == 4 && (cells(none.merge(l, "k", "outer"), "k") == Ints{3, 1, 0, 9}));
  REQUIRE(l.merge(none, "k", "anti").num_rows() == 4 && l.merge(none, "k", "semi").num_rows() == 0);
}

static void test_join_on_the_index() {
  // int64 labels
  DataFrame l(Names{"a"}, {Array::Make(Ints{1, 2, 3})}, Array::Make(Ints{10, 20, 30}));
  DataFrame r(Names{"b"}, {Array::Make(Ints{7, 8, 9})}, Array::Make(Ints{30, 10, 40}));
  DataFrame j = l.join(r);
  REQUIRE((j.m_names == Names{"a", "b"}) && (j.m_index->values_as<int64_t>() == Ints{10, 20, 30}));
  REQUIRE((cells(j, "b") == Ints{8, -1, 7}));
  DataFrame o = l.join(r, "outer");
  REQUIRE((o.m_index->values_as<int64_t>() == Ints{10, 20, 30, 40}) && o.m_index->null_count == 0);
  REQUIRE((cells(o, "a") == Ints{1, 2, 3, -1}) && (cells(o, "b") == Ints{8, -1, 7, 9}));
  REQUIRE((l.join(r, "inner").m_index->values_as<int64_t>() == Ints{10, 30}));
  DataFrame rj = l.join(r, "right");
  REQUIRE((rj.m_index->values_as<int64_t>() == Ints{30, 10, 40}) && (cells(rj, "a") == Ints{3, 1, -1}));
  REQUIRE((l.join(r, "anti").m_index->values_as<int64_t>() == Ints{20}));
  // timestamp labels
  DataFrame tl(Names{"a"}, {Array::Make(Ints{1, 2, 3, 4})}, date_range(kT0, 4));
  DataFrame tr(Names{"b"}, {Array::Make(Doubles{0.5, 1.5})}, date_range(kT0 + 2 * kMinute, 2));
  DataFrame tj = tl.join(tr);
  REQUIRE(tj.m_index->dtype == PDX_TIMESTAMP_NS && (tj.m_index->values_as<int64_t>() == Ints{kT0, kT0 + kMinute, kT0 + 2 * kMinute, kT0 + 3 * kMinute}));
  REQUIRE((flags(tj, "b") == Flags{false, false, true, true}) && doubles(tj, "b")[3] == 1.5);
  // frames without an index join on their row numbers; overlapping names are refused
  DataFrame p(Names{"a"}, {Array::Make(Ints{1, 2, 3})}), q(Names{"b"}, {Array::Make(Ints{4, 5})});
  REQUIRE((cells(p.join(q), "b") == Ints{4, 5, -1}));
  REQUIRE_THROWS(p.join(p));
}

int main() {
  ThrowOnFailure(pdx_init(0));
  try {
    test_merge_every_how();
    test_left_on_right_on_and_suffixes();
    test_four_byte_values_and_empty_sides();
    test_join_on_the_index();
  } catch (const std::exception& e) {
    std::printf("FAILED with an exception: %s\n", e.what());
    return 2;
  }
  std::printf("test_facade_join: %d checks, %d failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
