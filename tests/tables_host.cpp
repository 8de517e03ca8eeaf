// Host driver of the scenario family's table rules (cosim_amd/csrc/cosim_tables.h), built by tests/test_tables_host.py as plain C++
// (once more with -fsanitize=address,undefined): reads one raw table from stdin the way a setter of the C ABI is handed it, runs the
// setter's validator and prints the refusal, or packs the table, patches its pointers to a copy of the image and prints the derived
// values and every array as read back through its patched pointer.  Every array has exactly the size the caller gave it.
//   in:  kind | nq nv nu ngeom info_dim command_dim p_kp p_kd p_gmu p_floss | n_envs slots | tables (1; same_*: 2)
//        an int is a decimal; an array is its count (-1: a null pointer) and its words, floats as their int32 bits
//        scenario:               n_scn key_adr key_t key_cmd push_adr push_t push_v
//        params:                 n_scn adr t field index op value
//        checks, same_checks:    n_scn adr t signal index mode cmp bound
//        curves, same_curves:    n_scn adr t signal index lo hi bins
//   out: "ERR <message>"  |  "OK", then "val <name> <ints>" and "arr <name> <word offset> <n> <words>" lines and "words <n>"
//        same_*: "same 0|1", the in-place test of the second table over the first's image (0 too if the images differ in size)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "cosim_tables.h"

using namespace cosim;

static int rd() {
  int v = 0;
  if (scanf("%d", &v) != 1) exit(2);
  return v;
}

template <class T>
struct Arr {
  std::unique_ptr<T[]> p;
  int n = -1;
  const T* get() const { return n < 0 ? nullptr : p.get(); }
};
template <class T>
static Arr<T> rd_arr() {
  static_assert(sizeof(T) == 4, "words");
  Arr<T> a;
  a.n = rd();
  if (a.n < 0) return a;
  a.p.reset(new T[a.n]);
  for (int k = 0; k < a.n; k++) { const int32_t w = rd(); memcpy(&a.p[k], &w, 4); }
  return a;
}

static void val(const char* name, const std::vector<long long>& v) {
  printf("val %s", name);
  for (long long x : v) printf(" %lld", x);
  printf("\n");
}
template <class T>
static std::vector<long long> bits(const std::vector<T>& v) {
  std::vector<long long> o;
  for (const T& x : v) { int32_t w; memcpy(&w, &x, 4); o.push_back(w); }
  return o;
}

// the image at an address of its own, the table's pointers patched to it
struct Placed {
  std::unique_ptr<int32_t[]> dev;
  explicit Placed(const WordPacker& pk) : dev(new int32_t[pk.words()]) {
    memcpy(dev.get(), pk.data(), pk.bytes());
    pk.patch(dev.get());
  }
  template <class T>
  void arr(const char* name, const T* p, size_t n) const {
    printf("arr %s %lld %zu", name, (long long)(reinterpret_cast<const int32_t*>(p) - dev.get()), n);
    for (size_t k = 0; k < n; k++) { int32_t w; memcpy(&w, p + k, 4); printf(" %d", w); }
    printf("\n");
  }
};

static int refuse(const std::string& err) {
  printf("ERR %s\n", err.c_str());
  return 0;
}

struct Checks {
  Arr<int32_t> adr, t, signal, index, mode, cmp;
  Arr<float> bound;
  ChkRaw raw;
  Checks(int slots) {
    const int n_scn = rd();
    adr = rd_arr<int32_t>(); t = rd_arr<int32_t>(); signal = rd_arr<int32_t>(); index = rd_arr<int32_t>(); mode = rd_arr<int32_t>();
    cmp = rd_arr<int32_t>(); bound = rd_arr<float>();
    raw = {n_scn, adr.get(), t.get(), signal.get(), index.get(), mode.get(), cmp.get(), bound.get(), slots};
  }
};

struct Curves {
  Arr<int32_t> adr, t, signal, index, bins;
  Arr<float> lo, hi;
  CurRaw raw;
  Curves() {
    const int n_scn = rd();
    adr = rd_arr<int32_t>(); t = rd_arr<int32_t>(); signal = rd_arr<int32_t>(); index = rd_arr<int32_t>(); lo = rd_arr<float>();
    hi = rd_arr<float>(); bins = rd_arr<int32_t>();
    raw = {n_scn, adr.get(), t.get(), signal.get(), index.get(), lo.get(), hi.get(), bins.get()};
  }
};

int main() {
  char kind[32] = "";
  if (scanf("%31s", kind) != 1) return 2;
  const std::string k = kind;
  TableDims d;
  d.nq = rd(); d.nv = rd(); d.nu = rd(); d.ngeom = rd(); d.info_dim = rd(); d.command_dim = rd();
  d.p_kp = rd(); d.p_kd = rd(); d.p_gmu = rd(); d.p_floss = rd();
  const int n_envs = rd(), slots = rd();
  WordPacker pk;
  if (k == "scenario") {
    const int n_scn = rd();
    const Arr<int32_t> key_adr = rd_arr<int32_t>(), key_t = rd_arr<int32_t>();
    const Arr<float> key_cmd = rd_arr<float>();
    const Arr<int32_t> push_adr = rd_arr<int32_t>(), push_t = rd_arr<int32_t>();
    const Arr<float> push_v = rd_arr<float>();
    const ScnRaw raw = {n_scn, key_adr.get(), key_t.get(), key_cmd.get(), push_adr.get(), push_t.get(), push_v.get()};
    const ScnShape v = validate_scenario(d, raw);
    if (!v.err.empty()) return refuse(v.err);
    ScnTable tab = {};
    pack_scenario(pk, tab, d.command_dim, raw, v);
    const Placed at(pk);
    printf("OK\n");
    val("nkey", {v.nkey}); val("npush", {v.npush}); val("n_scn", {tab.n_scn}); val("cd", {tab.cd});
    at.arr("key_adr", tab.key_adr, (size_t)n_scn + 1); at.arr("push_adr", tab.push_adr, (size_t)n_scn + 1);
    at.arr("key_t", tab.key_t, v.nkey); at.arr("push_t", tab.push_t, 2 * (size_t)v.npush);
    at.arr("key_cmd", tab.key_cmd, (size_t)v.nkey * d.command_dim); at.arr("push_v", tab.push_v, 3 * (size_t)v.npush);
  } else if (k == "params") {
    const int n_scn = rd();
    const Arr<int32_t> adr = rd_arr<int32_t>(), t = rd_arr<int32_t>(), field = rd_arr<int32_t>(), index = rd_arr<int32_t>(), op = rd_arr<int32_t>();
    const Arr<float> value = rd_arr<float>();
    const ParRaw raw = {n_scn, adr.get(), t.get(), field.get(), index.get(), op.get(), value.get()};
    const ParShape v = validate_params(d, raw);
    if (!v.err.empty()) return refuse(v.err);
    ScnParTable tab = {};
    pack_params(pk, tab, raw, v);
    const Placed at(pk);
    printf("OK\n");
    val("n", {v.n}); val("word", bits(v.word)); val("n_scn", {tab.n_scn}); val("n_items", {tab.n_items});
    const size_t n = (size_t)v.n;
    at.arr("adr", tab.adr, (size_t)n_scn + 1); at.arr("t", tab.t, 2 * n); at.arr("word", tab.word, n); at.arr("op", tab.op, n);
    at.arr("value", tab.value, n);
  } else if (k == "checks") {
    const Checks c(slots);
    const ChkShape v = validate_checks(d, c.raw);
    if (!v.err.empty()) return refuse(v.err);
    ChkTable tab = {};
    pack_checks(pk, tab, c.raw, v);
    const Placed at(pk);
    printf("OK\n");
    val("n", {v.n}); val("I", {v.I}); val("n_scn", {tab.n_scn}); val("n_items", {tab.n_items}); val("tab_I", {tab.I});
    const size_t n = (size_t)v.n;
    at.arr("adr", tab.adr, (size_t)c.raw.n_scn + 1); at.arr("t", tab.t, 2 * n); at.arr("signal", tab.signal, n); at.arr("index", tab.index, n);
    at.arr("mode", tab.mode, n); at.arr("cmp", tab.cmp, n); at.arr("bound", tab.bound, n);
  } else if (k == "curves") {
    const Curves c;
    const CurShape v = validate_curves(d, n_envs, c.raw);
    if (!v.err.empty()) return refuse(v.err);
    CurTable tab = {};
    pack_curves(pk, tab, c.raw, v);
    const Placed at(pk);
    printf("OK\n");
    val("n", {v.n}); val("cells", {(long long)v.cells}); val("SW", {(long long)v.SW});
    val("n_scn", {tab.n_scn}); val("n_items", {tab.n_items}); val("tab_SW", {tab.SW});
    val("nt", bits(v.nt)); val("soff", bits(v.soff)); val("coff", bits(v.coff)); val("cw", bits(v.cw)); val("inv_w", bits(v.inv_w));
    const size_t n = (size_t)v.n;
    at.arr("adr", tab.adr, (size_t)c.raw.n_scn + 1); at.arr("t", tab.t, 3 * n); at.arr("signal", tab.signal, n); at.arr("index", tab.index, n);
    at.arr("bins", tab.bins, n); at.arr("nt", tab.nt, n); at.arr("soff", tab.soff, n); at.arr("coff", tab.coff, n); at.arr("cw", tab.cw, n);
    at.arr("lo", tab.lo, n); at.arr("hi", tab.hi, n); at.arr("inv_w", tab.inv_w, n);
  } else if (k == "same_checks") {
    const Checks a(slots), b(slots);
    const ChkShape va = validate_checks(d, a.raw), vb = validate_checks(d, b.raw);
    if (!va.err.empty() || !vb.err.empty()) return refuse(va.err + vb.err);
    ChkTable ta = {}, tb = {};
    WordPacker old;
    pack_checks(old, ta, a.raw, va);
    pack_checks(pk, tb, b.raw, vb);
    const bool sizes = tb.n_scn == ta.n_scn && tb.n_items == ta.n_items && tb.I == ta.I;   // what the setter holds against the engine's
    printf("same %d\n", (int)(sizes && pk.words() == old.words() && checks_same_rows(pk, tb, old.data())));
    return 0;
  } else if (k == "same_curves") {
    const Curves a, b;
    const CurShape va = validate_curves(d, n_envs, a.raw), vb = validate_curves(d, n_envs, b.raw);
    if (!va.err.empty() || !vb.err.empty()) return refuse(va.err + vb.err);
    CurTable ta = {}, tb = {};
    WordPacker old;
    pack_curves(old, ta, a.raw, va);
    pack_curves(pk, tb, b.raw, vb);
    const bool sizes = tb.n_scn == ta.n_scn && tb.n_items == ta.n_items && tb.SW == ta.SW && vb.cells == va.cells;
    printf("same %d\n", (int)(sizes && pk.words() == old.words() && curves_same_sizes(pk, tb, old.data())));
    return 0;
  } else {
    return 2;
  }
  printf("words %zu\n", pk.words());
  return 0;
}
