// Host driver of the owning buffer (cosim_amd/csrc/cosim_devbuf.h), built by tests/test_devbuf_host.py as plain C++ (once more with
// -fsanitize=address,undefined): DevBuf over an allocator on std::malloc that counts its live blocks, refuses a free of a block it
// does not hold and fails the k-th request on command.  argv[1] names the case; "ok <case>" and exit status 0, or the line that failed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <utility>

#include "cosim_devbuf.h"

using namespace cosim;

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

struct Fake {
  using error_t = int;
  static constexpr error_t ok = 0;
  static std::set<void*> live;
  static int requests, fail_at, frees;   // fail_at k: the k-th request from now fails (0: none)
  static error_t malloc(void** p, size_t bytes) {
    requests++;
    if (fail_at > 0 && --fail_at == 0) { *p = nullptr; return 2; }
    *p = std::malloc(bytes);
    memset(*p, 0xa5, bytes);   // never zero by chance
    live.insert(*p);
    return ok;
  }
  static void free(void* p) {
    CHECK(live.erase(p) == 1);   // a block that is live, once
    frees++;
    std::free(p);
  }
  static error_t memset(void* p, int v, size_t bytes) { ::memset(p, v, bytes); return ok; }
  static error_t to_device(void* dst, const void* host, size_t bytes) { memcpy(dst, host, bytes); return ok; }
  static error_t to_host(void* host, const void* src, size_t bytes) { memcpy(host, src, bytes); return ok; }
};
std::set<void*> Fake::live;
int Fake::requests = 0, Fake::fail_at = 0, Fake::frees = 0;
using Buf = DevBuf<int, Fake>;
static int live() { return (int)Fake::live.size(); }

// five buffers that only mean something together, as a feature of the engine holds them
struct Group {
  Buf a, b, c, d, e;
  int slots = 0;
  const int* ptr(int i) const { const Buf* all[5] = {&a, &b, &c, &d, &e}; return all[i]->get(); }
};
static int fill(Group& g, int slots) {   // the shape of a setter: the first error returns, the destructors undo the rest
  int r;
  if ((r = g.a.alloc(3)) || (r = g.b.alloc_zeroed(5)) || (r = g.c.alloc(7)) || (r = g.d.alloc_zeroed(2)) || (r = g.e.alloc(1))) return r;
  g.slots = slots;
  return 0;
}

static void empty_object() {
  { Buf b; CHECK(!b && b.get() == nullptr && b.size() == 0); }
  CHECK(Fake::frees == 0 && Fake::requests == 0 && live() == 0);
  Buf z;
  CHECK(z.alloc(0) == 0 && !z && Fake::requests == 0);   // no block of no bytes
}

static void alloc_destruct() {
  {
    Buf b;
    CHECK(b.alloc(10) == 0 && b && b.size() == 10 && live() == 1);
    b.get()[9] = 7;
  }
  CHECK(live() == 0 && Fake::frees == 1);
}

static void zeroed() {
  Buf b;
  CHECK(b.alloc_zeroed(33) == 0 && b.size() == 33);
  for (int i = 0; i < 33; i++) CHECK(b.get()[i] == 0);
  int host[4] = {4, 3, 2, 1}, back[4] = {0, 0, 0, 0};
  CHECK(b.upload(host, 4) == 0 && b.size() == 4 && live() == 1 && Fake::frees == 1);   // a fresh block: the old one went
  CHECK(b.download(back, 4) == 0 && !memcmp(host, back, sizeof host));
}

static void moves() {
  Buf src;
  CHECK(src.alloc(4) == 0);
  int* const p = src.get();
  Buf made(std::move(src));
  CHECK(!src && src.size() == 0 && made.get() == p && made.size() == 4 && live() == 1 && Fake::frees == 0);
  Buf dst;
  CHECK(dst.alloc(6) == 0 && live() == 2);
  int* const old = dst.get();
  dst = std::move(made);
  CHECK(!made && dst.get() == p && dst.size() == 4 && live() == 1 && Fake::frees == 1 && !Fake::live.count(old));   // the destination's block went, once
  dst = Buf();   // an empty source drops
  CHECK(!dst && live() == 0 && Fake::frees == 2);
}

static void self_move() {
  Buf b;
  CHECK(b.alloc(4) == 0);
  int* const p = b.get();
  Buf& alias = b;
  b = std::move(alias);
  CHECK(b.get() == p && b.size() == 4 && live() == 1 && Fake::frees == 0);
}

static void reset_twice() {
  Buf b;
  CHECK(b.alloc(4) == 0);
  b.reset();
  CHECK(!b && b.size() == 0 && live() == 0 && Fake::frees == 1);
  b.reset();
  CHECK(!b && Fake::frees == 1);
}

static void failed_alloc() {
  Buf b;
  CHECK(b.alloc(4) == 0 && live() == 1);
  Fake::fail_at = 1;
  CHECK(b.alloc(8) == 2 && !b && b.get() == nullptr && b.size() == 0 && live() == 0 && Fake::frees == 1);   // empty, never dangling
  Fake::fail_at = 1;
  CHECK(b.alloc_zeroed(8) == 2 && !b && live() == 0);
  Fake::fail_at = 1;
  int host[2] = {1, 2};
  CHECK(b.upload(host, 2) == 2 && !b && live() == 0);
  CHECK(b.alloc(2) == 0 && b && live() == 1);   // and usable again
}

// fill a local group, return on an error, move-assign into the target.  drop_first: the target is emptied ahead of the fill
static void set_group(bool drop_first) {
  Group target;
  CHECK(fill(target, 1) == 0 && live() == 5);
  for (int k = 1; k <= 6; k++) {   // the k-th request fails; k = 6: none does
    const int* before[5];
    for (int i = 0; i < 5; i++) before[i] = target.ptr(i);
    const int held = live();
    Fake::fail_at = k <= 5 ? k : 0;
    int rc;
    {
      if (drop_first) target = Group();
      Group fresh;
      rc = fill(fresh, 2);
      if (rc == 0) target = std::move(fresh);
    }
    Fake::fail_at = 0;
    if (k <= 5) {
      CHECK(rc == 2);
      if (drop_first) {   // nothing of the kind is set, nothing is live
        CHECK(live() == 0 && target.slots == 0);
        for (int i = 0; i < 5; i++) CHECK(target.ptr(i) == nullptr);
        CHECK(fill(target, 1) == 0);   // (set again for the next round)
      } else {            // what was set stays, pointer for pointer
        CHECK(live() == held && target.slots == 1);
        for (int i = 0; i < 5; i++) CHECK(target.ptr(i) == before[i] && Fake::live.count((void*)before[i]));
      }
    } else {
      CHECK(rc == 0 && live() == 5 && target.slots == 2);
      for (int i = 0; i < 5; i++) {
        CHECK(target.ptr(i) != nullptr && Fake::live.count((void*)target.ptr(i)));
        if (!drop_first) CHECK(target.ptr(i) != before[i] && !Fake::live.count((void*)before[i]));   // old and new stood side by side: other blocks, and the old ones are gone
      }
    }
  }
  target = Group();
  CHECK(live() == 0);
}

int main(int argc, char** argv) {
  const std::string c = argc > 1 ? argv[1] : "";
  if (c == "empty") empty_object();
  else if (c == "alloc_destruct") alloc_destruct();
  else if (c == "zeroed") zeroed();
  else if (c == "moves") moves();
  else if (c == "self_move") self_move();
  else if (c == "reset_twice") reset_twice();
  else if (c == "failed_alloc") failed_alloc();
  else if (c == "build_then_commit") set_group(false);
  else if (c == "drop_first") set_group(true);
  else { printf("unknown case %s\n", c.c_str()); return 2; }
  CHECK(live() == 0);   // every case ends with nothing live
  printf("ok %s\n", c.c_str());
  return 0;
}
