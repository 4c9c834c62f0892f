// csrc/devbuf.hpp on its own, on the CPU: DevBufT over host memory with an allocator that counts, logs the order of its
// calls, refuses a free of anything it does not hold and can be told to fail its N-th allocation.  Checks that every
// owned block is freed exactly once, that views free nothing, what a move leaves behind, ensure's grow-only rule and the
// order sync -> free -> alloc of a re-allocation, that keep = true carries the old bytes over, that a view is never
// re-sized, and that with any one allocation of a call sequence failing (the replace-two-buffers pattern of
// gpso_vgp_extend_q and a re-carved arena among them) nothing stays allocated once the buffers are gone.
// Exits 0 when every check holds (tests/test_tools_cpu.py builds it with -Wall -Wextra -Werror and runs it).
// By hand, under the sanitizers:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/devbuf_check.cpp -o devbuf_check
//     ./devbuf_check
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "../pygpso_amd/csrc/devbuf.hpp"

using namespace gpso;

static int failures = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);       \
      ++failures;                                                   \
    }                                                               \
  } while (0)

struct HostAlloc {
  using Stream = int;
  static inline std::map<void*, size_t> live;  // blocks handed out and not yet freed
  static inline size_t live_bytes = 0;
  static inline int allocs = 0, frees = 0, bad_frees = 0, fail_at = 0;  // fail_at: this allocation fails (1-based; 0: none)
  static inline std::string log;  // a(lloc) f(ree) c(opy) s(ync), in call order
  static void reset(int fail) {
    CHECK(live.empty() && live_bytes == 0);
    allocs = frees = bad_frees = 0;
    fail_at = fail;
    log.clear();
  }
  static int alloc(void** p, size_t bytes) {
    log += 'a';
    if (++allocs == fail_at) return 2;
    *p = std::malloc(bytes);
    std::memset(*p, 0xee, bytes);
    live[*p] = bytes;
    live_bytes += bytes;
    return 0;
  }
  static int free(void* p, size_t bytes) {
    log += 'f';
    auto it = live.find(p);
    if (it == live.end() || it->second != bytes) {  // not ours, freed before, or another size than it was made with
      ++bad_frees;
      return 1;
    }
    live.erase(it);
    live_bytes -= bytes;
    ++frees;
    std::free(p);
    return 0;
  }
  static int copy(void* dst, const void* src, size_t bytes, Stream) {
    log += 'c';
    std::memcpy(dst, src, bytes);
    return 0;
  }
  static int sync(Stream) {
    log += 's';
    return 0;
  }
};
using Buf = DevBufT<HostAlloc>;
using H = HostAlloc;

static void ownership() {
  H::reset(0);
  {
    Buf a, b;
    CHECK(a.p == nullptr && a.bytes == 0 && !a.view);
    CHECK(!a.ensure(100, 0) && a.p != nullptr && a.bytes == 100 && !a.view && H::live_bytes == 100);
    CHECK(!b.ensure(0, 0) && b.bytes == 16);  // the 16-byte minimum
    void* const pa = a.p;
    // below or at the current size: nothing is allocated, freed or waited for
    const std::string before = H::log;
    CHECK(!a.ensure(100, 0) && !a.ensure(7, 0) && !a.ensure(0, 0) && !a.ensure(64, 0, true));
    CHECK(a.p == pa && a.bytes == 100 && H::log == before);
    // above it: the stream is synchronised, THEN the old block freed, then the new one made; exactly the new size is held
    H::log.clear();
    CHECK(!a.ensure(300, 0) && a.bytes == 300 && H::log == "sfa" && H::live_bytes == 300 + 16);
    // a move leaves the source empty and frees what the target held
    Buf c(std::move(a));
    CHECK(a.p == nullptr && a.bytes == 0 && !a.view && c.bytes == 300 && H::frees == 1);
    b = std::move(c);
    CHECK(c.p == nullptr && c.bytes == 0 && b.bytes == 300 && H::frees == 2 && H::live_bytes == 300);
    Buf& self = b;
    b = std::move(self);
    CHECK(b.bytes == 300 && H::frees == 2);
    // drop: back to empty, once
    b.drop();
    CHECK(b.p == nullptr && b.bytes == 0 && H::frees == 3 && H::live_bytes == 0);
    b.drop();
    CHECK(H::frees == 3);
    CHECK(!b.ensure(40, 0));  // (an emptied buffer allocates without a sync: nothing can be reading it)
    CHECK(H::log.substr(H::log.size() - 2) == "fa" && H::live_bytes == 40);
  }
  CHECK(H::live_bytes == 0 && H::bad_frees == 0 && H::frees == H::allocs);
}

static void keep_carries_the_old_bytes() {
  H::reset(0);
  {
    Buf a;
    CHECK(!a.ensure(64, 0, true) && H::log == "a");
    for (int k = 0; k < 64; ++k) static_cast<unsigned char*>(a.p)[k] = (unsigned char)(3 * k + 1);
    H::log.clear();
    // the new block exists before the old one goes: alloc, copy, sync, free
    CHECK(!a.ensure(4096, 0, true) && a.bytes == 4096 && H::log == "acsf" && H::live_bytes == 4096);
    for (int k = 0; k < 64; ++k) CHECK(static_cast<unsigned char*>(a.p)[k] == (unsigned char)(3 * k + 1));
  }
  CHECK(H::live_bytes == 0 && H::bad_frees == 0 && H::frees == 2);
}

static void views() {
  H::reset(0);
  {
    Buf arena, v0, v1, none;
    CHECK(!arena.ensure(1024, 0));
    v0.slice(arena, 0, 256);
    v1.slice(arena, 256, 768);
    none.slice(arena, 1024, 0);
    CHECK(v0.p == arena.p && v0.bytes == 256 && v0.view && v1.p == static_cast<char*>(arena.p) + 256 && v1.bytes == 768);
    CHECK(none.p == nullptr && none.bytes == 0 && none.view);
    // re-sizing a view is refused and changes nothing, with or without keep; inside its size it is served like any buffer
    const std::string before = H::log;
    void* const p1 = v1.p;
    CHECK(v1.ensure(769, 0).step == BufStep::View && v1.ensure(4096, 0, true).step == BufStep::View);
    CHECK(none.ensure(1, 0).step == BufStep::View && !v1.ensure(768, 0));
    CHECK(v1.p == p1 && v1.bytes == 768 && v1.view && H::log == before && H::live_bytes == 1024);
    // a view moves as a view, is dropped without a free, and a buffer that owned a block frees it on becoming a view
    Buf w(std::move(v0));
    CHECK(w.view && w.bytes == 256 && v0.p == nullptr && !v0.view);
    w.drop();
    CHECK(w.p == nullptr && !w.view && H::frees == 0);
    Buf owner;
    CHECK(!owner.ensure(32, 0));
    owner.slice(arena, 0, 64);
    CHECK(H::frees == 1 && owner.view && H::live_bytes == 1024);
    owner.slice(arena, 64, 64);  // (re-sliced: a new layout in the same arena)
    CHECK(H::frees == 1 && owner.p == static_cast<char*>(arena.p) + 64);
  }
  CHECK(H::live_bytes == 0 && H::bad_frees == 0 && H::frees == 2 && H::allocs == 2);
}

// a call sequence as the library makes them, returning at the first failure as its callers do: plain growth, growth with
// keep, the two-buffer replacement of gpso_vgp_extend_q, an arena carved twice.  -> the allocations it asked for
static bool sequence(Buf& S, Buf& mu, Buf& cnt, Buf& arena, Buf (&slices)[3]) {
  if (S.ensure(128 * 128, 0) || mu.ensure(128, 0) || cnt.ensure(64, 0, true)) return false;
  if (S.ensure(256 * 256, 0) || cnt.ensure(256, 0, true)) return false;
  {
    Buf nS, nmu;
    if (nS.ensure(512 * 512, 0) || nmu.ensure(512, 0)) return false;  // (the second failing must not leak the first)
    std::memcpy(nmu.p, mu.p, mu.bytes);
    if (H::sync(0)) return false;
    S = std::move(nS);
    mu = std::move(nmu);
  }
  for (size_t total : {(size_t)3000, (size_t)9000}) {
    for (Buf& b : slices) b.drop();
    if (arena.ensure(total, 0)) return false;
    size_t off = 0;
    for (Buf& b : slices) {
      b.slice(arena, off, total / 3);
      off += total / 3;
    }
  }
  return true;
}

static void one_allocation_fails() {
  int asked = 0;
  for (int fail = 0; fail == 0 || fail <= asked; ++fail) {
    H::reset(fail);
    bool ok;
    {
      Buf S, mu, cnt, arena, slices[3];
      ok = sequence(S, mu, cnt, arena, slices);
      if (ok) CHECK(S.bytes == 512 * 512 && mu.bytes == 512 && cnt.bytes == 256 && arena.bytes == 9000 && slices[2].bytes == 3000);
      if (ok) CHECK(H::live_bytes == 512 * 512 + 512 + 256 + 9000);
    }
    CHECK(ok == (fail == 0));
    CHECK(H::live_bytes == 0 && H::live.empty() && H::bad_frees == 0);
    CHECK(H::frees == H::allocs - (fail ? 1 : 0));
    if (fail == 0) asked = H::allocs;
  }
  CHECK(asked == 9);
}

int main() {
  ownership();
  keep_carries_the_old_bytes();
  views();
  one_allocation_fails();
  if (failures) std::fprintf(stderr, "%d checks failed\n", failures);
  else std::printf("devbuf_check: ok\n");
  return failures ? 1 : 0;
}
