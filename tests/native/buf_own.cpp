// Ownership of pm::Buf (runtime.hpp) and of what holds one, under g++ ASan +
// UBSan (`make -C halo2-aggregation_amd buf_own` builds and runs this;
// tests/test_buf_own.py drives it).  The HIP
// allocator is a counting shim over malloc, so a leak shows as a live
// allocation at the end, a double free as an unknown pointer (and as an ASan
// report), and no device is needed.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "../../halo2-aggregation_amd/csrc/runtime.hpp"

static std::set<void*> g_live;
static int g_fail = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      g_fail++;                                                         \
    }                                                                   \
  } while (0)

extern "C" hipError_t hipMalloc(void** p, size_t bytes) {
  *p = std::malloc(bytes);
  g_live.insert(*p);
  return hipSuccess;
}
extern "C" hipError_t hipFree(void* p) {
  CHECK(g_live.erase(p) == 1);  // a pointer this shim handed out, freed once
  std::free(p);
  return hipSuccess;
}
extern "C" const char* hipGetErrorString(hipError_t) { return "shim"; }
int pm::set_error(int code, const std::string&) { return code; }

int main() {
  using pm::Buf;
  {
    Buf a;
    CHECK(a.ensure(100) == PM_OK && a.p && a.cap >= 100 && g_live.size() == 1);
    void* const p0 = a.p;
    const uint64_t g0 = a.gen;
    CHECK(a.ensure(50) == PM_OK && a.p == p0 && a.gen == g0);  // grow-only: no reallocation
    CHECK(a.ensure(1 << 20) == PM_OK && a.cap >= (1u << 20) && a.gen != g0 && g_live.size() == 1);

    Buf b(std::move(a));  // move construction: a gives its memory up
    CHECK(!a.p && a.cap == 0 && b.p && g_live.size() == 1);

    Buf c;
    CHECK(c.ensure(4096) == PM_OK && g_live.size() == 2);
    const uint64_t gc = c.gen;
    void* const pb = b.p;
    c = std::move(b);  // move assignment onto a live buffer frees the old one
    CHECK(c.p == pb && !b.p && c.gen != gc && g_live.size() == 1);
    c = std::move(c);  // self-assignment keeps it
    CHECK(c.p == pb && g_live.size() == 1);

    c.release();
    CHECK(!c.p && c.cap == 0 && g_live.empty());
    c.release();  // idempotent
    CHECK(c.ensure(10) == PM_OK && g_live.size() == 1);
  }
  CHECK(g_live.empty());
  {
    // a vector of twiddle slots that reallocates (pm_ctx::ntt_tw), and the
    // other holders of a Buf
    std::vector<pm::NttTwiddles> tw;
    for (int i = 0; i < 9; i++) {
      tw.emplace_back();
      tw.back().logn = (uint32_t)i;
      CHECK(tw.back().buf.ensure(1000 + (size_t)i) == PM_OK);
    }
    CHECK(g_live.size() == 9);
    for (int i = 0; i < 9; i++) CHECK(tw[(size_t)i].logn == (uint32_t)i && tw[(size_t)i].buf.cap >= 1000 + (size_t)i);
    tw.erase(tw.begin() + 2);
    CHECK(g_live.size() == 8);

    pm::ManyTable many;
    CHECK(many.d.ensure(128) == PM_OK);
    Buf grown;
    CHECK(grown.ensure(512) == PM_OK);
    many.d = std::move(grown);  // a rebuilt table replaces the old one (many_table_impl)
    pm_fixed_bases ft{};
    CHECK(ft.d.ensure(64) == PM_OK);
    auto* q = new pm_quotient{};
    CHECK(q->d_prog.ensure(8) == PM_OK && q->d_own.ensure(0) == PM_OK && !q->d_own.p);
    delete q;  // a half-built quotient frees what it has
    pm::CachedUpload up;
    CHECK(up.buf.ensure(32) == PM_OK);
    CHECK(g_live.size() == 8 + 3);
  }
  CHECK(g_live.empty());
  if (g_fail) return 1;
  std::printf("buf_own: all checks passed\n");
  return 0;
}
