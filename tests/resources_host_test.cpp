// Host test of csrc/sogm_resources.hpp: the owner compiled with the host compiler against a counting stand-in for the
// HIP entry points it calls (defined here; no GPU runtime is linked).  The stand-in hands out made-up handles, counts
// the live ones per kind, logs every call in order and can be told to fail the k-th acquisition from now.
#include "sogm_resources.hpp"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

namespace fake {
enum Kind { STREAM, EVENT, DEVICE, PINNED, N_KIND };
struct Call {
  std::string what;  // "acquire", "sync", "release"
  Kind        kind;
  void       *handle;
};
int                  live[N_KIND];
std::vector<Call>    calls;
std::map<void *, int> released;   // handle -> times released
std::map<void *, Kind> kind_of;   // every handle ever handed out
int                  fail_in = 0;   // > 0: the fail_in-th acquisition from now fails
int                  fail_memset = 0;
int                  memsets = 0;
uintptr_t            next_handle = 0x1000;

hipError_t acquire(Kind k, void **out, hipError_t err) {
  if (fail_in > 0 && --fail_in == 0) return err;
  void *h = (void *)(next_handle += 0x100);
  kind_of[h] = k;
  ++live[k];
  calls.push_back({"acquire", k, h});
  *out = h;
  return hipSuccess;
}
hipError_t release(Kind k, void *h) {
  if (!kind_of.count(h) || kind_of[h] != k) {
    std::printf("FAIL: release of a handle of the wrong kind or never handed out: %p\n", h);
    std::exit(1);
  }
  ++released[h];
  --live[k];
  calls.push_back({"release", k, h});
  return hipSuccess;
}
}  // namespace fake

extern "C" {
hipError_t hipMalloc(void **p, size_t) { return fake::acquire(fake::DEVICE, p, hipErrorOutOfMemory); }
hipError_t hipHostMalloc(void **p, size_t, unsigned) { return fake::acquire(fake::PINNED, p, hipErrorOutOfMemory); }
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned flags) {
  if (flags != hipStreamNonBlocking) return hipErrorInvalidValue;
  return fake::acquire(fake::STREAM, (void **)s, hipErrorUnknown);
}
hipError_t hipExtStreamCreateWithCUMask(hipStream_t *s, uint32_t, const uint32_t *) {
  return fake::acquire(fake::STREAM, (void **)s, hipErrorUnknown);
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return fake::acquire(fake::EVENT, (void **)e, hipErrorUnknown); }
hipError_t hipMemset(void *, int, size_t) {
  ++fake::memsets;
  return fake::fail_memset ? hipErrorUnknown : hipSuccess;
}
hipError_t hipFree(void *p) { return fake::release(fake::DEVICE, p); }
hipError_t hipHostFree(void *p) { return fake::release(fake::PINNED, p); }
hipError_t hipStreamSynchronize(hipStream_t s) {
  fake::calls.push_back({"sync", fake::STREAM, (void *)s});
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) { return fake::release(fake::STREAM, (void *)s); }
hipError_t hipEventDestroy(hipEvent_t e) { return fake::release(fake::EVENT, (void *)e); }
}

#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      return 1;                                                       \
    }                                                                 \
  } while (0)

static bool nothing_live() {
  for (int k = 0; k < fake::N_KIND; ++k)
    if (fake::live[k] != 0) return false;
  return true;
}
static bool each_released_once() {
  for (auto &kv : fake::kind_of)
    if (fake::released[kv.first] != 1) return false;
  return true;
}
static bool is_memory(fake::Kind k) { return k == fake::DEVICE || k == fake::PINNED; }

// 1, 2: a scripted set-up, two single releases, one regrow, then everything — counts, exactly-once and order
static int test_script() {
  sogm::Resources r;
  struct {
    float              *a = nullptr, *b = nullptr, *c = nullptr, *g = nullptr;
    int                *d = nullptr;
    unsigned long long *h = nullptr;
    hipStream_t         s1 = nullptr, s2 = nullptr, s3 = nullptr;
    hipEvent_t          e1 = nullptr, e2 = nullptr, e3 = nullptr;
  } f;
  const uint32_t mask[2] = {0xFFFFFFFFu, 0xFFFFu};
  EXPECT(r.device(&f.a, 64) == hipSuccess);
  EXPECT(r.device(&f.b, 128, true) == hipSuccess && fake::memsets == 1);
  EXPECT(r.pinned(&f.h, 32, hipHostMallocMapped) == hipSuccess);
  EXPECT(r.stream(&f.s1) == hipSuccess);
  EXPECT(r.stream_masked(&f.s2, 2, mask) == hipSuccess);
  EXPECT(r.event(&f.e1) == hipSuccess);
  EXPECT(r.event(&f.e2, hipEventDefault) == hipSuccess);
  EXPECT(r.device(&f.c, 256) == hipSuccess);
  EXPECT(r.array(&f.d, 0) == hipSuccess && f.d != nullptr);  // (no bytes asked: 16 taken, the pointer is real)
  EXPECT(r.event(&f.e3) == hipSuccess);
  EXPECT(r.stream(&f.s3) == hipSuccess);
  EXPECT(r.device(&f.g, 512) == hipSuccess);
  EXPECT(f.a && f.b && f.h && f.s1 && f.s2 && f.e1 && f.e2 && f.c && f.e3 && f.s3 && f.g);
  EXPECT(fake::live[fake::DEVICE] == 5 && fake::live[fake::PINNED] == 1 && fake::live[fake::STREAM] == 3 &&
         fake::live[fake::EVENT] == 3);
  // two single releases and one regrow
  r.release(&f.b);
  r.release(&f.e2);
  EXPECT(!f.b && !f.e2 && fake::live[fake::DEVICE] == 4 && fake::live[fake::EVENT] == 2);
  void *old_c = f.c;
  r.release(&f.c);
  EXPECT(r.device(&f.c, 1024) == hipSuccess && f.c && (void *)f.c != old_c && fake::live[fake::DEVICE] == 4);
  // what is held now, in order of acquisition
  std::vector<fake::Call> held;
  for (auto &c : fake::calls)
    if (c.what == "acquire" && !fake::released.count(c.handle)) held.push_back(c);
  EXPECT(held.size() == 10);
  const size_t before = fake::calls.size();
  void *const  last_stream = (void *)f.s3, *const first_memory = (void *)f.a;
  r.release_all();
  EXPECT(nothing_live() && each_released_once());
  EXPECT(!f.a && !f.c && !f.g && !f.d && !f.h && !f.s1 && !f.s2 && !f.s3 && !f.e1 && !f.e3);  // no field is left dangling
  // expected: streams (each synchronised, then destroyed), then events, then memory; reverse of acquisition within a kind
  std::vector<fake::Call> want;
  for (int pass = 0; pass < 3; ++pass)
    for (size_t i = held.size(); i-- > 0;) {
      const fake::Kind k = held[i].kind;
      if (pass == 0 && k == fake::STREAM) {
        want.push_back({"sync", k, held[i].handle});
        want.push_back({"release", k, held[i].handle});
      } else if ((pass == 1 && k == fake::EVENT) || (pass == 2 && is_memory(k))) {
        want.push_back({"release", k, held[i].handle});
      }
    }
  EXPECT(fake::calls.size() - before == want.size());
  for (size_t i = 0; i < want.size(); ++i) {
    const fake::Call &got = fake::calls[before + i];
    EXPECT(got.what == want[i].what && got.kind == want[i].kind && got.handle == want[i].handle);
  }
  EXPECT(want.front().handle == last_stream && want.back().handle == first_memory);
  r.release_all();  // (a second time does nothing)
  EXPECT(fake::calls.size() == before + want.size());
  return 0;
}

// 3: a marked set-up in the library's style — guarded by the field it fills first, error returns from the middle
struct Lazy {
  hipStream_t guard = nullptr, masked = nullptr;
  hipEvent_t  ev_in = nullptr, ev_done = nullptr;
  int        *ready = nullptr, *ctl = nullptr;
  long long  *host = nullptr;
  bool all() const { return guard && masked && ev_in && ev_done && ready && ctl && host; }
  bool none() const { return !guard && !masked && !ev_in && !ev_done && !ready && !ctl && !host; }
};
#define CHECK_HIP(expr) \
  do {                  \
    if ((expr) != hipSuccess) return -1; \
  } while (0)
static int lazy_setup(sogm::Resources &r, Lazy &z) {
  if (z.guard) return 0;
  sogm::Resources::Setup setup(r);
  const uint32_t mask[1] = {0xFFu};
  CHECK_HIP(r.stream(&z.guard));
  CHECK_HIP(r.stream_masked(&z.masked, 1, mask));
  CHECK_HIP(r.event(&z.ev_in));
  CHECK_HIP(r.event(&z.ev_done));
  CHECK_HIP(r.device(&z.ready, 64, true));
  CHECK_HIP(r.device(&z.ctl, 64));
  CHECK_HIP(r.pinned(&z.host, 32, hipHostMallocMapped));
  return setup.done();
}
static const int LAZY_ACQUISITIONS = 7;

static int test_rollback() {
  for (int k = 1; k <= LAZY_ACQUISITIONS + 1; ++k) {  // (the last round fails the zero-fill instead of an acquisition)
    sogm::Resources r;
    Lazy            z;
    float          *base0 = nullptr;
    hipEvent_t      base1 = nullptr;
    EXPECT(r.device(&base0, 64) == hipSuccess && r.event(&base1) == hipSuccess);
    int at_mark[fake::N_KIND];
    for (int i = 0; i < fake::N_KIND; ++i) at_mark[i] = fake::live[i];
    if (k <= LAZY_ACQUISITIONS)
      fake::fail_in = k;
    else
      fake::fail_memset = 1;
    EXPECT(lazy_setup(r, z) != 0);
    EXPECT(fake::fail_in == 0);  // (the injected failure was reached)
    fake::fail_memset = 0;
    for (int i = 0; i < fake::N_KIND; ++i) EXPECT(fake::live[i] == at_mark[i]);
    EXPECT(z.none() && base0 && base1);
    EXPECT(lazy_setup(r, z) == 0 && z.all());  // the second attempt is a whole one
    EXPECT(fake::live[fake::STREAM] == at_mark[fake::STREAM] + 2 && fake::live[fake::EVENT] == at_mark[fake::EVENT] + 2 &&
           fake::live[fake::DEVICE] == at_mark[fake::DEVICE] + 2 && fake::live[fake::PINNED] == at_mark[fake::PINNED] + 1);
    const size_t n_calls = fake::calls.size();
    EXPECT(lazy_setup(r, z) == 0 && fake::calls.size() == n_calls);  // guarded: nothing happens
    r.release_all();
    EXPECT(nothing_live() && each_released_once());
  }
  return 0;
}

// 4: releasing twice, releasing null, releasing what is not held
static int test_release_is_harmless() {
  sogm::Resources r, other;
  float          *p = nullptr, *null_field = nullptr, *foreign = nullptr;
  hipStream_t     s = nullptr;
  EXPECT(r.device(&p, 64) == hipSuccess && r.stream(&s) == hipSuccess && other.device(&foreign, 64) == hipSuccess);
  float      *p_copy = p;
  hipStream_t s_copy = s;
  r.release(&p);
  r.release(&p);       // null by now
  r.release(&p_copy);  // the same handle again, through a stale copy
  r.release(&s);
  r.release(&s_copy);
  r.release(&null_field);
  EXPECT(!p && !p_copy && !s && !s_copy && !null_field);
  float *foreign_copy = foreign;
  r.release(&foreign_copy);  // held by another owner: not freed here
  EXPECT(fake::released.count((void *)foreign) == 0);
  r.release_all();
  other.release_all();
  EXPECT(nothing_live() && each_released_once());
  return 0;
}

int main() {
  if (test_script() || test_rollback() || test_release_is_harmless()) return 1;
  std::printf("resources host ok\n");
  return 0;
}
