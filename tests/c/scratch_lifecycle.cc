// The context's scratch-buffer logic (nghttp3_amd/csrc/qh_scratch.h) over a
// malloc-backed allocator: built with -fsanitize=address,undefined and run
// by tests/test_scratch_lifecycle.py.  For every capacity policy the library
// uses: capacity never shrinks, "grown" is reported exactly when the buffer
// is a new allocation, every allocation is freed exactly once (after a
// quiesce when it was live), and a reserve that fails leaves the buffer
// empty or untouched, never a freed pointer with a stale capacity.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>

#include "qh_scratch.h"

#define CHECK(x)                                                      \
  do {                                                                \
    if (!(x)) {                                                       \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

namespace {

struct MallocAlloc {
  std::map<void *, size_t> live;  // pointer -> serial number of its allocation
  size_t serial = 0, frees = 0, quiesces = 0;
  bool fail_alloc = false, fail_quiesce = false;
  bool alloc(void **p, size_t bytes, qhs::Kind) {
    if (fail_alloc) {
      *p = reinterpret_cast<void *>(0x1);  // (a failed hipMalloc's output is unspecified)
      return false;
    }
    *p = malloc(bytes);
    CHECK(*p != nullptr && bytes > 0);
    live[*p] = ++serial;
    return true;
  }
  void free(void *p, qhs::Kind) {
    CHECK(live.erase(p) == 1);  // allocated here, and not freed before
    ::free(p);
    ++frees;
  }
  bool quiesce() {
    ++quiesces;
    return !fail_quiesce;
  }
  size_t serial_of(const void *p) const {
    if (!p) return 0;
    auto it = live.find(const_cast<void *>(p));
    CHECK(it != live.end());  // a buffer's pointer is always a live allocation
    return it->second;
  }
};

// One reserve, checked against the buffer's state before it.
int reserve_checked(MallocAlloc &a, qhs::Scratch &s, size_t bytes, qhs::Policy pol) {
  const size_t cap0 = s.cap, id0 = a.serial_of(s.p), frees0 = a.frees, q0 = a.quiesces;
  const int r = qhs::reserve(a, s, bytes, pol);
  CHECK(r == qhs::kGrown || r == qhs::kKept);
  CHECK(s.cap >= cap0 && s.cap >= bytes);
  CHECK((s.p == nullptr) == (s.cap == 0));
  const size_t id1 = a.serial_of(s.p);
  CHECK((r == qhs::kGrown) == (id1 != id0));
  if (r == qhs::kGrown) {  // the old allocation freed once, after a quiesce
    CHECK(a.frees == frees0 + (id0 ? 1 : 0) && a.quiesces == q0 + (id0 ? 1 : 0));
    CHECK(s.cap == (pol.min ? qhs::pow2_at_least(bytes, pol.min) : bytes));
  } else {
    CHECK(a.frees == frees0 && a.quiesces == q0 && s.cap == cap0);
  }
  if (s.p) memset(s.p, 0xA5, s.cap);  // (the whole capacity is the buffer's)
  return r;
}

void lifecycle(qhs::Policy pol) {
  MallocAlloc a;
  qhs::Scratch s;
  const size_t min = pol.min ? pol.min : 4096;
  CHECK(reserve_checked(a, s, 0, pol) == qhs::kKept && !s.p && a.serial == 0);
  CHECK(reserve_checked(a, s, 1, pol) == qhs::kGrown);
  CHECK(s.cap == (pol.min ? pol.min : 1));
  CHECK(reserve_checked(a, s, min - 1, pol) == (pol.min ? qhs::kKept : qhs::kGrown));
  CHECK(reserve_checked(a, s, min + 1, pol) == qhs::kGrown);
  CHECK(s.cap == (pol.min ? 2 * pol.min : min + 1));
  CHECK(reserve_checked(a, s, min / 2, pol) == qhs::kKept);
  CHECK(reserve_checked(a, s, s.cap, pol) == qhs::kKept);
  CHECK(reserve_checked(a, s, 37 * min + 5, pol) == qhs::kGrown);
  CHECK(s.cap == (pol.min ? 64 * pol.min : 37 * min + 5));

  // a failed quiesce: the buffer stays as it was, still live
  const qhs::Scratch before = s;
  a.fail_quiesce = true;
  CHECK(qhs::reserve(a, s, 2 * s.cap, pol) == qhs::kFailed);
  CHECK(s.p == before.p && s.cap == before.cap && a.serial_of(s.p) != 0);
  a.fail_quiesce = false;
  // a failed allocation: the old buffer freed once, the buffer empty
  const size_t frees0 = a.frees;
  a.fail_alloc = true;
  CHECK(qhs::reserve(a, s, 2 * s.cap, pol) == qhs::kFailed);
  CHECK(s.p == nullptr && s.cap == 0 && a.frees == frees0 + 1 && a.live.empty());
  CHECK(qhs::reserve(a, s, 16, pol) == qhs::kFailed && s.p == nullptr && s.cap == 0);
  a.fail_alloc = false;
  // and it can be reserved again, then released (twice: the second is a no-op)
  CHECK(reserve_checked(a, s, 3 * min, pol) == qhs::kGrown);
  qhs::release(a, s);
  CHECK(s.p == nullptr && s.cap == 0);
  qhs::release(a, s);
  CHECK(a.live.empty() && a.frees == a.serial);
}

}  // namespace

int main() {
  // the library's policies: exact size; powers of two from 1 MiB, from 1024
  // words (tile states) and from two halves of 1024 words (framing look-back)
  const qhs::Policy pols[] = {qhs::kExact, qhs::kPow2MiB, qhs::Policy{1024 * 8}, qhs::Policy{2 * 1024 * 8}};
  for (const qhs::Policy &p : pols) lifecycle(p);
  static_assert(qhs::pow2_at_least(0, 4096) == 4096 && qhs::pow2_at_least(4097, 4096) == 8192 &&
                    qhs::pow2_at_least(SIZE_MAX, 4096) == SIZE_MAX,
                "pow2_at_least");
  printf("scratch lifecycle ok: %zu policies\n", sizeof(pols) / sizeof(pols[0]));
  return 0;
}
