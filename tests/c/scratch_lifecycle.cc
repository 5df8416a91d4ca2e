// The context's scratch-buffer logic (nghttp3_amd/csrc/qh_scratch.h) over a
// malloc-backed allocator: built with -fsanitize=address,undefined and run
// by tests/test_scratch_lifecycle.py.  For every capacity policy the library
// uses: capacity never shrinks, "grown" is reported exactly when the buffer
// is a new allocation, every allocation is freed exactly once (after a
// quiesce when it was live), and a reserve that fails leaves the buffer
// empty or untouched, never a freed pointer with a stale capacity.
// Then the layout and staging types of the same header: a buffer of exactly
// a layout's total, every piece written to its full extent; host pieces
// copied in and back with memcpy in HIP's place.
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

// One piece list, as the library writes them: types of 1, 4, 8 and 16 bytes.
struct Wide {
  uint64_t a, b;
};
struct Pieces {
  static constexpr int kN = 6;
  uint8_t *bytes;
  uint32_t *words;
  Wide *wide;
  uint64_t *longs;
  uint8_t *pad;
  uint32_t *last;
  const uint8_t *at(int k) const {
    const void *const p[kN] = {bytes, words, wide, longs, pad, last};
    return static_cast<const uint8_t *>(p[k]);
  }
};
struct Counts {
  uint64_t n[Pieces::kN];
  uint64_t bytes(int k) const {
    const uint64_t size[Pieces::kN] = {1, 4, sizeof(Wide), 8, 1, 4};
    return n[k] * size[k];
  }
};
template <class L>
Pieces take_all(L &l, const Counts &c) {
  Pieces p;
  p.bytes = l.template take<uint8_t>(c.n[0]);
  p.words = l.template take<uint32_t>(c.n[1]);
  p.wide = l.template take<Wide>(c.n[2]);
  p.longs = l.template take<uint64_t>(c.n[3]);
  p.pad = l.template take<uint8_t>(c.n[4]);
  p.last = l.template take<uint32_t>(c.n[5]);
  return p;
}

void layout(const Counts &c) {
  // the sizing pass: no base, null pointers, the offsets from the totals
  qhs::Layout sized;
  uint64_t off[Pieces::kN + 1];
  {
    qhs::Layout l;
    for (int k = 0; k < Pieces::kN; ++k) {
      Counts upto = c;
      for (int j = k; j < Pieces::kN; ++j) upto.n[j] = 0;
      l = qhs::Layout{};
      const Pieces p = take_all(l, upto);
      off[k] = l.total;  // (what the pieces before k take)
      for (int j = 0; j < Pieces::kN; ++j) CHECK(p.at(j) == nullptr);
    }
    take_all(sized, c);
    off[Pieces::kN] = sized.total;
  }
  for (int k = 0; k < Pieces::kN; ++k) {
    CHECK(off[k] % 256 == 0 && off[k] <= off[k + 1]);
    CHECK(off[k] + c.bytes(k) <= off[k + 1]);                // disjoint, in order, inside total
    CHECK(off[k + 1] - off[k] < c.bytes(k) + 256);           // no more than the round-up
    if (c.n[k] == 0) CHECK(off[k + 1] == off[k]);            // a piece of nothing takes no room
  }
  // the placing pass over a buffer of exactly the total
  MallocAlloc a;
  qhs::Scratch s;
  CHECK(qhs::reserve(a, s, sized.total, qhs::kExact) != qhs::kFailed && s.cap == sized.total);
  qhs::Layout placed;
  placed.base = static_cast<uint8_t *>(s.p);
  const Pieces p = take_all(placed, c);
  CHECK(placed.total == sized.total);
  for (int k = 0; k < Pieces::kN; ++k) {
    if (!s.p) {
      CHECK(p.at(k) == nullptr);
      continue;
    }
    CHECK(p.at(k) == placed.base + off[k]);  // the same offsets as the sizing pass
    if (c.bytes(k)) memset(const_cast<uint8_t *>(p.at(k)), 0x40 + k, c.bytes(k));
  }
  for (int k = 0; k < Pieces::kN; ++k)  // (no piece's bytes were another's)
    for (uint64_t i = 0; i < c.bytes(k); ++i) CHECK(p.at(k)[i] == 0x40 + k);
  qhs::release(a, s);
}

int host_copy(void *to, const void *from, uint64_t bytes) {
  CHECK(to && from && bytes);  // (a null or empty piece is no copy)
  memcpy(to, from, bytes);
  return 0;
}

// Pieces in, both ways, back, and neither; null and empty ones among them.
void staging() {
  const uint64_t n_in = 257, n_both = 64, n_out = 3;
  uint8_t h_in[n_in];
  uint32_t h_both[n_both], h_both0[n_both];
  uint64_t h_out[n_out], h_never = 7;
  for (uint64_t i = 0; i < n_in; ++i) h_in[i] = (uint8_t)(i * 7 + 1);
  for (uint64_t i = 0; i < n_both; ++i) h_both0[i] = h_both[i] = (uint32_t)(i * 0x01010101u);
  memset(h_out, 0, sizeof(h_out));
  qhs::Staged st;
  const auto r_in = st.in(h_in, n_in);
  const auto r_null = st.in(static_cast<const uint8_t *>(nullptr), 5);  // room, no copy
  const auto r_both = st.take<uint32_t>(n_both, h_both, h_both);
  const auto r_empty = st.take<uint64_t>(0, &h_never, &h_never);  // no room, no copy
  const auto r_out = st.out(h_out, n_out);
  const auto r_none = st.out(static_cast<uint64_t *>(nullptr), 2);
  const auto r_pad = st.take<uint8_t>(16);  // (no host side)
  CHECK(st.npieces == 4 && st.sized.total == 512 + 256 + 256 + 0 + 256 + 256 + 256);
  CHECK(r_in.off == 0 && r_null.off == 512 && r_both.off == 768 && r_empty.off == 1024);
  CHECK(r_out.off == 1024 && r_none.off == 1280 && r_pad.off == 1536);
  MallocAlloc a;
  qhs::Scratch s;
  CHECK(qhs::reserve(a, s, st.sized.total, qhs::kExact) == qhs::kGrown);
  memset(s.p, 0xEE, s.cap);
  st.base = static_cast<uint8_t *>(s.p);
  uint8_t *const d_in = st(r_in), *const d_null = st(r_null), *const d_pad = st(r_pad);
  uint32_t *const d_both = st(r_both);
  uint64_t *const d_out = st(r_out), *const d_none = st(r_none);
  CHECK(d_in == st.base && (uint8_t *)d_both == st.base + 768 && (uint8_t *)st(r_empty) == (uint8_t *)d_out);
  int copies = 0;
  auto counted = [&](void *to, const void *from, uint64_t bytes) {
    ++copies;
    return host_copy(to, from, bytes);
  };
  CHECK(st.copy(false, counted) == 0 && copies == 2);  // h_in and h_both arrive
  CHECK(memcmp(d_in, h_in, n_in) == 0 && memcmp(d_both, h_both, sizeof(h_both)) == 0);
  for (int i = 0; i < 5; ++i) CHECK(d_null[i] == 0xEE);
  for (uint64_t i = 0; i < n_both; ++i) d_both[i] = ~d_both[i];  // the "kernel"
  for (uint64_t i = 0; i < n_out; ++i) d_out[i] = 0x1111111111111111ull * (i + 1);
  memset(d_none, 0x22, 2 * sizeof(uint64_t));
  memset(d_pad, 0x33, 16);
  copies = 0;
  CHECK(st.copy(true, counted) == 0 && copies == 2);  // h_both and h_out return
  for (uint64_t i = 0; i < n_both; ++i) CHECK(h_both[i] == ~h_both0[i]);
  for (uint64_t i = 0; i < n_out; ++i) CHECK(h_out[i] == 0x1111111111111111ull * (i + 1));
  CHECK(h_never == 7);
  // a copy's error ends the pass and is the pass's result
  copies = 0;
  CHECK(st.copy(false, [&](void *, const void *, uint64_t) { return ++copies, -5; }) == -5 && copies == 1);
  qhs::release(a, s);
  CHECK(a.live.empty());
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
  static_assert(qhs::align_up(0) == 0 && qhs::align_up(1) == 256 && qhs::align_up(256) == 256 &&
                    qhs::align_up(257) == 512,
                "align_up");
  // zero counts, one-byte pieces, pieces of exactly 256 and of 257 bytes
  const Counts lists[] = {
      {{0, 0, 0, 0, 0, 0}},  {{1, 1, 1, 1, 1, 1}},     {{256, 64, 16, 32, 16, 0}},
      {{257, 65, 17, 33, 0, 1}}, {{0, 3, 0, 0, 257, 64}}, {{255, 0, 16, 0, 0, 0}},
      {{0, 0, 0, 0, 0, 5}},  {{1000, 0, 1, 31, 256, 63}},
  };
  for (const Counts &c : lists) layout(c);
  staging();
  printf("scratch lifecycle ok: %zu policies, %zu layouts, staging\n", sizeof(pols) / sizeof(pols[0]),
         sizeof(lists) / sizeof(lists[0]));
  return 0;
}
