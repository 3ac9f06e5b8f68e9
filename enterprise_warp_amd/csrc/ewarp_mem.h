// ewarp_mem.h — the one owner of device and pinned host memory of the C ABI.
// Every allocation and every free of the library goes through mem_alloc /
// mem_free; a growable buffer is a Buf, a context's persistent uploads live in
// an Arena.  No HIP include: the two functions are the link-time seam behind
// which tests/hip/mem_owner_test.cpp checks this header on the host.
#pragma once

#include <cstddef>
#include <vector>

namespace ewh_mem {

// PinnedCoherent: portable, mapped and coherent host memory (the latency
// kernel's theta / output staging); PinnedPortable: plain portable staging
enum class MemKind { Device, PinnedPortable, PinnedCoherent };

// Defined once, in ewarp_hip.hip, with the HIP calls.  mem_alloc returns 0, or
// EWH_E_NOMEM with the thread's error message set and *p = nullptr.  mem_free
// is synchronous (hipFree / hipHostFree): work still queued on the block ends
// first.
int mem_alloc(MemKind kind, void** p, size_t bytes);
void mem_free(MemKind kind, void* p);

// What a (re)allocation invalidates, run before the block changes: a
// context's captured graphs (they hold device pointers), the latency path's
// record of a pinned buffer's device address.
struct Hook {
  void (*fn)(void*) = nullptr;
  void* arg = nullptr;
  void operator()() const {
    if (fn) fn(arg);
  }
};

// One growable buffer of `cap` elements.  Contents do not survive growth.
template <typename T>
struct Buf {
  T* p = nullptr;
  size_t cap = 0;
  MemKind kind = MemKind::Device;

  void release() {
    if (p) mem_free(kind, p);
    p = nullptr;
    cap = 0;
  }
  // room for `need` elements; after a failure the buffer is empty
  int reserve(size_t need, Hook changed = {}) {
    if (need <= cap) return 0;      // (inline: the single-theta path passes here on every call)
    return grow(need, changed);
  }
  int grow(size_t need, Hook changed) {
    changed();
    release();
    const int rc = mem_alloc(kind, (void**)&p, (need ? need : 1) * sizeof(T));
    if (rc) {
      p = nullptr;
      return rc;
    }
    cap = need;
    return 0;
  }
};

// Blocks that live as long as their owner and never grow: a context's tables
// and caches (create, setup), the scratch of one setup step (a local Arena).
struct Arena {
  MemKind kind = MemKind::Device;
  Hook changed;
  std::vector<void*> blocks;

  Arena() = default;
  explicit Arena(Hook h) : changed(h) {}
  Arena(const Arena&) = delete;
  Arena& operator=(const Arena&) = delete;
  ~Arena() { release(); }

  template <typename T>
  int alloc(T** p, size_t count) {
    changed();
    *p = nullptr;
    const int rc = mem_alloc(kind, (void**)p, (count ? count : 1) * sizeof(T));
    if (rc) {
      *p = nullptr;
      return rc;
    }
    blocks.push_back(*p);
    return 0;
  }
  void release() {
    for (void* q : blocks) mem_free(kind, q);
    blocks.clear();
  }
};

}  // namespace ewh_mem
