// arena.h -- the device arena's range allocator (host code only: it never touches the memory it hands out).
#pragma once
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <iterator>
#include <map>
#include <mutex>

namespace ibwa {

// Device arena (ibwa_reserve): one hipMalloc per device, made once, from which every buffer of the
// process's contexts on that device is carved (first fit, 4 KiB granules, freed ranges coalesce).
// A hipMalloc right after another process released a lot of HBM waits until the driver has wiped
// that memory (measured: 0.5-2.7 s for single allocations of `aln` end 2, profiles/r05_alloc.jsonl);
// a CLI that reserves its arena while it loads the index pays that once, overlapped, instead of in
// the middle of its first groups.  Without a reservation buffers are plain hipMallocs.
struct Arena {
  std::mutex mu;
  char *base = nullptr;
  size_t size = 0, used = 0, peak = 0;
  std::map<size_t, size_t> free_;  // offset -> bytes
  const bool trace = getenv("IBWA_ARENA_TRACE") != nullptr;  // every carve and release, on stderr
  void *alloc(size_t n) {
    n = (n + 4095) & ~(size_t)4095;
    std::lock_guard<std::mutex> lk(mu);
    for (auto it = free_.begin(); it != free_.end(); ++it) {
      if (it->second < n) continue;
      const size_t off = it->first, rest = it->second - n;
      free_.erase(it);
      if (rest) free_[off + n] = rest;
      used += n;
      peak = std::max(peak, used);
      if (trace) fprintf(stderr, "[ibwa_amd arena] +%.3f GB at %.3f GB: used %.3f GB\n", n / 1e9, off / 1e9, used / 1e9);
      return base + off;
    }
    return nullptr;
  }
  bool owns(const void *p) const {
    return base && static_cast<const char *>(p) >= base && static_cast<const char *>(p) < base + size;
  }
  void release(void *p, size_t n) {
    n = (n + 4095) & ~(size_t)4095;
    std::lock_guard<std::mutex> lk(mu);
    size_t off = (size_t)(static_cast<char *>(p) - base);
    used -= n;
    if (trace) fprintf(stderr, "[ibwa_amd arena] -%.3f GB at %.3f GB: used %.3f GB\n", n / 1e9, off / 1e9, used / 1e9);
    auto nx = free_.lower_bound(off);
    if (nx != free_.end() && off + n == nx->first) {  // merge with the next free range
      n += nx->second;
      nx = free_.erase(nx);
    }
    if (nx != free_.begin()) {
      auto pv = std::prev(nx);
      if (pv->first + pv->second == off) {  // and with the previous one
        pv->second += n;
        return;
      }
    }
    free_[off] = n;
  }
};

}  // namespace ibwa
