// Resident NF4 expansions: the bookkeeping behind ``nf4_dequant_resident`` (bindings.cpp).
//
// A frozen NF4 base expands to the same bf16 bytes in every step of a run, so the expansion is made once and
// kept.  This header is the registry's logic only — lookup, verification, byte budget — over plain integers,
// with the payload (the tensors, the producing event) a template parameter: it needs neither torch nor a GPU,
// and tests/native/nf4_resident_sanitize.cpp runs it under the address and undefined-behaviour sanitizers.
//
// Rules:
//  * one entry per codes pointer; the owner of the payload holds references to the codes and scales tensors,
//    so the allocator cannot hand a live entry's pointer to another weight;
//  * a lookup hits only when the scales pointer, n, k and both tensor versions match what was recorded — any
//    mismatch (an in-place rewrite of the base, another weight at a recycled pointer) drops the entry;
//  * over the byte budget nothing is evicted: the caller keeps its expansion as a throw-away copy.  Which
//    weights are resident is then decided by first use and stays put (no thrash).
#pragma once

#include <cstddef>
#include <cstdint>
#include <map>
#include <utility>

struct Nf4ResidentKey {
  uintptr_t codes = 0, scales = 0;                  // device pointers
  int64_t n = 0, k = 0;                             // the weight is [n, k]
  uint64_t codes_version = 0, scales_version = 0;   // the tensors' in-place write counters

  bool operator==(const Nf4ResidentKey& o) const {
    return codes == o.codes && scales == o.scales && n == o.n && k == o.k && codes_version == o.codes_version &&
           scales_version == o.scales_version;
  }
};

template <class Payload>
class Nf4ResidentRegistry {
 public:
  // The entry recorded for exactly this key, or nullptr.  An entry at key.codes that does not match is dropped.
  Payload* find(const Nf4ResidentKey& key) {
    auto it = entries_.find(key.codes);
    if (it == entries_.end()) return nullptr;
    if (it->second.key == key) return &it->second.payload;
    erase(it);
    return nullptr;
  }

  // Whether ``bytes`` more fit under ``budget`` (bytes; <= 0: nothing is resident).
  bool admits(int64_t bytes, int64_t budget) const { return bytes >= 0 && budget > 0 && bytes <= budget - bytes_; }

  // Records ``payload`` for ``key`` when it fits the budget (replacing whatever sat at key.codes); else nullptr and
  // the registry is unchanged apart from that replaced entry.
  Payload* insert(const Nf4ResidentKey& key, int64_t bytes, int64_t budget, Payload payload) {
    drop(key.codes);
    if (!admits(bytes, budget)) return nullptr;
    auto res = entries_.emplace(key.codes, Entry{key, bytes, std::move(payload)});
    bytes_ += bytes;
    return &res.first->second.payload;
  }

  bool drop(uintptr_t codes) {
    auto it = entries_.find(codes);
    if (it == entries_.end()) return false;
    erase(it);
    return true;
  }

  // The key recorded at this codes pointer, or nullptr.
  const Nf4ResidentKey* key_at(uintptr_t codes) const {
    auto it = entries_.find(codes);
    return it == entries_.end() ? nullptr : &it->second.key;
  }

  void clear() {
    entries_.clear();
    bytes_ = 0;
  }

  int64_t bytes() const { return bytes_; }
  size_t size() const { return entries_.size(); }

 private:
  struct Entry {
    Nf4ResidentKey key;
    int64_t bytes;
    Payload payload;
  };
  using Map = std::map<uintptr_t, Entry>;

  void erase(typename Map::iterator it) {
    bytes_ -= it->second.bytes;
    entries_.erase(it);
  }

  Map entries_;
  int64_t bytes_ = 0;
};
