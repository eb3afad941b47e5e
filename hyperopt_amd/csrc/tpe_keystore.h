// tpe_keystore.h — content keys of the per-label fits a suggest keeps across
// calls (tpe_suggest.cpp, include/tpe_hip.h "Resident levels"), internal.
//
// A label's posterior fit is a pure function of a few scalars and of the
// arrays its record points at.  A slot keeps a private copy of all of them —
// the key — and a generation number; a later call whose label has the same
// key, byte for byte, keeps the fit and the generation.  Addresses are never
// compared: histories are rebuilt, and their arrays come back at the same
// address with other content.  No HIP, no library dependency: the stand-alone
// test (tools/ubench/keystore_test.cpp) builds this header alone.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace tpe_keystore {

// one piece of a key: n bytes at p (n == 0: an absent array, p ignored)
struct Seg {
  const void* p;
  size_t n;
};

constexpr int64_t kCapBytes = (int64_t)64 << 20;   // key copies of the whole process

class Store {
 public:
  // total: the process-wide byte count this store's copies are charged to
  Store(std::atomic<int64_t>* total, int64_t cap) : total_(total), cap_(cap) {}
  ~Store() { clear(); }
  Store(const Store&) = delete;
  Store& operator=(const Store&) = delete;

  // at least n slots (new slots: no key, generation 0)
  void reserve_slots(size_t n) {
    if (slots_.size() < n) slots_.resize(n);
  }
  size_t n_slots() const { return slots_.size(); }

  // the slot holds exactly these pieces: the piece count and sizes first,
  // then the bytes
  bool match(size_t slot, const Seg* segs, int n_segs) const {
    if (slot >= slots_.size()) return false;
    const Slot& s = slots_[slot];
    if (!s.valid || (int)s.sizes.size() != n_segs) return false;
    for (int k = 0; k < n_segs; ++k)
      if (s.sizes[(size_t)k] != segs[k].n) return false;
    const unsigned char* at = s.bytes.data();
    for (int k = 0; k < n_segs; ++k) {
      if (segs[k].n && memcmp(at, segs[k].p, segs[k].n) != 0) return false;
      at += segs[k].n;
    }
    return true;
  }

  // the slot's key replaced by a copy of these pieces; false (the slot left
  // without a key) when the copy would take the process past the cap.  Slots
  // of one store may be stored from different threads at once.
  bool store(size_t slot, const Seg* segs, int n_segs) {
    if (slot >= slots_.size()) return false;
    Slot& s = slots_[slot];
    size_t bytes = 0;
    for (int k = 0; k < n_segs; ++k) bytes += segs[k].n;
    const int64_t old = s.valid || !s.bytes.empty() ? (int64_t)s.bytes.size() : 0;
    const int64_t delta = (int64_t)bytes - old;
    s.valid = false;
    if (total_->fetch_add(delta, std::memory_order_relaxed) + delta > cap_) {
      total_->fetch_sub(delta + old, std::memory_order_relaxed);   // (the old copy goes too)
      std::vector<unsigned char>().swap(s.bytes);
      s.sizes.clear();
      return false;
    }
    if (bytes < s.bytes.capacity() / 2) std::vector<unsigned char>().swap(s.bytes);   // (a shrunk key gives memory back)
    s.bytes.resize(bytes);
    s.sizes.resize((size_t)n_segs);
    unsigned char* at = s.bytes.data();
    for (int k = 0; k < n_segs; ++k) {
      s.sizes[(size_t)k] = segs[k].n;
      if (segs[k].n) memcpy(at, segs[k].p, segs[k].n);
      at += segs[k].n;
    }
    s.valid = true;
    return true;
  }

  // the slot's key is no longer evidence (its bytes stay charged until the
  // next store or clear)
  void invalidate(size_t slot) {
    if (slot < slots_.size()) slots_[slot].valid = false;
  }
  bool valid(size_t slot) const { return slot < slots_.size() && slots_[slot].valid; }

  uint64_t gen(size_t slot) const { return slot < slots_.size() ? slots_[slot].gen : 0; }
  void set_gen(size_t slot, uint64_t g) {
    if (slot < slots_.size()) slots_[slot].gen = g;
  }

  // every key dropped and its bytes given back (generations too)
  void clear() {
    int64_t mine = 0;
    for (Slot& s : slots_) {
      mine += (int64_t)s.bytes.size();
      std::vector<unsigned char>().swap(s.bytes);
      s.sizes.clear();
      s.valid = false;
      s.gen = 0;
    }
    if (mine) total_->fetch_sub(mine, std::memory_order_relaxed);
  }

  // bytes this store is charged
  int64_t bytes() const {
    int64_t mine = 0;
    for (const Slot& s : slots_) mine += (int64_t)s.bytes.size();
    return mine;
  }

 private:
  struct Slot {
    std::vector<unsigned char> bytes;
    std::vector<size_t> sizes;
    uint64_t gen = 0;
    bool valid = false;
  };
  std::vector<Slot> slots_;
  std::atomic<int64_t>* total_;
  int64_t cap_;
};

}  // namespace tpe_keystore
