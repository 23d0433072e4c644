// layout.hpp — where the host puts things in the handles' device scratch: the
// hand-off words of dqz_learner::sync and dqz_meta::arrive by name, and the
// carver of the handles' one allocation.  Plain host C++ (no HIP), so
// tests/layout_check.cpp compiles it alone.
#pragma once
#include <cstddef>
#include <cstdint>

namespace dqz {

constexpr int kWordStride = 64;  // ints between two hand-off words: Handoff::kStride (asserted in learner_impl.hpp)

// One in-launch hand-off (common.hpp Handoff): its arrival and ack words as offsets in ints, the arrivals a wait
// needs, the consumers that pass it, and whether its waits take the learner's spin_max or keep Handoff's default.
struct HandoffWords {
  int64_t cnt, ack;
  int need, consumers;
  bool learner_spin;
};

// dqz_learner::sync of a learner configured for batch B (not a call's n): one word per sample and side (Z n <= 3 B
// samples in a forward), then the error word every launch shares (dqz_learner_sync_status).
struct SyncLayout {
  int64_t B;
  constexpr int64_t word(int64_t w) const { return w * kWordStride; }
  constexpr HandoffWords dy2() const { return {word(0), word(B), 8, 16, true}; }  // conv3 dX -> conv2 dX
  constexpr HandoffWords fwd_y1(int jobs) const { return {word(2 * B), word(5 * B), 4, jobs, false}; }  // conv1 -> conv2
  constexpr HandoffWords fwd_y2(int jobs) const { return {word(8 * B), word(11 * B), jobs, jobs, false}; }
  constexpr HandoffWords dy1() const { return {word(14 * B), word(15 * B), 8, 8, true}; }  // conv2 dX -> conv1 dW
  constexpr int64_t err() const { return word(16 * B); }
  constexpr int64_t ints() const { return word(16 * B + 3) + 64; }  // the allocation, and what a reset clears
};

// dqz_meta::arrive, in words (x kWordStride ints); all zero between launches
enum MetaWord {
  kMetaReseed,     // meta_adam_chunks_kernel's re-seed arrival counter
  kMetaDdot1Cnt,   // the HVP's ddot1 hand-off
  kMetaDdot1Ack,
  kMetaAdamEntry,  // the Adam entry counter
  kMetaErr,        // the meta-level error word (dqz_meta_sync_status)
  kMetaWords
};

// One buffer of a handle's scratch: where its pointer is kept, and its size in floats.
struct Carve {
  void** pp;
  int64_t n;
  template <class T>
  Carve(T** p, int64_t n_floats) : pp(reinterpret_cast<void**>(p)), n(n_floats) {}
};

// Consecutive blocks in table order, each rounded up to 64 floats.  Returns the total in floats; with a base (the
// allocation) it also sets the pointers.
template <size_t N>
int64_t carve(const Carve (&bufs)[N], float* base) {
  int64_t off = 0;
  for (const Carve& b : bufs) {
    if (base) *b.pp = base + off;
    off += (b.n + 63) / 64 * 64;
  }
  return off;
}

}  // namespace dqz
