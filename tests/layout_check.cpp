// layout_check.cpp — host-only check of csrc/layout.hpp (tests/test_layout_cpu.py
// compiles and runs it): the named hand-off words against the layout's
// formulas written out, and the scratch carver over a made-up table.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "layout.hpp"

using namespace dqz;

static int g_bad = 0;
#define CHECK(cond)                                           \
  do {                                                        \
    if (!(cond)) {                                            \
      std::printf("line %d: %s is false\n", __LINE__, #cond); \
      ++g_bad;                                                \
    }                                                         \
  } while (0)

int main() {
  static_assert(kWordStride == 64, "Handoff::kStride");
  for (int64_t B : {1, 3, 32, 256}) {
    const SyncLayout s{B};
    for (int jobs : {4, 8}) {
      // {cnt, ack, arrivals needed, consumers, learner's spin_max} as the kernels' launches had them written out
      const HandoffWords want[] = {{0, B * 64, 8, 16, true},                                  // dy2
                                   {2 * B * 64, 2 * B * 64 + 3 * B * 64, 4, jobs, false},     // y1: 2B, 5B
                                   {2 * B * 64 + 6 * B * 64, 2 * B * 64 + 9 * B * 64, jobs, jobs, false},  // y2: 8B, 11B
                                   {14 * B * 64, 15 * B * 64, 8, 8, true}};               // dy1
      const HandoffWords got[] = {s.dy2(), s.fwd_y1(jobs), s.fwd_y2(jobs), s.dy1()};
      for (int i = 0; i < 4; ++i) {
        CHECK(got[i].cnt == want[i].cnt && got[i].ack == want[i].ack);
        CHECK(got[i].need == want[i].need && got[i].consumers == want[i].consumers);
        CHECK(got[i].learner_spin == want[i].learner_spin);
        // each side's B (backward) or 3 B (forward) words stop before the next range starts
        const int64_t span = (i == 0 || i == 3 ? B : 3 * B) * 64;
        CHECK(got[i].ack == got[i].cnt + span);
        CHECK(got[i].ack + span <= (i < 3 ? got[i + 1].cnt : s.err()));
      }
    }
    CHECK(s.fwd_y1(4).ack == 5 * B * 64 && s.fwd_y2(4).cnt == 8 * B * 64 && s.fwd_y2(4).ack == 11 * B * 64);
    CHECK(s.err() == 16 * B * 64);
    CHECK(s.ints() == (16 * B + 3) * 64 + 64);
    CHECK(s.err() + 1 <= s.ints());
    CHECK(s.word(B - 1) == (B - 1) * 64);  // a sample's word within a range
  }
  CHECK(kMetaReseed == 0);
  CHECK(kMetaDdot1Cnt == 1);
  CHECK(kMetaDdot1Ack == 2);
  CHECK(kMetaAdamEntry == 3);
  CHECK(kMetaErr == 4);
  CHECK(kMetaWords == 5);

  // the carver: pointers of several types, sizes that are and are not
  // multiples of 64 floats, empty buffers among them
  float* a = nullptr;
  int32_t* b = nullptr;
  double* c = nullptr;
  uint8_t* d = nullptr;
  float *e = nullptr, *f = nullptr, *g = nullptr;
  const int64_t n[] = {1, 64, 65, 0, 1000, 0, 4096};
  const Carve bufs[] = {{&a, n[0]}, {&b, n[1]}, {&c, n[2]}, {&d, n[3]}, {&e, n[4]}, {&f, n[5]}, {&g, n[6]}};
  int64_t want = 0;
  for (int64_t k : n) want += (k + 63) / 64 * 64;
  CHECK(carve(bufs, nullptr) == want);
  CHECK(a == nullptr && g == nullptr);  // the sizing pass sets nothing
  static float block[64 + 64 + 128 + 0 + 1024 + 0 + 4096];
  CHECK((int64_t)(sizeof(block) / sizeof(block[0])) == want);
  CHECK(carve(bufs, block) == want);
  const float* at[] = {a, (float*)b, (float*)c, (float*)d, e, f, g};
  CHECK(at[0] == block);
  for (int i = 0; i < 7; ++i) {
    CHECK((at[i] - block) % 64 == 0);                                          // aligned
    if (i > 0) CHECK(at[i] - at[i - 1] == (n[i - 1] + 63) / 64 * 64);          // in order, rounded, no gap
    if (i > 0) CHECK(at[i] >= at[i - 1] + n[i - 1]);                           // no overlap
    CHECK(at[i] + n[i] <= block + want);                                       // inside the allocation
  }
  if (g_bad == 0) std::printf("layout ok\n");
  return g_bad ? 1 : 0;
}
