// learner.hip — everything of libdqz but the learner step's kernels (those
// are learner_step.hip's code object; common.hpp, "Two translation units"):
// the replay-side device code (frame store puts and gathers, the uniform,
// learned-logit and prioritized samplers, sum trees), the MGSC meta-update
// and its HVP, Atari preprocessing, the optimizers applied to a finished
// gradient (Adam, plain RMSProp, global-norm clipping), the categorical (C51)
// and quantile (QR-DQN) heads the learner step launches in place of its own, the
// Rainbow agent's noisy dueling network around the categorical head,
// and the C-ABI entries that drive them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <functional>
#include <cmath>
#include <vector>
#include <cstdlib>
#include <cstring>

#include "learner_impl.hpp"
#include "meta.hpp"
#include "hvp.hpp"
#include "preprocess.hpp"
#include "census.hpp"
#include "optim.hpp"
#include "c51.hpp"
#include "qr.hpp"
#include "rainbow.hpp"

using namespace dqz;

// the meta-update's tangent launch takes conv1's dynamic LDS
static int g_meta_attr_done = 0;

static int init_meta_attrs() {
  if (g_meta_attr_done) return DQZ_OK;
  DQZ_HIP(hipFuncSetAttribute((const void*)tangent_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)kConv1FwdSmem));
  g_meta_attr_done = 1;
  return DQZ_OK;
}

extern "C" {

const char* dqz_last_error(void) { return err_buf().c_str(); }

#ifndef DQZ_BUILD_ID
#define DQZ_BUILD_ID "unset"
#endif
const char* dqz_build_id(void) { return DQZ_BUILD_ID; }

int dqz_store_put(const dqz_store* S, const dqz_transition_put* t, const uint8_t* frames, void* stream) {
  if (int rc = check_store(S)) return rc;
  if (!t) return fail(DQZ_ERR_INVALID, "null transition");
  if (t->slot < 0 || t->slot >= S->capacity)
    return fail(DQZ_ERR_INVALID, "slot %lld out of range [0, %lld)", (long long)t->slot, (long long)S->capacity);
  if (t->num_frames < 0 || t->num_frames > 8) return fail(DQZ_ERR_INVALID, "num_frames must be in [0, 8]");
  for (int i = 0; i < 8; ++i)
    if (t->fidx[i] < -1 || t->fidx[i] >= S->num_frames) return fail(DQZ_ERR_INVALID, "fidx[%d] out of range", i);
  for (int i = 0; i < t->num_frames; ++i)
    if (t->frame_rows[i] < 0 || t->frame_rows[i] >= S->num_frames)
      return fail(DQZ_ERR_INVALID, "frame_rows[%d] out of range", i);
  const void* dframes = nullptr;
  if (t->num_frames > 0) {
    if (!frames) return fail(DQZ_ERR_INVALID, "null frames");
    if (int rc = device_view(frames, &dframes, "frames")) return rc;
    if (reinterpret_cast<uintptr_t>(dframes) % 16) return fail(DQZ_ERR_INVALID, "frames must be 16-byte aligned");
  }
  hipLaunchKernelGGL(store_put_kernel, dim3(t->num_frames > 0 ? t->num_frames : 1), dim3(256), 0,
                     (hipStream_t)stream, const_cast<uint8_t*>(S->frames), const_cast<int32_t*>(S->fidx),
                     const_cast<int32_t*>(S->action), const_cast<float*>(S->reward),
                     const_cast<float*>(S->discount), *t, static_cast<const uint8_t*>(dframes));
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

int dqz_store_jumble(const dqz_store* S, const dqz_jumble* j, void* stream) {
  if (int rc = check_store(S)) return rc;
  if (!j) return fail(DQZ_ERR_INVALID, "null jumble");
  const int64_t slots[6] = {j->slot, j->src_s_tm1, j->src_action, j->src_reward, j->src_discount, j->src_s_t};
  for (int i = 0; i < 6; ++i)
    if (slots[i] < 0 || slots[i] >= S->capacity)
      return fail(DQZ_ERR_INVALID, "jumble slot %lld out of range [0, %lld)", (long long)slots[i],
                  (long long)S->capacity);
  for (int i = 0; i < 8; ++i) {
    if (j->frame_rows[i] < 0 || j->frame_rows[i] >= S->num_frames)
      return fail(DQZ_ERR_INVALID, "frame_rows[%d] out of range", i);
    for (int k = 0; k < i; ++k)
      if (j->frame_rows[k] == j->frame_rows[i])
        return fail(DQZ_ERR_INVALID, "frame_rows[%d] repeats frame_rows[%d]", i, k);
  }
  hipLaunchKernelGGL(store_jumble_kernel, dim3(8), dim3(256), 0, (hipStream_t)stream, const_cast<uint8_t*>(S->frames),
                     const_cast<int32_t*>(S->fidx), const_cast<int32_t*>(S->action), const_cast<float*>(S->reward),
                     const_cast<float*>(S->discount), *j);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

int dqz_sample_uniform(int64_t base, int64_t size, int64_t capacity, int n, uint64_t seed, uint64_t* counter_dev,
                       int32_t* out_slots, void* stream) {
  if (!counter_dev || !out_slots) return fail(DQZ_ERR_INVALID, "null argument");
  if (size < 1) return fail(DQZ_ERR_INVALID, "cannot sample from an empty replay (size=%lld)", (long long)size);
  if (capacity < size) return fail(DQZ_ERR_INVALID, "size exceeds capacity");
  if (n < 1 || n > 65536) return fail(DQZ_ERR_INVALID, "n out of range");
  if (base < 0) return fail(DQZ_ERR_INVALID, "base must be >= 0");
  hipLaunchKernelGGL(sample_uniform_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, base % capacity, size, capacity, n, seed,
                     counter_dev, out_slots);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

int dqz_gather_stacks(const dqz_store* S, const int32_t* slots, int n, int which, uint8_t* out, void* stream) {
  if (int rc = check_store(S)) return rc;
  if (!slots || !out) return fail(DQZ_ERR_INVALID, "null argument");
  if (n < 0) return fail(DQZ_ERR_INVALID, "n must be >= 0");
  if (int rc = check_which(which)) return rc;
  if (n == 0) return DQZ_OK;
  const int64_t total = (int64_t)n * FB;
  hipLaunchKernelGGL(gather_stacks_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     S->frames, S->fidx, slots, n, which, out);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

// ---------------------------------------------------------------------------
// learned-logit and prioritized samplers

struct dqz_logit_buffer {
  int64_t capacity;
  int nblocks, max_queries;
  void* block;  // double csum[nblocks] | MaxSum part[nblocks] | int dirty[nblocks] | float lse | LogitRun | sync |
                // exact mode: double csum_x[nblocks] | float part_x[nblocks] | bsum_x[nbuf] | scal_x[2] | programs
  double* csum;    // per-chunk sums of the sampling terms (sampling.hpp chunk_sum)
  MaxSum* part;
  int* dirty;      // chunks a writer changed, for chunk_sums_kernel
  float* lse;
  LogitRun* run;   // running log-sum-exp (sampling.hpp)
  int* sync;       // (x SampleSync::kStride) [1] softmax_sample_kernel's done word, [3] / [4] the arrival
                   // tickets of the exact preparation's first / second launch (npx_take_ticket)
  // exact mode (dqz_logits_sample_exact): chunk sums of the exact terms,
  // chunk maxima, numpy-buffer sums, {c, lse}
  int nbuf;
  double* csum_x;
  float *part_x, *bsum_x, *scal_x;
  int *prog_full, *prog_last;  // npx_program of a full and of the last buffer
  bool run_known;  // host side: every write since the last scan went through the library
  int run_adds;    // running adds since the last scan
  void* census;    // dqz_logits_census: CensusScan[nblocks] | CensusMass[nblocks], allocated by its first call
};

// numpy's pairwise-summation recursion over one buffer of length L
// (sampling.hpp npx_bufsum_kernel's program): the leaves in order, then the
// internal additions grouped by height, each (dst, left, right).
static std::vector<int> npx_program(int L) {
  std::vector<int> lo, len;
  std::vector<std::array<int, 4>> ops;  // height, dst, a, b
  int nleaf = 0;
  std::function<void(int, int)> leaves = [&](int l, int m) {
    if (m <= NPX_LEAF) {
      lo.push_back(l);
      len.push_back(m);
      return;
    }
    int m2 = m / 2;
    m2 -= m2 % 8;
    leaves(l, m2);
    leaves(l + m2, m - m2);
  };
  leaves(0, L);
  nleaf = (int)lo.size();
  int next_leaf = 0, next = nleaf;
  std::function<std::pair<int, int>(int)> build = [&](int m) -> std::pair<int, int> {
    if (m <= NPX_LEAF) return {next_leaf++, 0};
    int m2 = m / 2;
    m2 -= m2 % 8;
    const auto a = build(m2);
    const auto b = build(m - m2);
    const int h = std::max(a.second, b.second) + 1, d = next++;
    ops.push_back({h, d, a.first, b.first});
    return {d, h};
  };
  const int root = build(L).first;
  std::stable_sort(ops.begin(), ops.end(), [](const std::array<int, 4>& x, const std::array<int, 4>& y) { return x[0] < y[0]; });
  const int nlev = ops.empty() ? 0 : ops.back()[0];
  std::vector<int> prog = {nleaf, nlev, root};
  prog.insert(prog.end(), lo.begin(), lo.end());
  prog.insert(prog.end(), len.begin(), len.end());
  size_t k = 0;
  for (int h = 1; h <= nlev + 1; ++h) {  // lev_off[h - 1] = first op of height h
    prog.push_back((int)k);
    while (k < ops.size() && ops[k][0] == h) ++k;
  }
  for (const auto& o : ops) prog.insert(prog.end(), {o[1], o[2], o[3]});
  if (prog.size() > (size_t)NPX_PROG || next > 2 * NPX_MAXLEAF) std::abort();
  return prog;
}

// 256-byte lines of a logit buffer's sync words: softmax_sample_kernel's three,
// then one per arrival ticket of the exact preparation.
constexpr int kLogitSyncLines = 5;
constexpr int kNpxTicketMax = 3, kNpxTicketSum = 4;

// Running adds between full re-scans of a logit buffer (bounds the running
// sum's drift; each scan reads the whole buffer once).
constexpr int kLogitReseed = 4096;

int dqz_logit_buffer_create(int64_t capacity, int max_queries, dqz_logit_buffer** out) {
  if (!out || capacity < 1 || max_queries < 1) return fail(DQZ_ERR_INVALID, "bad logit buffer arguments");
  if (capacity > ((int64_t)INT32_MAX + 1) * SM_CHUNK / 2) return fail(DQZ_ERR_INVALID, "capacity too large");
  dqz_logit_buffer* b = new dqz_logit_buffer();
  b->capacity = capacity;
  b->max_queries = max_queries;
  b->nblocks = (int)((capacity + SM_CHUNK - 1) / SM_CHUNK);
  const size_t head = (size_t)b->nblocks * (sizeof(MaxSum) + sizeof(double) + sizeof(int));
  const size_t sync_off = (head + 64 + sizeof(LogitRun) + 255) / 256 * 256;
  b->nbuf = (int)((capacity + NPX_BUF - 1) / NPX_BUF);
  const size_t x_off = sync_off + kLogitSyncLines * SampleSync::kStride * sizeof(int);  // 256-aligned
  const size_t prog_off = (x_off + (size_t)b->nblocks * (sizeof(double) + sizeof(float)) + (size_t)b->nbuf * sizeof(float) +
                            64 + 255) / 256 * 256;
  const size_t bytes = prog_off + 2 * NPX_PROG * sizeof(int);
  if (hipMalloc(&b->block, bytes) != hipSuccess) {
    delete b;
    return fail(DQZ_ERR_HIP, "hipMalloc of logit scratch failed");
  }
  if (hipMemset(b->block, 0, bytes) != hipSuccess) {
    (void)hipFree(b->block);
    delete b;
    return fail(DQZ_ERR_HIP, "hipMemset of logit scratch failed");
  }
  char* p = (char*)b->block;
  b->csum = (double*)p;
  b->part = (MaxSum*)(p + (size_t)b->nblocks * sizeof(double));
  b->dirty = (int*)(p + (size_t)b->nblocks * (sizeof(double) + sizeof(MaxSum)));
  b->lse = (float*)(p + head);
  b->run = (LogitRun*)(p + head + 64);
  b->sync = (int*)(p + sync_off);
  b->csum_x = (double*)(p + x_off);
  b->part_x = (float*)(p + x_off + (size_t)b->nblocks * sizeof(double));
  b->bsum_x = b->part_x + b->nblocks;
  b->scal_x = b->bsum_x + b->nbuf;
  b->prog_full = (int*)(p + prog_off);
  b->prog_last = b->prog_full + NPX_PROG;
  {
    const std::vector<int> full = npx_program(NPX_BUF), last = npx_program((int)(capacity - (int64_t)(b->nbuf - 1) * NPX_BUF));
    if (hipMemcpy(b->prog_full, full.data(), full.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(b->prog_last, last.data(), last.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipFree(b->block);
      delete b;
      return fail(DQZ_ERR_HIP, "hipMemcpy of the exact-mode programs failed");
    }
  }
  b->run_known = false;
  b->run_adds = 0;
  *out = b;
  return DQZ_OK;
}

int dqz_logit_buffer_destroy(dqz_logit_buffer* b) {
  if (!b) return DQZ_OK;
  if (b->block) (void)hipFree(b->block);
  if (b->census) (void)hipFree(b->census);
  delete b;
  return DQZ_OK;
}

// csum of the flagged chunks (dirty != null) or of all of them.
static int chunk_sums(dqz_logit_buffer* b, const float* logits, bool dirty_only, hipStream_t st) {
  hipLaunchKernelGGL(chunk_sums_kernel, dim3(b->nblocks), dim3(SM_THREADS), 0, st, logits, b->capacity, b->run,
                     b->csum, dirty_only ? b->dirty : nullptr);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

// Full two-pass log-sum-exp over the buffer (re-seeds the running state),
// then every chunk sum about the new shift.
static int logits_lse(dqz_logit_buffer* b, float* logits, int64_t clear_pos, int64_t write_pos, int64_t size,
                      float* lse_out, hipStream_t st) {
  hipLaunchKernelGGL(lse_partial_kernel, dim3(b->nblocks), dim3(SM_THREADS), 0, st, logits, b->capacity, b->part,
                     clear_pos);
  DQZ_HIP(hipGetLastError());
  hipLaunchKernelGGL(lse_final_kernel, dim3(1), dim3(SM_THREADS), 0, st, b->part, b->nblocks, lse_out ? lse_out : b->lse,
                     logits, write_pos, size, b->run);
  DQZ_HIP(hipGetLastError());
  if (int rc = chunk_sums(b, logits, false, st)) return rc;
  b->run_known = true;
  b->run_adds = 0;
  return DQZ_OK;
}

int dqz_logits_add(dqz_logit_buffer* b, float* logits, int64_t clear_pos, int64_t write_pos, int64_t size,
                   float* lse_out, void* stream) {
  if (!b || !logits) return fail(DQZ_ERR_INVALID, "null argument");
  if (write_pos < 0 || write_pos >= b->capacity || clear_pos >= b->capacity)
    return fail(DQZ_ERR_INVALID, "position out of range");
  if (size < 0) return fail(DQZ_ERR_INVALID, "size must be >= 0");
  hipStream_t st = (hipStream_t)stream;
  if (!b->run_known || b->run_adds >= kLogitReseed) {
    // the reservoir `replace` clear (logits[clear_pos] = -inf) happens inside pass 1
    if (int rc = logits_lse(b, logits, clear_pos, write_pos, size, lse_out, st)) return rc;
  } else {
    hipLaunchKernelGGL(logits_add_running_kernel, dim3(1), dim3(SM_THREADS), 0, st, logits, b->capacity, b->run,
                       b->csum, clear_pos, write_pos, size, lse_out ? lse_out : b->lse);
    DQZ_HIP(hipGetLastError());
    ++b->run_adds;
  }
  if (lse_out) DQZ_HIP(hipMemcpyAsync(b->lse, lse_out, sizeof(float), hipMemcpyDeviceToDevice, st));
  return DQZ_OK;
}

int dqz_logits_write(dqz_logit_buffer* b, float* logits, const int64_t* positions, const float* values, int n,
                     void* stream) {
  if (!b || !logits || (n > 0 && (!positions || !values))) return fail(DQZ_ERR_INVALID, "null argument");
  if (n < 0) return fail(DQZ_ERR_INVALID, "n must be >= 0");
  if (n == 0) return DQZ_OK;
  hipStream_t st = (hipStream_t)stream;
  if (!b->run_known) {  // no running state to keep: write, and the next use re-seeds
    hipLaunchKernelGGL(logits_scatter_kernel, dim3(1), dim3(64), 0, st, logits, positions, values, n);
    DQZ_HIP(hipGetLastError());
    return DQZ_OK;
  }
  hipLaunchKernelGGL(logits_write_kernel, dim3(1), dim3(SM_THREADS), 0, st, logits, b->capacity, b->run, b->dirty,
                     positions, values, n);
  DQZ_HIP(hipGetLastError());
  return chunk_sums(b, logits, true, st);
}

int dqz_logits_put(dqz_logit_buffer* b, float* logits, int64_t position, float value, void* stream) {
  if (!b || !logits) return fail(DQZ_ERR_INVALID, "null argument");
  if (position < 0 || position >= b->capacity) return fail(DQZ_ERR_INVALID, "position out of range");
  hipStream_t st = (hipStream_t)stream;
  if (!b->run_known) {
    hipLaunchKernelGGL(logits_scatter1_kernel, dim3(1), dim3(64), 0, st, logits, position, value);
    DQZ_HIP(hipGetLastError());
    return DQZ_OK;
  }
  hipLaunchKernelGGL(logits_put1_kernel, dim3(1), dim3(SM_THREADS), 0, st, logits, b->capacity, b->run, b->csum,
                     position, value);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

__global__ void logits_run_set_kernel(LogitRun* run, LogitRun v) {
  if (threadIdx.x == 0) *run = v;
}

int dqz_logits_run_get(dqz_logit_buffer* b, double* S, float* c, int* valid, int* known, int* adds, void* stream) {
  if (!b || !S || !c || !valid || !known || !adds) return fail(DQZ_ERR_INVALID, "null argument");
  hipStream_t st = (hipStream_t)stream;
  LogitRun r{0.0, 0.f, 0};
  DQZ_HIP(hipMemcpyAsync(&r, b->run, sizeof(LogitRun), hipMemcpyDeviceToHost, st));
  DQZ_HIP(hipStreamSynchronize(st));
  *S = r.S;
  *c = r.c;
  *valid = r.valid;
  *known = b->run_known ? 1 : 0;
  *adds = b->run_adds;
  return DQZ_OK;
}

int dqz_logits_run_set(dqz_logit_buffer* b, const float* logits, double S, float c, int valid, int known, int adds,
                       void* stream) {
  if (!b || !logits) return fail(DQZ_ERR_INVALID, "null argument");
  if (adds < 0) return fail(DQZ_ERR_INVALID, "adds must be >= 0");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(logits_run_set_kernel, dim3(1), dim3(64), 0, st, b->run, LogitRun{S, c, valid ? 1 : 0});
  DQZ_HIP(hipGetLastError());
  b->run_known = known != 0 && valid != 0;
  b->run_adds = adds;
  // the chunk sums are a function of (logits, c): the restored state's
  if (b->run_known) return chunk_sums(b, logits, false, st);
  return DQZ_OK;
}

int dqz_logits_invalidate(dqz_logit_buffer* b) {
  if (!b) return fail(DQZ_ERR_INVALID, "null argument");
  b->run_known = false;
  return DQZ_OK;
}

// The samplers use the running state and its chunk sums: seed both with a
// scan first when the host cannot vouch for them.
static int ensure_run(dqz_logit_buffer* b, const float* logits, hipStream_t st) {
  if (b->run_known) return DQZ_OK;
  return logits_lse(b, const_cast<float*>(logits), -1, -1, 0, nullptr, st);
}

static int logits_sample_impl(dqz_logit_buffer* b, const float* logits, uint64_t seed, uint64_t* counter_dev,
                              const double* uniforms, int n, int32_t* out_slots, int64_t* out_idx, hipStream_t st) {
  if (!b || !logits || (!uniforms && !counter_dev) || (!out_slots && !out_idx))
    return fail(DQZ_ERR_INVALID, "null argument");
  if (n < 1 || n > 65535) return fail(DQZ_ERR_INVALID, "n out of range");
  if (out_slots && b->capacity > INT32_MAX) return fail(DQZ_ERR_INVALID, "int32 slots need capacity < 2^31");
  if (int rc = ensure_run(b, logits, st)) return rc;
  hipLaunchKernelGGL(softmax_sample_kernel, dim3(n), dim3(SM_THREADS), 0, st, logits, b->capacity, b->run, b->csum,
                     b->nblocks, SampleSync{b->sync}, seed, counter_dev, uniforms, n, out_slots, out_idx);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

int dqz_logits_sample(dqz_logit_buffer* b, const float* logits, const double* uniforms, int n, int64_t* out_idx,
                      void* stream) {
  if (!uniforms || !out_idx) return fail(DQZ_ERR_INVALID, "null argument");
  return logits_sample_impl(b, logits, 0, nullptr, uniforms, n, nullptr, out_idx, (hipStream_t)stream);
}

int dqz_logits_sample_slots(dqz_logit_buffer* b, const float* logits, uint64_t seed, uint64_t* counter_dev,
                            const double* uniforms, int n, int32_t* out_slots, int64_t* out_idx, void* stream) {
  return logits_sample_impl(b, logits, seed, counter_dev, uniforms, n, out_slots, out_idx, (hipStream_t)stream);
}

// numpy's float32 logsumexp of the whole buffer -> b->scal_x[1] (c in [0]):
// two launches, each finished by its last workgroup to arrive.
static int npx_lse(dqz_logit_buffer* b, const float* logits, hipStream_t st) {
  hipLaunchKernelGGL(npx_max_kernel, dim3(b->nblocks), dim3(SM_THREADS), 0, st, logits, b->capacity, b->part_x,
                     b->scal_x, b->sync + kNpxTicketMax * SampleSync::kStride);
  DQZ_HIP(hipGetLastError());
  hipLaunchKernelGGL(npx_bufsum_kernel, dim3(b->nbuf), dim3(SM_THREADS), 0, st, logits, b->capacity, b->scal_x,
                     b->bsum_x, b->prog_full, b->prog_last, b->sync + kNpxTicketSum * SampleSync::kStride);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

// The exact mode's preparation, three launches: the logsumexp, then the
// chunk sums of p = np_expf(x - lse) -> b->csum_x (and p itself, if asked).
static int npx_prepare(dqz_logit_buffer* b, const float* logits, float* p_out, hipStream_t st) {
  if (int rc = npx_lse(b, logits, st)) return rc;
  hipLaunchKernelGGL(npx_chunk_kernel, dim3(b->nblocks), dim3(SM_THREADS), 0, st, logits, b->capacity, b->scal_x,
                     b->csum_x, p_out);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

int dqz_logits_add_exact(dqz_logit_buffer* b, float* logits, int64_t clear_pos, int64_t write_pos, int64_t size,
                         void* stream) {
  if (!b || !logits) return fail(DQZ_ERR_INVALID, "null argument");
  if (write_pos < 0 || write_pos >= b->capacity || clear_pos >= b->capacity)
    return fail(DQZ_ERR_INVALID, "position out of range");
  if (size < 0) return fail(DQZ_ERR_INVALID, "size must be >= 0");
  hipStream_t st = (hipStream_t)stream;
  if (clear_pos >= 0) {
    hipLaunchKernelGGL(npx_clear_kernel, dim3(1), dim3(64), 0, st, logits, clear_pos);
    DQZ_HIP(hipGetLastError());
  }
  if (size > 0)
    if (int rc = npx_lse(b, logits, st)) return rc;
  hipLaunchKernelGGL(npx_add_kernel, dim3(1), dim3(64), 0, st, logits, write_pos, size, b->scal_x);
  DQZ_HIP(hipGetLastError());
  b->run_known = false;  // the running state did not follow this write
  return DQZ_OK;
}

int dqz_logits_sample_exact(dqz_logit_buffer* b, const float* logits, const double* uniforms, int n, int64_t* out_idx,
                            float* p_out, void* stream) {
  if (!b || !logits) return fail(DQZ_ERR_INVALID, "null argument");
  if (n < 0 || n > 65535) return fail(DQZ_ERR_INVALID, "n out of range");
  if (n > 0 && (!uniforms || !out_idx)) return fail(DQZ_ERR_INVALID, "null argument");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = npx_prepare(b, logits, p_out, st)) return rc;
  if (n > 0) {
    hipLaunchKernelGGL(npx_sample_kernel, dim3(n), dim3(SM_THREADS), 0, st, logits, b->capacity, b->scal_x, b->csum_x,
                       b->nblocks, uniforms, out_idx);
    DQZ_HIP(hipGetLastError());
  }
  return DQZ_OK;
}

int dqz_logits_probs(dqz_logit_buffer* b, const float* logits, float* p_out, float* lse_out, void* stream) {
  if (!b || !logits || !p_out) return fail(DQZ_ERR_INVALID, "null argument");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = ensure_run(b, logits, st)) return rc;
  hipLaunchKernelGGL(logit_terms_kernel, dim3(b->nblocks), dim3(SM_THREADS), 0, st, logits, b->capacity, b->run,
                     b->csum, b->nblocks, p_out, (float*)nullptr, lse_out, (float*)nullptr);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

int dqz_logits_census(dqz_logit_buffer* b, const float* logits, const uint8_t* flags, int64_t left_head, int64_t size,
                      dqz_census* acc_dev, void* stream) {
  if (!b || !logits || !flags || !acc_dev) return fail(DQZ_ERR_INVALID, "null argument");
  if (left_head < 0 || left_head >= b->capacity)
    return fail(DQZ_ERR_INVALID, "left_head %lld out of range [0, %lld)", (long long)left_head, (long long)b->capacity);
  if (size < 0 || size > b->capacity)
    return fail(DQZ_ERR_INVALID, "size %lld out of range [0, %lld]", (long long)size, (long long)b->capacity);
  if (!b->census)
    DQZ_HIP(hipMalloc(&b->census, (size_t)b->nblocks * (sizeof(CensusScan) + sizeof(CensusMass))));
  hipStream_t st = (hipStream_t)stream;
  CensusScan* scan = (CensusScan*)b->census;
  CensusMass* mass = (CensusMass*)(scan + b->nblocks);
  const int nparts = (int)((size + SM_CHUNK - 1) / SM_CHUNK);  // <= nblocks
  if (nparts > 0) {
    hipLaunchKernelGGL(census_scan_kernel, dim3(nparts), dim3(SM_THREADS), 0, st, logits, flags, b->capacity, left_head,
                       size, scan);
    DQZ_HIP(hipGetLastError());
    hipLaunchKernelGGL(census_mass_kernel, dim3(nparts), dim3(SM_THREADS), 0, st, logits, flags, b->capacity, left_head,
                       size, scan, nparts, mass);
    DQZ_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(census_final_kernel, dim3(1), dim3(SM_THREADS), 0, st, logits, flags, b->capacity, left_head, size,
                     scan, mass, nparts, acc_dev);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

int dqz_logits_terms(dqz_logit_buffer* b, const float* logits, float* t_out, double* csum_out, float* c_out,
                     void* stream) {
  if (!b || !logits || !t_out) return fail(DQZ_ERR_INVALID, "null argument");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = ensure_run(b, logits, st)) return rc;
  hipLaunchKernelGGL(logit_terms_kernel, dim3(b->nblocks), dim3(SM_THREADS), 0, st, logits, b->capacity, b->run,
                     b->csum, b->nblocks, (float*)nullptr, t_out, (float*)nullptr, c_out);
  DQZ_HIP(hipGetLastError());
  if (csum_out)
    DQZ_HIP(hipMemcpyAsync(csum_out, b->csum, sizeof(double) * b->nblocks, hipMemcpyDeviceToDevice, st));
  return DQZ_OK;
}

int dqz_learner_step_logits(dqz_learner* L, const dqz_params* P, const dqz_store* S, dqz_logit_buffer* buf,
                            const float* logits, uint64_t seed, uint64_t* counter_dev, const double* uniforms,
                            int32_t* slots_out, void* stream) {
  if (!L || !buf || !logits || (!counter_dev && !uniforms) || !slots_out)
    return fail(DQZ_ERR_INVALID, "null argument");
  if (L->cfg.algo == DQZ_ALGO_PER) return fail(DQZ_ERR_INVALID, "PER samples by priority, not by learned logits");
  if (buf->capacity > INT32_MAX) return fail(DQZ_ERR_INVALID, "int32 slots need capacity < 2^31");
  hipStream_t st = (hipStream_t)stream;
  if (int rc = ensure_run(buf, logits, st)) return rc;
  SoftmaxDraw sm{logits, buf->capacity, buf->run, buf->csum, buf->nblocks,
                 seed,   uniforms ? nullptr : counter_dev,    uniforms,  slots_out};
  return step_impl(L, P, S, {.sm = &sm}, stream);
}

int dqz_learner_step_logits_exact(dqz_learner* L, const dqz_params* P, const dqz_store* S, dqz_logit_buffer* buf,
                                  const float* logits, uint64_t seed, uint64_t* counter_dev, const double* uniforms,
                                  int32_t* slots_out, void* stream) {
  if (!L || !buf || !logits || !slots_out) return fail(DQZ_ERR_INVALID, "null argument");
  if (!counter_dev == !uniforms) return fail(DQZ_ERR_INVALID, "give exactly one of counter_dev and uniforms");
  if (L->cfg.algo == DQZ_ALGO_PER) return fail(DQZ_ERR_INVALID, "PER samples by priority, not by learned logits");
  if (buf->capacity > INT32_MAX) return fail(DQZ_ERR_INVALID, "int32 slots need capacity < 2^31");
  SoftmaxDrawExact smx{logits, buf->capacity, buf->scal_x, buf->csum_x, buf->nblocks,
                       seed,   counter_dev,   uniforms,    slots_out};
  const StepRequest r{.smx = &smx};
  // the step's own checks first: nothing is enqueued for a call that fails
  if (int rc = check_step(L, P, S, r)) return rc;
  if (int rc = npx_prepare(buf, logits, nullptr, (hipStream_t)stream)) return rc;
  return step_enqueue(L, P, S, r, stream);
}

int dqz_uniform_philox(uint64_t seed, uint64_t* counter_dev, int n, double* out, void* stream) {
  if (!counter_dev || !out || n < 1 || n > 65536) return fail(DQZ_ERR_INVALID, "bad argument");
  hipLaunchKernelGGL(philox_uniform_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, seed, counter_dev, n, out);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

int dqz_sumtree_set(double* tree, int64_t cap, const int64_t* idx, const double* values, int n, void* stream) {
  if (!tree || !idx || !values) return fail(DQZ_ERR_INVALID, "null argument");
  if (cap < 1 || (cap & (cap - 1))) return fail(DQZ_ERR_INVALID, "cap must be a power of two");
  if (n < 0 || n > 65536) return fail(DQZ_ERR_INVALID, "n out of range");
  if (n == 0) return DQZ_OK;
  const int levels = tree_levels(cap);
  if (n <= ST_FAST && levels <= 32)
    hipLaunchKernelGGL(sumtree_set_small_kernel, dim3(1), dim3(ST_FAST), 0, (hipStream_t)stream, tree, cap, levels,
                       idx, values, n);
  else
    hipLaunchKernelGGL(sumtree_set_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, tree, cap, levels, idx,
                       values, n);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

int dqz_per_write_back(dqz_learner* L, double* tree, int64_t cap, const int32_t* slots, double alpha,
                       double* max_seen_dev, void* stream) {
  if (!L || !tree || !slots || !max_seen_dev) return fail(DQZ_ERR_INVALID, "null argument");
  if (cap < 1 || (cap & (cap - 1))) return fail(DQZ_ERR_INVALID, "cap must be a power of two");
  const int n = L->cfg.batch;
  const int levels = tree_levels(cap);
  if (n > ST_FAST || levels > 32) return fail(DQZ_ERR_INVALID, "batch must be <= %d and cap <= 2^32", ST_FAST);
  hipLaunchKernelGGL(per_write_back_kernel, dim3(1), dim3(ST_FAST), 0, (hipStream_t)stream, tree, cap, levels, slots,
                     L->td, alpha, n, max_seen_dev);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

int dqz_sumtree_query(const double* tree, int64_t cap, const double* targets, int n, int64_t* out, void* stream) {
  if (!tree || !targets || !out) return fail(DQZ_ERR_INVALID, "null argument");
  if (cap < 1 || (cap & (cap - 1))) return fail(DQZ_ERR_INVALID, "cap must be a power of two");
  if (n < 0) return fail(DQZ_ERR_INVALID, "n must be >= 0");
  if (n == 0) return DQZ_OK;
  hipLaunchKernelGGL(sumtree_query_kernel, dim3((n + 7) / 8), dim3(256), 0, (hipStream_t)stream, tree, cap,
                     tree_levels(cap), targets, n, out);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

// The prioritized draw's checks on its filled kernel argument, whose tree levels this sets.  (The learner
// step's fused draw has n = its batch <= MAXB, so the n check only ever refuses a dqz_per_sample call.)
static int per_draw_args(PerSampleArgs* a) {
  if (!a->inj_u && !a->counter) return fail(DQZ_ERR_INVALID, "Philox draws need counter_dev");
  if ((a->inj_u == nullptr) != (a->inj_uniform == nullptr))
    return fail(DQZ_ERR_INVALID, "injected_uniform and injected_u go together");
  if (a->cap < a->capacity || (a->cap & (a->cap - 1))) return fail(DQZ_ERR_INVALID, "cap must be a power of two >= capacity");
  if (a->size < 1) return fail(DQZ_ERR_INVALID, "No IDs to sample.");
  if (a->n < 1 || a->n > 1024) return fail(DQZ_ERR_INVALID, "n must be in [1, 1024]");
  if (!(a->beta >= 0.0 && a->beta <= 1.0)) return fail(DQZ_ERR_INVALID, "Require 0 <= exponent <= 1.");
  if (!(a->usp >= 0.0 && a->usp <= 1.0)) return fail(DQZ_ERR_INVALID, "Require 0 <= uniform_sample_probability <= 1.");
  a->levels = tree_levels(a->cap);
  return DQZ_OK;
}

int dqz_per_sample(const double* tree, int64_t cap, int64_t live_base, int64_t size, int64_t capacity, int n,
                   double usp, double beta, int normalize, uint64_t seed, uint64_t* counter_dev,
                   const int32_t* injected_uniform, const double* injected_u, const int32_t* index_to_slot,
                   int32_t* out_indices, int32_t* out_slots, float* out_weights, double* out_probs, void* stream) {
  if (!tree || !out_slots || !out_weights) return fail(DQZ_ERR_INVALID, "null argument");
  PerSampleArgs a{.tree = tree, .cap = cap, .live_base = live_base, .size = size, .capacity = capacity, .n = n,
                  .usp = usp, .beta = beta, .normalize = normalize, .seed = seed, .counter = counter_dev,
                  .inj_uniform = injected_uniform, .inj_u = injected_u, .index_to_slot = index_to_slot,
                  .out_indices = out_indices, .out_slots = out_slots, .out_weights = out_weights,
                  .out_probs = out_probs};
  if (int rc = per_draw_args(&a)) return rc;
  hipLaunchKernelGGL(per_sample_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

// The fused prioritized step's draw and write-back (dqz_learner_step_per_draw, dqz_learner_step_opt_per_draw):
// d's checks, then *a and *wb, the request's pd and wb.
static int per_draw_request(const dqz_learner* L, const dqz_per_draw* d, PerSampleArgs* a, PerWbArgs* wb) {
  if (!L || !d || !d->tree || !d->out_indices || !d->out_slots || !d->out_probs || !d->max_seen_dev)
    return fail(DQZ_ERR_INVALID, "null argument");
  if (L->cfg.algo != DQZ_ALGO_PER) return fail(DQZ_ERR_INVALID, "the learner is not a PER learner");
  *a = PerSampleArgs{.tree = d->tree, .cap = d->cap, .live_base = d->live_base, .size = d->size,
                     .capacity = d->capacity, .n = L->cfg.batch, .usp = d->uniform_sample_probability,
                     .beta = d->importance_sampling_exponent, .normalize = d->normalize_weights, .seed = d->seed,
                     .counter = d->counter_dev, .inj_uniform = d->injected_uniform, .inj_u = d->injected_u,
                     .index_to_slot = d->index_to_slot, .out_indices = d->out_indices, .out_slots = d->out_slots,
                     .out_weights = d->out_weights, .out_probs = d->out_probs};
  if (int rc = per_draw_args(a)) return rc;
  if (!per_wb_args(L, d->tree, d->cap, d->out_indices, d->alpha, d->max_seen_dev, wb))
    return fail(DQZ_ERR_INVALID, "the fused PER step takes batch <= 64 and cap <= 2^%d", PWB_LEVELS);
  return DQZ_OK;
}

int dqz_learner_step_per_draw(dqz_learner* L, const dqz_params* P, const dqz_store* S, const dqz_per_draw* d,
                              void* stream) {
  PerSampleArgs a;
  PerWbArgs wb;
  if (int rc = per_draw_request(L, d, &a, &wb)) return rc;
  return step_impl(L, P, S, {.pd = &a, .wb = &wb}, stream);
}

// ---------------------------------------------------------------------------
// optimizers on a finished gradient (optim.hpp)

struct dqz_optimizer {
  dqz_optimizer_config cfg;
  int64_t total;
  OptLeavesRb lv;     // every layout in the widest table: leaves the layout does not have are empty
  int nblocks;        // workgroups of the apply launch
  int nparts;         // workgroups of the norm launch = its partials
  float* grad;        // [total] the steps' gradient; padding zero since creation
  double* part;       // [nparts] sums of squares of the last gradient normed
  const float* last;  // the most recent apply's gradient (dqz_optimizer_outputs without clipping)
  int wide_n;         // 0: dqz_param_layout; N: a wide head's layout (dqz_c51_param_layout, dqz_qr_param_layout)
  int rb;             // 1: the Rainbow network's twenty leaves (dqz_rainbow_param_layout), wide_n its N
  void* block;
};

// The Rainbow network's layout (dqz.h, "the Rainbow agent"): leaves 0-7 are any DQN network's, A1-mu being fc1.
static void rb_param_layout(int A, int N, int64_t off[DQZ_RAINBOW_NUM_LEAVES], int64_t sz[DQZ_RAINBOW_NUM_LEAVES],
                            int64_t* total) {
  const int64_t w1 = (int64_t)FLAT * HID, wa = (int64_t)HID * A * N, wv = (int64_t)HID * N;
  const int64_t sizes[DQZ_RAINBOW_NUM_LEAVES] = {C1KK * C1CO, C1CO, C2KK * C2CO, C2CO, C3KK * C3CO, C3CO,
                                                 w1, HID, w1, HID, wa, wa, (int64_t)A * N,
                                                 w1, HID, w1, HID, wv, wv, N};
  int64_t o = 0;
  for (int i = 0; i < DQZ_RAINBOW_NUM_LEAVES; ++i) {
    off[i] = o;
    sz[i] = sizes[i];
    o += (sizes[i] + 63) / 64 * 64;
  }
  *total = o;
}

// wide_n = 0: the scalar head's layout; N: a wide head's (fc2 leaves A * N wide, no shared bias)
static int optimizer_create(const dqz_optimizer_config* cfg, int wide_n, dqz_optimizer** out, int rb = 0) {
  if (!cfg || !out) return fail(DQZ_ERR_INVALID, "null argument");
  if (cfg->kind != DQZ_OPT_ADAM && cfg->kind != DQZ_OPT_RMSPROP)
    return fail(DQZ_ERR_INVALID, "optimizer kind must be DQZ_OPT_ADAM or DQZ_OPT_RMSPROP");
  if (cfg->num_actions < 1 || cfg->num_actions > MAXA) return fail(DQZ_ERR_INVALID, "num_actions must be in [1, %d]", MAXA);
  if (!(cfg->eps >= 0.f)) return fail(DQZ_ERR_INVALID, "eps must be >= 0");
  if (cfg->kind == DQZ_OPT_ADAM && !(cfg->b1 >= 0.f && cfg->b1 < 1.f && cfg->b2 >= 0.f && cfg->b2 < 1.f))
    return fail(DQZ_ERR_INVALID, "b1 and b2 must be in [0, 1)");
  if (cfg->kind == DQZ_OPT_RMSPROP && !(cfg->decay >= 0.f && cfg->decay <= 1.f))
    return fail(DQZ_ERR_INVALID, "decay must be in [0, 1]");
  dqz_optimizer* o = new dqz_optimizer();
  o->cfg = *cfg;
  o->wide_n = wide_n;
  o->rb = rb;
  int64_t off[DQZ_RAINBOW_NUM_LEAVES], sz[DQZ_RAINBOW_NUM_LEAVES];
  if (rb)
    rb_param_layout(cfg->num_actions, wide_n, off, sz, &o->total);
  else if (wide_n)
    wide_param_layout(cfg->num_actions, wide_n, off, sz, &o->total);
  else
    param_layout(cfg->num_actions, cfg->shared_bias, off, sz, &o->total);
  const int leaves = rb ? DQZ_RAINBOW_NUM_LEAVES : DQZ_NUM_LEAVES;
  for (int i = 0; i < DQZ_RAINBOW_NUM_LEAVES; ++i) {  // leaves the layout does not have: empty, behind the last float4
    o->lv.off4[i] = i < leaves ? off[i] / 4 : o->total / 4;
    o->lv.end[i] = i < leaves ? off[i] + sz[i] : o->total;
  }
  o->lv.n4 = o->total / 4;
  o->nblocks = (int)((o->lv.n4 + OPT_THREADS * OPT_UNROLL - 1) / (OPT_THREADS * OPT_UNROLL));
  o->nparts = (int)((o->lv.n4 + OPT_THREADS * OPT_NORM_UNROLL - 1) / (OPT_THREADS * OPT_NORM_UNROLL));
  const size_t grad_b = (size_t)o->total * sizeof(float);  // a multiple of 256
  const size_t bytes = grad_b + (size_t)o->nparts * sizeof(double);
  if (hipMalloc(&o->block, bytes) != hipSuccess || hipMemset(o->block, 0, bytes) != hipSuccess) {
    if (o->block) (void)hipFree(o->block);
    delete o;
    return fail(DQZ_ERR_HIP, "hipMalloc of %lld bytes of optimizer scratch failed", (long long)bytes);
  }
  o->grad = (float*)o->block;
  o->part = (double*)((char*)o->block + grad_b);
  o->last = nullptr;
  *out = o;
  return DQZ_OK;
}

int dqz_optimizer_create(const dqz_optimizer_config* cfg, dqz_optimizer** out) {
  return optimizer_create(cfg, 0, out);
}

int dqz_optimizer_destroy(dqz_optimizer* o) {
  if (!o) return DQZ_OK;
  if (o->block) (void)hipFree(o->block);
  delete o;
  return DQZ_OK;
}

// The ten-leaf table of the kernels every layout but the Rainbow network's runs on
static OptLeaves opt_leaves10(const dqz_optimizer* o) {
  OptLeaves lv;
  for (int i = 0; i < DQZ_NUM_LEAVES; ++i) {
    lv.off4[i] = o->lv.off4[i];
    lv.end[i] = o->lv.end[i];
  }
  lv.n4 = o->lv.n4;
  return lv;
}

}  // extern "C"

// An apply kernel's argument on either table
template <class Args, class Leaves>
static Args opt_args(const dqz_optimizer* o, const Leaves& lv, float* th, const float* grad, float* mu, float* nu,
                     int32_t* count, bool clip) {
  Args a{};
  a.lv = lv;
  a.th = (float4*)th;
  a.m = (float4*)mu;
  a.v = (float4*)nu;
  a.g = (const float4*)grad;
  a.kind = o->cfg.kind;
  a.lr = o->cfg.learning_rate;
  a.b1 = o->cfg.b1;
  a.b2 = o->cfg.b2;
  a.decay = o->cfg.decay;
  a.eps = o->cfg.eps;
  a.clip = o->cfg.max_global_grad_norm;
  a.part = clip ? o->part : nullptr;
  a.nparts = o->nparts;
  a.count = count;
  return a;
}

extern "C" {

static int opt_norm(dqz_optimizer* o, const float* grad, hipStream_t st) {
  if (o->rb)
    hipLaunchKernelGGL(opt_norm_rb_kernel, dim3(o->nparts), dim3(OPT_THREADS), 0, st, (const float4*)grad, o->lv,
                       o->part);
  else
    hipLaunchKernelGGL(opt_norm_kernel, dim3(o->nparts), dim3(OPT_THREADS), 0, st, (const float4*)grad,
                       opt_leaves10(o), o->part);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

int dqz_optimizer_apply(dqz_optimizer* o, float* th, const float* grad, float* mu, float* nu, int32_t* count,
                        void* stream) {
  if (!o || !th || !grad || !nu) return fail(DQZ_ERR_INVALID, "null argument");
  const bool is_adam = o->cfg.kind == DQZ_OPT_ADAM;
  if (is_adam && (!mu || !count)) return fail(DQZ_ERR_INVALID, "Adam needs mu and count");
  if ((reinterpret_cast<uintptr_t>(th) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(nu) |
       reinterpret_cast<uintptr_t>(mu)) % 16)
    return fail(DQZ_ERR_INVALID, "parameters, gradient and moments must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const bool clip = o->cfg.max_global_grad_norm > 0.f;
  if (clip)
    if (int rc = opt_norm(o, grad, st)) return rc;
  const dim3 grid(o->nblocks), block(OPT_THREADS);
  if (o->rb) {
    const OptArgsRb a = opt_args<OptArgsRb>(o, o->lv, th, grad, mu, nu, count, clip);
    if (is_adam)
      hipLaunchKernelGGL(opt_adam_rb_kernel, grid, block, 0, st, a);
    else
      hipLaunchKernelGGL(opt_rms_rb_kernel, grid, block, 0, st, a);
  } else {
    const OptArgs a = opt_args<OptArgs>(o, opt_leaves10(o), th, grad, mu, nu, count, clip);
    if (is_adam)
      hipLaunchKernelGGL(opt_adam_kernel, grid, block, 0, st, a);
    else
      hipLaunchKernelGGL(opt_rms_kernel, grid, block, 0, st, a);
  }
  if (is_adam) {
    DQZ_HIP(hipGetLastError());
    hipLaunchKernelGGL(opt_count_kernel, dim3(1), dim3(64), 0, st, count);
  }
  DQZ_HIP(hipGetLastError());
  o->last = grad;
  return DQZ_OK;
}

int dqz_optimizer_outputs(dqz_optimizer* o, float* gnorm, void* stream) {
  if (!o || !gnorm) return fail(DQZ_ERR_INVALID, "null argument");
  if (!o->last) return fail(DQZ_ERR_INVALID, "no step or apply has run on this optimizer");
  hipStream_t st = (hipStream_t)stream;
  if (!(o->cfg.max_global_grad_norm > 0.f))
    if (int rc = opt_norm(o, o->last, st)) return rc;
  hipLaunchKernelGGL(opt_norm_out_kernel, dim3(1), dim3(OPT_THREADS), 0, st, o->part, o->nparts, gnorm);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

// What a step in gradient mode followed by dqz_optimizer_apply needs checked before anything is enqueued; the
// entry has refused a null handle of its own, and L is not read before the layout is compared.
// wide: null for the scalar head, else the request's wide head (its N is read behind a live L only), whose
// optimizers have no shared bias (dqz_c51_optimizer_create, dqz_qr_optimizer_create), as its learner has none.
static int check_step_apply(const dqz_learner* L, const dqz_params* P, const dqz_optimizer* o, const int32_t* count,
                            const WideHead* wide) {
  if (!P || !o) return fail(DQZ_ERR_INVALID, "null argument");
  if (!P->online || !P->nu) return fail(DQZ_ERR_INVALID, "null optimizer state");
  if (o->cfg.kind == DQZ_OPT_ADAM && (!P->mu || !count)) return fail(DQZ_ERR_INVALID, "Adam needs mu and count");
  if ((reinterpret_cast<uintptr_t>(P->online) | reinterpret_cast<uintptr_t>(P->nu) |
       reinterpret_cast<uintptr_t>(P->mu)) % 16)
    return fail(DQZ_ERR_INVALID, "parameters and moments must be 16-byte aligned");
  if (!L || o->cfg.num_actions != L->cfg.num_actions || (o->cfg.shared_bias != 0) != (L->shared_bias != 0) ||
      o->wide_n != (wide ? wide->N : 0) || o->rb != (wide && wide->kind == WIDE_RB ? 1 : 0))
    return fail(DQZ_ERR_INVALID, "the optimizer was created for another parameter layout");
  return DQZ_OK;
}

// The request's step in gradient mode into the optimizer's own buffer, then the optimizer on it.  An entry whose
// request has a draw to build calls check_step_apply ahead of that, so a call is refused for its optimizer first.
static int step_then_apply(dqz_learner* L, const dqz_params* P, const dqz_store* S, StepRequest r, dqz_optimizer* o,
                           int32_t* count, void* stream) {
  if (int rc = check_step_apply(L, P, o, count, r.wide)) return rc;
  r.gout = o->grad;
  if (int rc = step_impl(L, P, S, r, stream)) return rc;
  return dqz_optimizer_apply(o, P->online, o->grad, P->mu, P->nu, count, stream);
}

int dqz_learner_step_opt(dqz_learner* L, const dqz_params* P, const dqz_store* S, const int32_t* slots,
                         const float* is_weights, dqz_optimizer* o, int32_t* count, void* stream) {
  if (!L) return fail(DQZ_ERR_INVALID, "null argument");
  return step_then_apply(L, P, S, {.slots = slots, .is_weights = is_weights}, o, count, stream);
}

int dqz_learner_step_opt_uniform(dqz_learner* L, const dqz_params* P, const dqz_store* S, int64_t base, int64_t size,
                                 int64_t capacity, uint64_t seed, uint64_t* counter_dev, int32_t* slots_out,
                                 dqz_optimizer* o, int32_t* count, void* stream) {
  if (!L) return fail(DQZ_ERR_INVALID, "null argument");
  if (int rc = check_step_apply(L, P, o, count, nullptr)) return rc;
  UniformDraw d;
  if (int rc = uniform_draw_args(L, base, size, capacity, seed, counter_dev, slots_out, &d)) return rc;
  return step_then_apply(L, P, S, {.draw = &d}, o, count, stream);
}

int dqz_learner_step_opt_per_draw(dqz_learner* L, const dqz_params* P, const dqz_store* S, const dqz_per_draw* d,
                                  dqz_optimizer* o, int32_t* count, void* stream) {
  if (!L) return fail(DQZ_ERR_INVALID, "null argument");
  if (int rc = check_step_apply(L, P, o, count, nullptr)) return rc;
  PerSampleArgs a;
  PerWbArgs wb;
  if (int rc = per_draw_request(L, d, &a, &wb)) return rc;
  return step_then_apply(L, P, S, {.pd = &a, .wb = &wb}, o, count, stream);
}

int dqz_per_add(double* tree, int64_t cap, int32_t remove_index, int32_t add_index, double priority,
                const double* max_seen_dev, double alpha, int32_t* index_to_slot, int32_t slot, void* stream) {
  if (!tree) return fail(DQZ_ERR_INVALID, "null tree");
  if (cap < 1 || (cap & (cap - 1))) return fail(DQZ_ERR_INVALID, "cap must be a power of two");
  const int levels = tree_levels(cap);
  if (levels > 32) return fail(DQZ_ERR_INVALID, "cap must be <= 2^32");
  if (add_index < 0 || add_index >= cap || remove_index >= cap) return fail(DQZ_ERR_INVALID, "index out of range");
  if (priority < 0.0 && !max_seen_dev) return fail(DQZ_ERR_INVALID, "priority < 0 needs max_seen_dev");
  if (priority >= 0.0 && !std::isfinite(priority)) return fail(DQZ_ERR_INVALID, "value must be finite and positive.");
  if (alpha < 0.0) return fail(DQZ_ERR_INVALID, "Require priority_exponent >= 0.");
  hipLaunchKernelGGL(per_add_kernel, dim3(1), dim3(ST_FAST), 0, (hipStream_t)stream, tree, cap, levels, remove_index,
                     add_index, priority, max_seen_dev, alpha, index_to_slot, slot);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

int dqz_target_copy(float* target, const float* online, int64_t total, void* stream) {
  if (!target || !online || total < 0) return fail(DQZ_ERR_INVALID, "bad argument");
  DQZ_HIP(hipMemcpyAsync(target, online, total * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return DQZ_OK;
}

int dqz_learner_debug_activations(dqz_learner* L, int z, float* y1, float* y2, float* y3, float* h1, float* q,
                                  float* dz1, float* dy3, float* dy2, float* dy1, void* stream) {
  if (!L) return fail(DQZ_ERR_INVALID, "null learner");
  if (z < 0 || z >= L->Z) return fail(DQZ_ERR_INVALID, "z must be in [0, %d)", L->Z);
  hipStream_t st = (hipStream_t)stream;
  const int64_t B = L->cfg.batch, A = L->cfg.num_actions;
  // slab zc of a [Z][B][n] forward array, or the one [B][n] backward array
  const struct {
    float* dst;
    const float* src;
    int64_t n, zc;
  } rows[] = {{y1, L->y1, (int64_t)C1M * C1CO, z}, {y2, L->y2, (int64_t)C2M * C2CO, z}, {y3, L->y3, FLAT, z},
              {h1, L->h1, HID, z},                 {q, L->q, A, z},                     {dz1, L->dz1, HID, 0},
              {dy3, L->dy3, FLAT, 0},              {dy2, L->dy2, (int64_t)C2M * C2CO, 0},
              {dy1, L->dy1, (int64_t)C1M * C1CO, 0}};
  for (const auto& r : rows)
    if (r.dst)
      DQZ_HIP(hipMemcpyAsync(r.dst, r.src + r.zc * B * r.n, sizeof(float) * B * r.n, hipMemcpyDeviceToDevice, st));
  return DQZ_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// the categorical (C51), quantile (QR-DQN) and Rainbow agents (c51.hpp, qr.hpp, rainbow.hpp): one host path, three
// sets of entries (Rainbow's own launches and entries: the next section)

static_assert(C51_MAX_ATOMS == C51_MAXN && C51_MAX_OUT == C51_MAXOUT, "learner_impl.hpp restates c51.hpp's limits");
static_assert(QR_MAX_QUANTILES == QR_MAXN && QR_MAX_OUT == QR_MAXOUT, "learner_impl.hpp restates qr.hpp's limits");

// The Rainbow agent's noisy dueling network in front of the categorical head (rainbow.hpp): its leaves, noise
// layout, twenty-leaf parameter layout and scratch.  Of the inner learner's buffers fc1p holds A1-mu's partials,
// h1 is h_adv, dz1 is dz_adv and dy3 the combined dX, so the step's own fc1 dW and update find A1-mu as fc1.
struct dqz::RbNet {
  RbLeaves lf;
  RbNoise nl;
  int64_t off[DQZ_RAINBOW_NUM_LEAVES], sz[DQZ_RAINBOW_NUM_LEAVES], total;
  float* ys;                            // [2][Z][B][3136] e_in * y3 of A1 and of V1
  float* part[3];                       // [Z][S][B][512] split-K partials of V1-mu, A1-sigma, V1-sigma
  float *h_val, *adv, *val;             // [Z][B][512], [Z][B][A N], [Z][B][N]
  float *dz_val, *dz_adv_e, *dz_val_e;  // [B][512]
  float* dx;                            // [4][B][3136]
  void* block;
};

// A dqz_learner on the wide layout plus the head's own buffers: what a dqz_c51, a dqz_qr and a dqz_rainbow handle
// point to.
struct dqz_wide {
  dqz_learner* L;
  int A, N;
  WideHead head;  // grid and outputs, carved from block
  RbNet* rb;      // WIDE_RB alone (head.rb is its view of it); null otherwise
  void* block;
};
static dqz_wide* wide_of(dqz_c51* C) { return reinterpret_cast<dqz_wide*>(C); }
static dqz_wide* wide_of(dqz_qr* Q) { return reinterpret_cast<dqz_wide*>(Q); }
static dqz_wide* wide_of(dqz_rainbow* R) { return reinterpret_cast<dqz_wide*>(R); }
static dqz_learner* learner_of(dqz_wide* W) { return W ? W->L : nullptr; }  // null: the shared checks refuse it

static int wide_check_shape(WideKind kind, int A, int N) {
  const WideDesc& d = kWide[kind];
  if (A < 1 || A > MAXA) return fail(DQZ_ERR_INVALID, "num_actions must be in [1, %d]", MAXA);
  if (N < d.min_n || N > d.max_n) return fail(DQZ_ERR_INVALID, "%s must be in [%d, %d]", d.count, d.min_n, d.max_n);
  if (A * N > d.max_out) return fail(DQZ_ERR_INVALID, "num_actions * %s must be <= %d", d.count, d.max_out);
  return DQZ_OK;
}

static int c51_logits(dqz_learner* L, const NetZ& nz, int Z, int B, int AN, float* logits, hipStream_t st) {
  if (L->S_fc1 > FC1_S) return fail(DQZ_ERR_INVALID, "the categorical head takes at most %d fc1 partials", FC1_S);
  for (int z = 0; z < Z; ++z)  // the kernel reads fc1/b as float4
    if (reinterpret_cast<uintptr_t>(nz.p[z]) % 16) return fail(DQZ_ERR_INVALID, "parameters must be 16-byte aligned");
  C51LogitsArgs a{};
  a.fc1p = L->fc1p;
  a.S = L->S_fc1;
  a.h1 = L->h1;
  a.nz = nz;
  a.b1_off = L->off[7];
  a.w2_off = L->off[8];
  a.b2_off = L->off[9];
  a.Z = Z;
  a.B = B;
  a.AN = AN;
  a.logits = logits;
  const dim3 grid((AN + C51_COLS - 1) / C51_COLS, Z * ((B + C51_ROWS - 1) / C51_ROWS));
  hipLaunchKernelGGL(c51_logits_kernel, grid, dim3(256), 0, st, a);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

// The head kernels' arguments that learn and forward mode share
static C51HeadArgs c51_head_args(const WideHead& c, int Z, int B, int A) {
  C51HeadArgs h{};
  h.logits = c.out;
  h.support = c.grid;
  h.Z = Z;
  h.B = B;
  h.A = A;
  h.N = c.N;
  return h;
}
static QrHeadArgs qr_head_args(const WideHead& c, int Z, int B, int A) {
  QrHeadArgs h{};
  h.out = c.out;
  h.tau = c.grid;
  h.kappa = c.kappa;
  h.Z = Z;
  h.B = B;
  h.A = A;
  h.N = c.N;
  return h;
}

// The noisy network's launches (below, behind the entries' shared bodies)
static int rb_outputs(dqz_learner* L, const WideHead& c, const NetZ& nz, int Z, int B, const float* noise,
                      hipStream_t st);
static int rb_launch(WideLaunch which, dqz_learner* L, const dqz_params* P, const StepRequest& r, hipStream_t st);

int dqz::wide_launch(WideLaunch which, dqz_learner* L, const dqz_params* P, const StepRequest& r, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const WideHead& c = *r.wide;
  const bool qr = c.kind == WIDE_QR, rb = c.kind == WIDE_RB;
  const int B = L->cfg.batch, A = L->cfg.num_actions, N = c.N;
  const int Z = L->Z;  // 3 with double_q: the selector, online(s_t), is copy 2
  const int mode = (c.double_q ? WIDE_DOUBLE : 0) | (c.weighted ? WIDE_WEIGHTED : 0) | (rb ? WIDE_NO_DZ1 : 0);
  if (rb && which != WIDE_HEAD) return rb_launch(which, L, P, r, st);  // its head is the categorical one, below
  if (which == WIDE_OUTPUTS) {
    const NetZ nz{{P->online, P->target, P->online}, {0, 1, 1}};
    return c51_logits(L, nz, Z, B, A * N, c.out, st);
  }
  if (which == WIDE_HEAD && qr) {
    QrHeadArgs h = qr_head_args(c, Z, B, A);
    h.rec = reinterpret_cast<const float4*>(L->rec);
    h.qv = c.qv;
    h.theta = c.taken;
    h.dtheta = c.dtaken;
    h.dout = c.dout;
    h.astar = c.astar;
    h.loss_part = L->loss_part;
    h.gq = L->gq;
    h.ga = L->ga;
    h.weights = r.is_weights;
    h.loss_b = c.loss_b;
    h.prio = L->td;
    auto* const k = mode == 3 ? qr_head_kernel<3> : mode == 2 ? qr_head_kernel<2>
                  : mode == 1 ? qr_head_kernel<1> : qr_head_kernel<0>;
    hipLaunchKernelGGL(k, dim3(B), dim3(QR_THREADS), 0, st, h);
  } else if (which == WIDE_HEAD) {  // plain, or behind the noisy network
    C51HeadArgs h = c51_head_args(c, Z, B, A);
    if (!rb) {  // WIDE_NO_DZ1: dz is rb_dhidden_kernel's (WIDE_DZ1), and h1, w2 and dz1 stay unset
      h.h1 = L->h1;
      h.w2 = P->online + L->off[8];
      h.dz1 = L->dz1;
    }
    h.rec = reinterpret_cast<const float4*>(L->rec);
    h.qv = c.qv;
    h.la = c.taken;
    h.dl = c.dtaken;
    h.astar = c.astar;
    h.loss_part = L->loss_part;
    h.gq = L->gq;
    h.ga = L->ga;
    h.weights = r.is_weights;
    h.loss_b = c.loss_b;
    h.prio = L->td;
    // a Rainbow head is double_q and weighted (dqz_rainbow_create): 7 is its one mode, the only one built with
    // WIDE_NO_DZ1; no other may fall through to a kernel that reads the h1, w2 and dz1 left unset above
    if (rb && mode != 7) return fail(DQZ_ERR_INVALID, "the rainbow head is built double-Q and weighted only");
    auto* const k = mode == 7 ? c51_head_kernel<7> : mode == 3 ? c51_head_kernel<3> : mode == 2 ? c51_head_kernel<2>
                  : mode == 1 ? c51_head_kernel<1> : c51_head_kernel<0>;
    hipLaunchKernelGGL(k, dim3(B), dim3(HID), 0, st, h);
  } else if (which == WIDE_DZ1) {  // the quantile head alone (WideHead::dout)
    QrDz1Args d{};
    d.dout = c.dout;
    d.w2 = P->online + L->off[8];
    d.h1 = L->h1;
    d.B = B;
    d.AN = A * N;
    d.dz1 = L->dz1;
    hipLaunchKernelGGL(qr_dz1_kernel, dim3(HID / QR_DZ_ROWS, (B + 15) / 16), dim3(64 * QR_DZ_WAVES), 0, st, d);
  } else if (qr) {  // WIDE_FC2_GRAD
    QrGradArgs g{};
    g.h1 = L->h1;
    g.dout = c.dout;
    g.B = B;
    g.AN = A * N;
    g.gw = r.gout + L->off[8];
    g.gb = r.gout + L->off[9];
    g.acc = r.gacc;
    const dim3 grid(HID / 16 + 1, (A * N + 64 * QR_FG_TILES - 1) / (64 * QR_FG_TILES));
    hipLaunchKernelGGL(qr_fc2_grad_kernel, grid, dim3(256), 0, st, g);
  } else {
    C51GradArgs g{};
    g.h1 = L->h1;
    g.dl = c.dtaken;
    g.ga = L->ga;
    g.B = B;
    g.A = A;
    g.N = N;
    g.gw = r.gout + L->off[8];
    g.gb = r.gout + L->off[9];
    g.acc = r.gacc;
    const int64_t elems = (int64_t)(HID + 1) * A * N;
    hipLaunchKernelGGL(c51_fc2_grad_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, g);
  }
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

// The head in forward mode: q_values to q_out and, for the actor, its draw
template <class Args>
static void set_forward(Args* h, float* q_out, const ActorDraw* act) {
  h->fwd_only = 1;
  h->qv = q_out;
  if (act) {
    h->act_out = act->out;
    h->eps = act->eps;
    h->act_seed = act->seed;
    h->act_ctr = act->counter;
  }
}

// q_values of n states through one copy: the torso, the outputs (a WIDE_RB head's: one application of the noisy
// network under `noise` [len], null from the others), the head in forward mode (actor: with a draw)
static int wide_forward_q(dqz_wide* W, const float* params, const Conv1Src& src, int which, int n, const float* noise,
                          float* q_out, const ActorDraw* act, hipStream_t st) {
  dqz_learner* L = W->L;
  const bool rb = W->head.kind == WIDE_RB;
  // the noisy network's launches read the parameters as float4: refused before the torso; the others' outputs
  // launch alone does, and c51_logits refuses there
  if (rb && reinterpret_cast<uintptr_t>(params) % 16)
    return fail(DQZ_ERR_INVALID, "parameters must be 16-byte aligned");
  if (int rc = forward_torso(L, params, src, which, n, st)) return rc;
  const NetZ nz{{params, params, params}, {which, which, which}};
  if (int rc = rb ? rb_outputs(L, W->head, nz, 1, n, noise, st)
                  : c51_logits(L, nz, 1, n, W->A * W->N, W->head.out, st))
    return rc;
  if (W->head.kind == WIDE_QR) {
    QrHeadArgs h = qr_head_args(W->head, 1, n, W->A);
    set_forward(&h, q_out, act);
    hipLaunchKernelGGL(qr_head_kernel<0>, dim3(n), dim3(QR_THREADS), 0, st, h);
  } else {
    C51HeadArgs h = c51_head_args(W->head, 1, n, W->A);
    set_forward(&h, q_out, act);
    hipLaunchKernelGGL(c51_head_kernel<0>, dim3(n), dim3(HID), 0, st, h);
  }
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

// The entries' bodies.  A null handle is refused first; of a live one nothing but L is read before the shared
// checks (forward_src, check_step_apply, check_step) have met a null L.

static int wide_layout(WideKind kind, int A, int N, int64_t offsets[10], int64_t sizes[10], int64_t* total) {
  if (int rc = wide_check_shape(kind, A, N)) return rc;
  if (!offsets || !sizes || !total) return fail(DQZ_ERR_INVALID, "null output pointer");
  wide_param_layout(A, N, offsets, sizes, total);
  return DQZ_OK;
}

static int wide_optimizer_create(WideKind kind, const dqz_optimizer_config* cfg, int N, dqz_optimizer** out) {
  if (!cfg || !out) return fail(DQZ_ERR_INVALID, "null argument");
  if (int rc = wide_check_shape(kind, cfg->num_actions, N)) return rc;
  if (cfg->shared_bias) return fail(DQZ_ERR_INVALID, "the %s head has no shared bias", kWide[kind].noun);
  // the wide layout depends on A * N alone; the Rainbow network's is the twenty-leaf one
  return optimizer_create(cfg, N, out, kind == WIDE_RB);
}

// What a create refuses of its configuration before it reads the grid: cfg is non-null
static int wide_check_config(WideKind kind, const dqz_learner_config* cfg, int N) {
  if (int rc = wide_check_shape(kind, cfg->num_actions, N)) return rc;
  if (cfg->batch < 2 || cfg->batch > MAXB) return fail(DQZ_ERR_INVALID, "batch must be in [2, %d]", MAXB);
  if (cfg->algo != DQZ_ALGO_DQN) return fail(DQZ_ERR_INVALID, "the %s head runs on a DQN learner", kWide[kind].noun);
  return DQZ_OK;
}

static int wide_destroy(dqz_wide* W) {
  if (!W) return DQZ_OK;
  if (W->rb && W->rb->block) (void)hipFree(W->rb->block);
  delete W->rb;
  if (W->block) (void)hipFree(W->block);
  (void)dqz_learner_destroy(W->L);
  delete W;
  return DQZ_OK;
}

// The back half of both creates, behind wide_check_config and the entry's own checks of its grid (host, [N])
// opt: null for the plain creates.  With double_q the inner learner is the three-copy one (DQZ_ALGO_DOUBLE's Z),
// on the wide layout like the plain one: no shared bias.
static int wide_create(WideKind kind, const dqz_learner_config* cfg, int N, const float* grid_host, float kappa,
                       const dqz_wide_options* opt, dqz_wide** out) {
  const WideDesc& d = kWide[kind];
  const int double_q = opt ? opt->double_q : 0, weighted = opt ? opt->weighted : 0;
  dqz_learner_config inner = *cfg;
  if (double_q) inner.algo = DQZ_ALGO_DOUBLE;
  dqz_learner* L = nullptr;
  if (int rc = dqz_learner_create(&inner, &L)) return rc;
  const int A = cfg->num_actions;
  wide_param_layout(A, N, L->off, L->sz, &L->total);  // leaves 0-7 unchanged; the scalar head's L->q stays unused
  L->shared_bias = 0;
  dqz_wide* W = new dqz_wide();
  W->L = L;
  W->A = A;
  W->N = N;
  // every piece on a 64-float boundary, in WideHead's order; astar [B] last
  const auto pad = [](int64_t n) { return (n + 63) / 64 * 64; };
  const int64_t B = cfg->batch, AN = (int64_t)A * N, Z = L->Z;
  const int64_t n_grid = pad(N), n_out = pad(Z * B * AN), n_tk = pad(B * N);
  const int64_t n_do = kind == WIDE_QR ? pad(B * AN + QR_PAD) : 0, n_qv = pad(Z * B * A);
  const int64_t n_as = pad(B), n_lb = weighted ? pad(B) : 0;  // loss_b behind astar, in a weighted head alone
  const int64_t floats = n_grid + n_out + 2 * n_tk + n_do + n_qv + n_as + n_lb;
  if (hipMalloc(&W->block, floats * sizeof(float)) != hipSuccess ||
      hipMemset(W->block, 0, floats * sizeof(float)) != hipSuccess) {
    (void)wide_destroy(W);
    return fail(DQZ_ERR_HIP, "hipMalloc of %lld bytes of %s-head scratch failed", (long long)(floats * 4), d.noun);
  }
  float* p = (float*)W->block;
  WideHead& h = W->head;
  h.kind = kind;
  h.N = N;
  h.grid = p;
  h.kappa = kappa;
  h.out = p + n_grid;
  h.taken = h.out + n_out;
  h.dtaken = h.taken + n_tk;
  h.dout = n_do ? h.dtaken + n_tk : nullptr;
  h.qv = h.dtaken + n_tk + n_do;
  h.astar = reinterpret_cast<int32_t*>(h.qv + n_qv);
  h.double_q = double_q;
  h.weighted = weighted;
  h.loss_b = n_lb ? h.qv + n_qv + n_as : nullptr;
  if (hipMemcpy(p, grid_host, sizeof(float) * N, hipMemcpyHostToDevice) != hipSuccess) {
    (void)wide_destroy(W);
    return fail(DQZ_ERR_HIP, "copy of the %s failed", d.grid);
  }
  *out = W;
  return DQZ_OK;
}

static int wide_learner(dqz_wide* W, dqz_learner** out) {
  if (!W || !out) return fail(DQZ_ERR_INVALID, "null argument");
  *out = W->L;
  return DQZ_OK;
}

// is_weights: null from the plain entries; the _w entries have refused a null one.  noise: [3][len], null from
// every head but Rainbow's, whose entries have refused a null one.
static int wide_step(dqz_wide* W, const dqz_params* P, const dqz_store* S, const int32_t* slots,
                     const float* is_weights, const float* noise, dqz_optimizer* o, int32_t* count, void* stream) {
  if (!W) return fail(DQZ_ERR_INVALID, "null argument");
  const StepRequest r{.slots = slots, .is_weights = is_weights, .wide = &W->head, .noise = noise};
  return step_then_apply(W->L, P, S, r, o, count, stream);
}

static int wide_grad(dqz_wide* W, const dqz_params* P, const dqz_store* S, const int32_t* slots,
                     const float* is_weights, const float* noise, float* grad_out, void* stream) {
  if (!W) return fail(DQZ_ERR_INVALID, "null argument");
  if (!grad_out) return fail(DQZ_ERR_INVALID, "null grad_out");
  const StepRequest r{.slots = slots, .is_weights = is_weights, .gout = grad_out, .wide = &W->head, .noise = noise};
  return step_impl(W->L, P, S, r, stream);
}

static int wide_profile(dqz_wide* W, const dqz_params* P, const dqz_store* S, const int32_t* slots,
                        const float* is_weights, const float* noise, float* grad_out, int iters, float* phase_ms,
                        void* stream) {
  if (!W) return fail(DQZ_ERR_INVALID, "null argument");
  if (!grad_out) return fail(DQZ_ERR_INVALID, "null grad_out");
  const StepRequest r{.slots = slots, .is_weights = is_weights, .gout = grad_out, .wide = &W->head, .noise = noise};
  return profile_step(W->L, P, S, r, iters, phase_ms, stream);
}

static int wide_check_weights(const void* handle, const float* is_weights) {
  if (!handle || !is_weights) return fail(DQZ_ERR_INVALID, "null argument");
  return DQZ_OK;
}

static int wide_outputs(dqz_wide* W, float* taken, float* q_values, float* loss_b, float* loss, int32_t* a_star,
                        void* stream) {
  if (!W) return fail(DQZ_ERR_INVALID, "null argument");
  hipStream_t st = (hipStream_t)stream;
  const int64_t B = W->L->cfg.batch;
  const struct {
    void* dst;
    const void* src;
    int64_t n;
  } rows[] = {{taken, W->head.taken, B * W->N},
              {q_values, W->head.qv, 2 * B * W->A},
              // a weighted head's loss_part holds w_b loss_b; loss_b is in a buffer of its own
              {loss_b, W->head.loss_b ? W->head.loss_b : W->L->loss_part, B},
              {loss, W->L->loss, 1},
              {a_star, W->head.astar, B}};
  for (const auto& r : rows)
    if (r.dst) DQZ_HIP(hipMemcpyAsync(r.dst, r.src, 4 * r.n, hipMemcpyDeviceToDevice, st));
  return DQZ_OK;
}

// What a head with options adds to wide_outputs: the selector's q_values and the priorities
static int wide_outputs_opt(dqz_wide* W, float* q_selector, float* priorities, void* stream) {
  if (!W) return fail(DQZ_ERR_INVALID, "null argument");
  if (q_selector && !W->head.double_q) return fail(DQZ_ERR_INVALID, "q_selector needs a head created with double_q");
  if (priorities && !W->head.weighted) return fail(DQZ_ERR_INVALID, "priorities need a head created with weighted");
  hipStream_t st = (hipStream_t)stream;
  const int64_t B = W->L->cfg.batch;
  if (q_selector)
    DQZ_HIP(hipMemcpyAsync(q_selector, W->head.qv + 2 * B * W->A, 4 * B * W->A, hipMemcpyDeviceToDevice, st));
  if (priorities) DQZ_HIP(hipMemcpyAsync(priorities, W->L->td, 4 * B, hipMemcpyDeviceToDevice, st));
  return DQZ_OK;
}

static int wide_debug(dqz_wide* W, float* outputs, float* dtaken, void* stream) {
  if (!W) return fail(DQZ_ERR_INVALID, "null argument");
  hipStream_t st = (hipStream_t)stream;
  const int64_t B = W->L->cfg.batch;
  if (outputs) DQZ_HIP(hipMemcpyAsync(outputs, W->head.out, 4 * W->L->Z * B * W->A * W->N, hipMemcpyDeviceToDevice, st));
  if (dtaken) DQZ_HIP(hipMemcpyAsync(dtaken, W->head.dtaken, 4 * B * W->N, hipMemcpyDeviceToDevice, st));
  return DQZ_OK;
}

// noise: [len], null from every head but Rainbow's, whose entries have refused a null one
static int wide_forward(dqz_wide* W, const float* params, const uint8_t* states, int n, const float* noise,
                        float* q_out, void* stream) {
  Conv1Src src;
  if (int rc = forward_src(learner_of(W), params, n, {.states = states, .q_out = q_out}, &src)) return rc;
  return wide_forward_q(W, params, src, 0, n, noise, q_out, nullptr, (hipStream_t)stream);
}

static int wide_forward_slots(dqz_wide* W, const float* params, const dqz_store* S, const int32_t* slots, int n,
                              int which, const float* noise, float* q_out, void* stream) {
  Conv1Src src;
  const ForwardInput in{.from_store = true, .store = S, .slots = slots, .which = which, .q_out = q_out};
  if (int rc = forward_src(learner_of(W), params, n, in, &src)) return rc;
  return wide_forward_q(W, params, src, which, n, noise, q_out, nullptr, (hipStream_t)stream);
}

// The Rainbow actor has no epsilon (its entry passes 0): the noise explores, and behind the head in plain forward
// mode rb_act_kernel takes the first argmax with no draw (eps_greedy at eps = 0 breaks ties by its uniform).
static int wide_act(dqz_wide* W, const float* params, const uint8_t* states, int n, const float* noise,
                    double epsilon, uint64_t seed, uint64_t counter, dqz_action* out, void* stream) {
  ActorDraw act{epsilon, seed, counter, out};
  Conv1Src src;
  if (int rc = forward_src(learner_of(W), params, n, {.states = states, .act = &act}, &src)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (W->head.kind != WIDE_RB) return wide_forward_q(W, params, src, 0, n, nullptr, W->head.qv, &act, st);
  if (int rc = wide_forward_q(W, params, src, 0, n, noise, W->head.qv, nullptr, st)) return rc;
  hipLaunchKernelGGL(rb_act_kernel, dim3((n + 63) / 64), dim3(64), 0, st, W->head.qv, n, W->A, act.out);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

static int wide_check_options(const dqz_wide_options* opt) {
  if (!opt) return fail(DQZ_ERR_INVALID, "null argument");
  if ((opt->double_q != 0 && opt->double_q != 1) || (opt->weighted != 0 && opt->weighted != 1))
    return fail(DQZ_ERR_INVALID, "double_q and weighted must be 0 or 1");
  return DQZ_OK;
}

// opt: null for the plain probes (a default WideHead, which keeps refusing weights)
static int wide_debug_check(WideKind kind, int batch, unsigned request, const dqz_wide_options* opt) {
  // a host-only learner, parameters and store whose pointers are set but never followed: check_step alone runs
  static float word[4];
  dqz_learner L{};
  L.cfg.batch = batch;
  L.cfg.num_actions = 6;
  L.cfg.algo = opt && opt->double_q ? DQZ_ALGO_DOUBLE : DQZ_ALGO_DQN;
  const dqz_params P{word, word, word, word};
  dqz_store S{};
  S.frames = reinterpret_cast<uint8_t*>(word);
  S.fidx = reinterpret_cast<int32_t*>(word);
  S.action = reinterpret_cast<int32_t*>(word);
  S.reward = S.discount = word;
  S.capacity = 1;
  int32_t* iw = reinterpret_cast<int32_t*>(word);
  UniformDraw draw{};
  draw.slots_out = iw;
  SoftmaxDraw sm{};
  sm.slots_out = iw;
  SoftmaxDrawExact smx{};
  smx.slots_out = iw;
  PerSampleArgs pd{};
  pd.out_slots = iw;
  const Rms epi{};
  const MetaSoftmax msm{};
  const PerWbArgs wb{};
  WideHead head{};
  head.kind = kind;
  if (opt) {
    head.double_q = opt->double_q;
    head.weighted = opt->weighted;
  }
  StepRequest r{};
  r.slots = iw;
  r.gout = word;
  r.wide = &head;
  if (request & DQZ_C51_REQ_WEIGHTS) r.is_weights = word;
  if (request & DQZ_C51_REQ_PER_DRAW) r.pd = &pd;
  if (request & DQZ_C51_REQ_UNIFORM_DRAW) r.draw = &draw;
  if (request & DQZ_C51_REQ_LOGIT_DRAW) r.sm = &sm;
  if (request & DQZ_C51_REQ_EXACT_DRAW) r.smx = &smx;
  if (request & DQZ_C51_REQ_META_P) r.meta_p = word;
  if (request & DQZ_C51_REQ_META_EPI) r.meta_epi = &epi;
  if (request & DQZ_C51_REQ_META_SOFTMAX) r.meta_sm = &msm;
  if (request & DQZ_C51_REQ_UNIT) r.unit = 1;
  if (request & DQZ_C51_REQ_WRITE_BACK) r.wb = &wb;
  if (request & DQZ_C51_REQ_FUSED_RMSPROP) r.gout = nullptr;
  return check_step(&L, &P, &S, r);
}

// A categorical head's support (C51's, Rainbow's) copied to z and checked on the host (this call may synchronise;
// the step never does); behind wide_check_config, so num_atoms <= C51_MAXN
static int c51_check_support(const float* support, int num_atoms, float z[C51_MAXN]) {
  DQZ_HIP(hipMemcpy(z, support, sizeof(float) * num_atoms, hipMemcpyDefault));
  for (int i = 0; i < num_atoms; ++i)
    if (!std::isfinite(z[i]) || (i > 0 && !(z[i] > z[i - 1])))
      return fail(DQZ_ERR_INVALID, "support must be finite and strictly increasing (atom %d)", i);
  return DQZ_OK;
}

static int c51_create(const dqz_learner_config* cfg, int num_atoms, const float* support,
                      const dqz_wide_options* opt, dqz_c51** out) {
  if (!cfg || !support || !out) return fail(DQZ_ERR_INVALID, "null argument");
  if (int rc = wide_check_config(WIDE_C51, cfg, num_atoms)) return rc;
  float z[C51_MAXN];
  if (int rc = c51_check_support(support, num_atoms, z)) return rc;
  return wide_create(WIDE_C51, cfg, num_atoms, z, 0.f, opt, reinterpret_cast<dqz_wide**>(out));
}

static int qr_create(const dqz_learner_config* cfg, int num_quantiles, const float* quantiles, float huber_param,
                     const dqz_wide_options* opt, dqz_qr** out) {
  if (!cfg || !quantiles || !out) return fail(DQZ_ERR_INVALID, "null argument");
  if (int rc = wide_check_config(WIDE_QR, cfg, num_quantiles)) return rc;
  if (!std::isfinite(huber_param) || !(huber_param > 0.f))
    return fail(DQZ_ERR_INVALID,
                "huber_param must be finite and > 0 (huber_param = 0, rlax's plain |delta| branch, is not built); "
                "got %g", (double)huber_param);
  // the quantiles, checked on the host (this call may synchronise; the step never does)
  float tau[QR_MAXN];
  DQZ_HIP(hipMemcpy(tau, quantiles, sizeof(float) * num_quantiles, hipMemcpyDefault));
  for (int i = 0; i < num_quantiles; ++i)
    if (!std::isfinite(tau[i]) || !(tau[i] > 0.f && tau[i] < 1.f))
      return fail(DQZ_ERR_INVALID, "quantiles must be finite and strictly inside (0, 1) (quantile %d)", i);
  return wide_create(WIDE_QR, cfg, num_quantiles, tau, huber_param, opt, reinterpret_cast<dqz_wide**>(out));
}

extern "C" {

int dqz_c51_create(const dqz_learner_config* cfg, int num_atoms, const float* support, dqz_c51** out) {
  return c51_create(cfg, num_atoms, support, nullptr, out);
}
int dqz_c51_create_opt(const dqz_learner_config* cfg, int num_atoms, const float* support,
                       const dqz_wide_options* options, dqz_c51** out) {
  if (int rc = wide_check_options(options)) return rc;
  return c51_create(cfg, num_atoms, support, options, out);
}

int dqz_qr_create(const dqz_learner_config* cfg, int num_quantiles, const float* quantiles, float huber_param,
                  dqz_qr** out) {
  return qr_create(cfg, num_quantiles, quantiles, huber_param, nullptr, out);
}
int dqz_qr_create_opt(const dqz_learner_config* cfg, int num_quantiles, const float* quantiles, float huber_param,
                      const dqz_wide_options* options, dqz_qr** out) {
  if (int rc = wide_check_options(options)) return rc;
  return qr_create(cfg, num_quantiles, quantiles, huber_param, options, out);
}

int dqz_c51_param_layout(int num_actions, int num_atoms, int64_t offsets[10], int64_t sizes[10], int64_t* total) {
  return wide_layout(WIDE_C51, num_actions, num_atoms, offsets, sizes, total);
}
int dqz_c51_optimizer_create(const dqz_optimizer_config* cfg, int num_atoms, dqz_optimizer** out) {
  return wide_optimizer_create(WIDE_C51, cfg, num_atoms, out);
}
int dqz_c51_destroy(dqz_c51* C) { return wide_destroy(wide_of(C)); }
int dqz_c51_learner(dqz_c51* C, dqz_learner** out) { return wide_learner(wide_of(C), out); }
int dqz_c51_step(dqz_c51* C, const dqz_params* P, const dqz_store* S, const int32_t* slots, dqz_optimizer* o,
                 int32_t* count, void* stream) {
  return wide_step(wide_of(C), P, S, slots, nullptr, nullptr, o, count, stream);
}
int dqz_c51_step_w(dqz_c51* C, const dqz_params* P, const dqz_store* S, const int32_t* slots, const float* is_weights,
                   dqz_optimizer* o, int32_t* count, void* stream) {
  if (int rc = wide_check_weights(C, is_weights)) return rc;
  return wide_step(wide_of(C), P, S, slots, is_weights, nullptr, o, count, stream);
}
int dqz_c51_grad(dqz_c51* C, const dqz_params* P, const dqz_store* S, const int32_t* slots, float* grad_out,
                 void* stream) {
  return wide_grad(wide_of(C), P, S, slots, nullptr, nullptr, grad_out, stream);
}
int dqz_c51_grad_w(dqz_c51* C, const dqz_params* P, const dqz_store* S, const int32_t* slots, const float* is_weights,
                   float* grad_out, void* stream) {
  if (int rc = wide_check_weights(C, is_weights)) return rc;
  return wide_grad(wide_of(C), P, S, slots, is_weights, nullptr, grad_out, stream);
}
int dqz_c51_profile(dqz_c51* C, const dqz_params* P, const dqz_store* S, const int32_t* slots, float* grad_out,
                    int iters, float* phase_ms, void* stream) {
  return wide_profile(wide_of(C), P, S, slots, nullptr, nullptr, grad_out, iters, phase_ms, stream);
}
int dqz_c51_profile_w(dqz_c51* C, const dqz_params* P, const dqz_store* S, const int32_t* slots,
                      const float* is_weights, float* grad_out, int iters, float* phase_ms, void* stream) {
  if (int rc = wide_check_weights(C, is_weights)) return rc;
  return wide_profile(wide_of(C), P, S, slots, is_weights, nullptr, grad_out, iters, phase_ms, stream);
}
int dqz_c51_outputs(dqz_c51* C, float* logits_a, float* q_values, float* loss_b, float* loss, int32_t* a_star,
                    void* stream) {
  return wide_outputs(wide_of(C), logits_a, q_values, loss_b, loss, a_star, stream);
}
int dqz_c51_outputs_opt(dqz_c51* C, float* q_selector, float* priorities, void* stream) {
  return wide_outputs_opt(wide_of(C), q_selector, priorities, stream);
}
int dqz_c51_debug(dqz_c51* C, float* logits, float* dlogits, void* stream) {
  return wide_debug(wide_of(C), logits, dlogits, stream);
}
int dqz_c51_forward(dqz_c51* C, const float* params, const uint8_t* states, int n, float* q_out, void* stream) {
  return wide_forward(wide_of(C), params, states, n, nullptr, q_out, stream);
}
int dqz_c51_forward_slots(dqz_c51* C, const float* params, const dqz_store* S, const int32_t* slots, int n, int which,
                          float* q_out, void* stream) {
  return wide_forward_slots(wide_of(C), params, S, slots, n, which, nullptr, q_out, stream);
}
int dqz_c51_act(dqz_c51* C, const float* params, const uint8_t* states, int n, double epsilon, uint64_t seed,
                uint64_t counter, dqz_action* out, void* stream) {
  return wide_act(wide_of(C), params, states, n, nullptr, epsilon, seed, counter, out, stream);
}
int dqz_c51_debug_check(int batch, unsigned request) { return wide_debug_check(WIDE_C51, batch, request, nullptr); }
int dqz_c51_debug_check_opt(int batch, unsigned request, const dqz_wide_options* options) {
  if (int rc = wide_check_options(options)) return rc;
  return wide_debug_check(WIDE_C51, batch, request, options);
}

int dqz_qr_param_layout(int num_actions, int num_quantiles, int64_t offsets[10], int64_t sizes[10], int64_t* total) {
  return wide_layout(WIDE_QR, num_actions, num_quantiles, offsets, sizes, total);
}
int dqz_qr_optimizer_create(const dqz_optimizer_config* cfg, int num_quantiles, dqz_optimizer** out) {
  return wide_optimizer_create(WIDE_QR, cfg, num_quantiles, out);
}
int dqz_qr_destroy(dqz_qr* Q) { return wide_destroy(wide_of(Q)); }
int dqz_qr_learner(dqz_qr* Q, dqz_learner** out) { return wide_learner(wide_of(Q), out); }
int dqz_qr_step(dqz_qr* Q, const dqz_params* P, const dqz_store* S, const int32_t* slots, dqz_optimizer* o,
                int32_t* count, void* stream) {
  return wide_step(wide_of(Q), P, S, slots, nullptr, nullptr, o, count, stream);
}
int dqz_qr_step_w(dqz_qr* Q, const dqz_params* P, const dqz_store* S, const int32_t* slots, const float* is_weights,
                   dqz_optimizer* o, int32_t* count, void* stream) {
  if (int rc = wide_check_weights(Q, is_weights)) return rc;
  return wide_step(wide_of(Q), P, S, slots, is_weights, nullptr, o, count, stream);
}
int dqz_qr_grad(dqz_qr* Q, const dqz_params* P, const dqz_store* S, const int32_t* slots, float* grad_out,
                void* stream) {
  return wide_grad(wide_of(Q), P, S, slots, nullptr, nullptr, grad_out, stream);
}
int dqz_qr_grad_w(dqz_qr* Q, const dqz_params* P, const dqz_store* S, const int32_t* slots, const float* is_weights,
                   float* grad_out, void* stream) {
  if (int rc = wide_check_weights(Q, is_weights)) return rc;
  return wide_grad(wide_of(Q), P, S, slots, is_weights, nullptr, grad_out, stream);
}
int dqz_qr_profile(dqz_qr* Q, const dqz_params* P, const dqz_store* S, const int32_t* slots, float* grad_out,
                   int iters, float* phase_ms, void* stream) {
  return wide_profile(wide_of(Q), P, S, slots, nullptr, nullptr, grad_out, iters, phase_ms, stream);
}
int dqz_qr_profile_w(dqz_qr* Q, const dqz_params* P, const dqz_store* S, const int32_t* slots,
                      const float* is_weights, float* grad_out, int iters, float* phase_ms, void* stream) {
  if (int rc = wide_check_weights(Q, is_weights)) return rc;
  return wide_profile(wide_of(Q), P, S, slots, is_weights, nullptr, grad_out, iters, phase_ms, stream);
}
int dqz_qr_outputs(dqz_qr* Q, float* theta, float* q_values, float* loss_b, float* loss, int32_t* a_star,
                   void* stream) {
  return wide_outputs(wide_of(Q), theta, q_values, loss_b, loss, a_star, stream);
}
int dqz_qr_outputs_opt(dqz_qr* Q, float* q_selector, float* priorities, void* stream) {
  return wide_outputs_opt(wide_of(Q), q_selector, priorities, stream);
}
int dqz_qr_debug(dqz_qr* Q, float* outputs, float* dtheta, void* stream) {
  return wide_debug(wide_of(Q), outputs, dtheta, stream);
}
int dqz_qr_forward(dqz_qr* Q, const float* params, const uint8_t* states, int n, float* q_out, void* stream) {
  return wide_forward(wide_of(Q), params, states, n, nullptr, q_out, stream);
}
int dqz_qr_forward_slots(dqz_qr* Q, const float* params, const dqz_store* S, const int32_t* slots, int n, int which,
                         float* q_out, void* stream) {
  return wide_forward_slots(wide_of(Q), params, S, slots, n, which, nullptr, q_out, stream);
}
int dqz_qr_act(dqz_qr* Q, const float* params, const uint8_t* states, int n, double epsilon, uint64_t seed,
               uint64_t counter, dqz_action* out, void* stream) {
  return wide_act(wide_of(Q), params, states, n, nullptr, epsilon, seed, counter, out, stream);
}
int dqz_qr_debug_check(int batch, unsigned request) { return wide_debug_check(WIDE_QR, batch, request, nullptr); }
int dqz_qr_debug_check_opt(int batch, unsigned request, const dqz_wide_options* options) {
  if (int rc = wide_check_options(options)) return rc;
  return wide_debug_check(WIDE_QR, batch, request, options);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// the Rainbow agent (rainbow.hpp): a categorical head (double_q and weighted) behind the noisy dueling network

// A dqz_rainbow handle is a dqz_wide whose head is WIDE_RB and whose rb is the network (RbNet, above).

// Everything between the torso's fc1 launch (A1-mu, in L->fc1p) and the head: q_logits of Z applications on B
// rows under `noise` [Z][len] into the head's `out`.
static int rb_outputs(dqz_learner* L, const WideHead& c, const NetZ& nz, int Z, int B, const float* noise,
                      hipStream_t st) {
  const RbNet* R = c.rb;
  const int A = L->cfg.num_actions, N = c.N, AN = A * N;
  const int64_t rows = (int64_t)Z * B;
  RbScaleArgs sc{L->y3, noise, R->nl, Z, B, R->ys};
  hipLaunchKernelGGL(rb_scale_kernel, dim3((unsigned)((rows * (FLAT / 4) + 255) / 256)), dim3(256), 0, st, sc);
  DQZ_HIP(hipGetLastError());
  Fc1FwdArgs f = make_fwd_args(L, nz, Z, B, Conv1Src{}).f1;
  const struct {
    const float* in;
    int64_t w_off;
  } prod[3] = {{L->y3, R->lf.v1w}, {R->ys, R->lf.a1sw}, {R->ys + rows * FLAT, R->lf.v1sw}};
  for (int i = 0; i < 3; ++i) {
    f.in = prod[i].in;
    f.w_off = prod[i].w_off;
    f.part = R->part[i];
    if (int rc = fc1_forward(f, Z, st)) return rc;
  }
  RbHiddenArgs h{};
  h.part[0] = L->fc1p;
  h.part[1] = R->part[0];
  h.part[2] = R->part[1];
  h.part[3] = R->part[2];
  h.S = L->S_fc1;
  h.nz = nz;
  h.lf = R->lf;
  h.noise = noise;
  h.nl = R->nl;
  h.Z = Z;
  h.B = B;
  h.h_adv = L->h1;
  h.h_val = R->h_val;
  hipLaunchKernelGGL(rb_hidden_kernel, dim3((unsigned)((rows * HID + 255) / 256)), dim3(256), 0, st, h);
  DQZ_HIP(hipGetLastError());
  RbLogitsArgs g{L->h1, R->h_val, nz, R->lf, noise, R->nl, Z, B, AN, N, R->adv, R->val};
  hipLaunchKernelGGL(rb_logits_kernel, dim3((AN + N + 255) / 256, (unsigned)rows), dim3(256), 0, st, g);
  DQZ_HIP(hipGetLastError());
  RbCombineArgs cm{R->adv, R->val, Z, B, A, N, c.out};
  hipLaunchKernelGGL(rb_combine_kernel, dim3((unsigned)((rows * N + 255) / 256)), dim3(256), 0, st, cm);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

static int rb_launch(WideLaunch which, dqz_learner* L, const dqz_params* P, const StepRequest& r, hipStream_t st) {
  const WideHead& c = *r.wide;
  const RbNet* R = c.rb;
  const int B = L->cfg.batch, A = L->cfg.num_actions, N = c.N;
  if (which == WIDE_OUTPUTS) {
    const NetZ nz{{P->online, P->target, P->online}, {0, 1, 1}};
    return rb_outputs(L, c, nz, L->Z, B, r.noise, st);
  }
  if (which == WIDE_DZ1) {
    RbDhiddenArgs d{c.dtaken, L->ga, L->h1, R->h_val, P->online, R->lf, r.noise, R->nl, B, A, N,
                    L->dz1, R->dz_val, R->dz_adv_e, R->dz_val_e};
    hipLaunchKernelGGL(rb_dhidden_kernel, dim3(B, HID / RB_DH_ROWS), dim3(512), 0, st, d);
  } else if (which == WIDE_FC1_DX) {
    const int64_t n = (int64_t)B * FLAT;
    Fc1BwdArgs f{};
    f.y3 = L->y3;
    f.th = P->online;
    f.B = B;
    const struct {
      const float* dz;
      int64_t w_off;
    } prod[4] = {{L->dz1, R->lf.a1w}, {R->dz_val, R->lf.v1w}, {R->dz_adv_e, R->lf.a1sw}, {R->dz_val_e, R->lf.v1sw}};
    for (int i = 0; i < 4; ++i) {
      f.dz1 = prod[i].dz;
      f.w_off = prod[i].w_off;
      f.dy3 = R->dx + i * n;
      // the dX-ordered W3 / W2 copies of this step: written by the first launch alone
      f.w3 = i == 0 ? P->online + L->off[4] : nullptr;
      f.w2 = i == 0 ? P->online + L->off[2] : nullptr;
      f.w3p = i == 0 ? L->w3p : nullptr;
      f.w2p = i == 0 ? L->w2p : nullptr;
      if (int rc = fc1_dx(f, st)) return rc;
    }
    RbDxCombineArgs x{R->dx, r.noise, R->nl, B, L->dy3};
    hipLaunchKernelGGL(rb_dx_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x);
  } else {  // WIDE_FC2_GRAD: every fc leaf but A1-mu
    RbFc2GradArgs g{c.dtaken, L->ga, L->h1, R->h_val, R->dz_val, R->dz_adv_e, R->dz_val_e, r.noise, R->nl, R->lf,
                    B, A, N, r.gout, r.gacc};
    hipLaunchKernelGGL(rb_fc2_grad_kernel, dim3((unsigned)((rb_fc2_grad_elems(A * N, N) + 255) / 256)), dim3(256), 0,
                       st, g);
    DQZ_HIP(hipGetLastError());
    RbFc1DwArgs w{{L->y3, R->ys, R->ys + (int64_t)L->Z * B * FLAT}, {R->dz_val, R->dz_adv_e, R->dz_val_e},
                  {R->lf.v1w, R->lf.a1sw, R->lf.v1sw}, B, r.gout, r.gacc};
    hipLaunchKernelGGL(rb_fc1_dw_kernel, dim3(FLAT * (HID / 4) / 256, 3), dim3(256), 0, st, w);
  }
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

// The noisy network of a WIDE_RB head fresh from wide_create: the twenty-leaf layout (the inner learner's too) and
// the scratch.  On failure W, which owns what was made so far, is the caller's to destroy.
static int rb_attach(dqz_wide* W) {
  RbNet* R = new RbNet();
  W->rb = R;
  W->head.rb = R;
  dqz_learner* L = W->L;
  const int A = W->A, N = W->N;
  rb_param_layout(A, N, R->off, R->sz, &R->total);
  for (int i = 0; i < 10; ++i) {  // the step's view: leaves 0-7 (A1-mu as fc1); 8 and 9 it never touches behind a wide head
    L->off[i] = R->off[i];
    L->sz[i] = R->sz[i];
  }
  L->total = R->total;
  const int64_t* o = R->off;
  R->lf = RbLeaves{o[6], o[7], o[8], o[9], o[10], o[11], o[12], o[13], o[14], o[15], o[16], o[17], o[18], o[19]};
  R->nl = rb_noise_layout(A, N);
  const auto pad = [](int64_t n) { return (n + 63) / 64 * 64; };
  const int64_t B = L->cfg.batch, Z = L->Z, AN = (int64_t)A * N;
  const int64_t n_ys = pad(2 * Z * B * FLAT), n_part = pad(Z * L->S_fc1 * B * HID), n_h = pad(Z * B * HID);
  const int64_t n_adv = pad(Z * B * AN), n_val = pad(Z * B * N), n_dz = pad(B * HID), n_dx = pad(4 * B * FLAT);
  const int64_t floats = n_ys + 3 * n_part + n_h + n_adv + n_val + 3 * n_dz + n_dx;
  if (hipMalloc(&R->block, floats * sizeof(float)) != hipSuccess ||
      hipMemset(R->block, 0, floats * sizeof(float)) != hipSuccess)
    return fail(DQZ_ERR_HIP, "hipMalloc of %lld bytes of rainbow scratch failed", (long long)(floats * 4));
  float* p = (float*)R->block;
  R->ys = p;
  p += n_ys;
  for (int i = 0; i < 3; ++i, p += n_part) R->part[i] = p;
  R->h_val = p;
  p += n_h;
  R->adv = p;
  p += n_adv;
  R->val = p;
  p += n_val;
  R->dz_val = p;
  R->dz_adv_e = p + n_dz;
  R->dz_val_e = p + 2 * n_dz;
  p += 3 * n_dz;
  R->dx = p;
  return DQZ_OK;
}

static int rb_check_step(const dqz_rainbow* R, const float* is_weights, const float* noise) {
  if (!R || !is_weights || !noise) return fail(DQZ_ERR_INVALID, "null argument");
  return DQZ_OK;
}

extern "C" {

int dqz_rainbow_param_layout(int num_actions, int num_atoms, int64_t offsets[DQZ_RAINBOW_NUM_LEAVES],
                             int64_t sizes[DQZ_RAINBOW_NUM_LEAVES], int64_t* total) {
  if (int rc = wide_check_shape(WIDE_RB, num_actions, num_atoms)) return rc;
  if (!offsets || !sizes || !total) return fail(DQZ_ERR_INVALID, "null output pointer");
  rb_param_layout(num_actions, num_atoms, offsets, sizes, total);
  return DQZ_OK;
}

int dqz_rainbow_noise_len(int num_actions, int num_atoms, int* out) {
  if (int rc = wide_check_shape(WIDE_RB, num_actions, num_atoms)) return rc;
  if (!out) return fail(DQZ_ERR_INVALID, "null output pointer");
  *out = rb_noise_layout(num_actions, num_atoms).len;
  return DQZ_OK;
}

int dqz_rainbow_noise(uint64_t seed, uint64_t* counter_dev, int n, float* out, void* stream) {
  if (!counter_dev || !out || n < 1 || n > 65536) return fail(DQZ_ERR_INVALID, "bad argument");
  hipLaunchKernelGGL(rb_noise_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, seed, counter_dev, n,
                     out);
  DQZ_HIP(hipGetLastError());
  hipLaunchKernelGGL(rb_noise_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, counter_dev, n);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

int dqz_rainbow_optimizer_create(const dqz_optimizer_config* cfg, int num_atoms, dqz_optimizer** out) {
  return wide_optimizer_create(WIDE_RB, cfg, num_atoms, out);
}

int dqz_rainbow_create(const dqz_learner_config* cfg, int num_atoms, const float* support,
                       const dqz_wide_options* options, dqz_rainbow** out) {
  if (!cfg || !support || !out) return fail(DQZ_ERR_INVALID, "null argument");
  if (options && (options->double_q != 1 || options->weighted != 1))
    return fail(DQZ_ERR_INVALID, "the rainbow step is always double-Q and weighted: options must be {1, 1} or null");
  if (int rc = wide_check_config(WIDE_RB, cfg, num_atoms)) return rc;
  float z[C51_MAXN];
  if (int rc = c51_check_support(support, num_atoms, z)) return rc;
  const dqz_wide_options both{1, 1};
  dqz_wide* W = nullptr;
  if (int rc = wide_create(WIDE_RB, cfg, num_atoms, z, 0.f, &both, &W)) return rc;
  if (int rc = rb_attach(W)) {
    (void)wide_destroy(W);  // it words no refusal: rb_attach's stands
    return rc;
  }
  *out = reinterpret_cast<dqz_rainbow*>(W);
  return DQZ_OK;
}

int dqz_rainbow_destroy(dqz_rainbow* R) { return wide_destroy(wide_of(R)); }
int dqz_rainbow_learner(dqz_rainbow* R, dqz_learner** out) { return wide_learner(wide_of(R), out); }

int dqz_rainbow_step(dqz_rainbow* R, const dqz_params* P, const dqz_store* S, const int32_t* slots,
                     const float* is_weights, const float* noise, dqz_optimizer* o, int32_t* count, void* stream) {
  if (int rc = rb_check_step(R, is_weights, noise)) return rc;
  return wide_step(wide_of(R), P, S, slots, is_weights, noise, o, count, stream);
}
int dqz_rainbow_grad(dqz_rainbow* R, const dqz_params* P, const dqz_store* S, const int32_t* slots,
                     const float* is_weights, const float* noise, float* grad_out, void* stream) {
  if (int rc = rb_check_step(R, is_weights, noise)) return rc;
  return wide_grad(wide_of(R), P, S, slots, is_weights, noise, grad_out, stream);
}
int dqz_rainbow_profile(dqz_rainbow* R, const dqz_params* P, const dqz_store* S, const int32_t* slots,
                        const float* is_weights, const float* noise, float* grad_out, int iters, float* phase_ms,
                        void* stream) {
  if (int rc = rb_check_step(R, is_weights, noise)) return rc;
  return wide_profile(wide_of(R), P, S, slots, is_weights, noise, grad_out, iters, phase_ms, stream);
}
int dqz_rainbow_outputs(dqz_rainbow* R, float* logits_a, float* q_values, float* loss_b, float* loss,
                        int32_t* a_star, void* stream) {
  return wide_outputs(wide_of(R), logits_a, q_values, loss_b, loss, a_star, stream);
}
int dqz_rainbow_outputs_opt(dqz_rainbow* R, float* q_selector, float* priorities, void* stream) {
  return wide_outputs_opt(wide_of(R), q_selector, priorities, stream);
}
int dqz_rainbow_debug_head(dqz_rainbow* R, float* q_logits, float* dlogits, void* stream) {
  return wide_debug(wide_of(R), q_logits, dlogits, stream);
}

int dqz_rainbow_debug(dqz_rainbow* R, float* h_adv, float* h_val, float* adv, float* val, float* dz_adv,
                      float* dz_val, void* stream) {
  if (!R) return fail(DQZ_ERR_INVALID, "null argument");
  hipStream_t st = (hipStream_t)stream;
  const dqz_wide* W = wide_of(R);
  const dqz_learner* L = W->L;
  const RbNet* net = W->rb;
  const int64_t B = L->cfg.batch, AN = (int64_t)W->A * W->N;
  const struct {
    float* dst;
    const float* src;
    int64_t n;
  } rows[] = {{h_adv, L->h1, B * HID},   {h_val, net->h_val, B * HID}, {adv, net->adv, B * AN},
              {val, net->val, B * W->N}, {dz_adv, L->dz1, B * HID},    {dz_val, net->dz_val, B * HID}};
  for (const auto& r : rows)
    if (r.dst) DQZ_HIP(hipMemcpyAsync(r.dst, r.src, 4 * r.n, hipMemcpyDeviceToDevice, st));
  return DQZ_OK;
}

int dqz_rainbow_forward(dqz_rainbow* R, const float* params, const uint8_t* states, int n, const float* noise,
                        float* q_out, void* stream) {
  if (!R || !noise) return fail(DQZ_ERR_INVALID, "null argument");
  return wide_forward(wide_of(R), params, states, n, noise, q_out, stream);
}
int dqz_rainbow_forward_slots(dqz_rainbow* R, const float* params, const dqz_store* S, const int32_t* slots, int n,
                              int which, const float* noise, float* q_out, void* stream) {
  if (!R || !noise) return fail(DQZ_ERR_INVALID, "null argument");
  return wide_forward_slots(wide_of(R), params, S, slots, n, which, noise, q_out, stream);
}
int dqz_rainbow_act(dqz_rainbow* R, const float* params, const uint8_t* states, int n, const float* noise,
                    dqz_action* out, void* stream) {
  if (!R || !noise) return fail(DQZ_ERR_INVALID, "null argument");
  return wide_act(wide_of(R), params, states, n, noise, 0.0, 0, 0, out, stream);  // no epsilon, no draw
}

int dqz_rainbow_debug_check(int batch, unsigned request) {
  const dqz_wide_options both{1, 1};
  return wide_debug_check(WIDE_RB, batch, request, &both);
}

}  // extern "C"

// ---------------------------------------------------------------------------
// MGSC meta-update (meta.hpp)


struct dqz_meta {
  dqz_meta_config cfg;
  // Meta batches larger than the learner's MAXB run in K chunks of C samples
  // (the last one padded with p = 0 samples): G accumulates over the chunks,
  // and once v is known each chunk's backward signals are recomputed for the
  // tangent pass (K = 1 keeps them from the first pass).
  int C, K;
  dqz_learner* lm;   // meta batch learner (B = C)
  dqz_learner* l1;   // one-transition learner (B = 1)
  int64_t total;
  float *G, *thp, *mu1, *nu1, *J;  // [total] each; first order: G is overwritten with v (the second order's v: HQ)
  float *zv1, *zv2, *zv3, *zvp;    // tangent forward outputs
  float *x, *p, *s, *dl, *loss, *loss_part, *td;  // p, s, td: [K C] (p = 0 past M)
  int32_t* slots_pad;                                // [K C]
  float* Gs;                                         // [total] scratch gradient of the recompute pass (K > 1)
  int nparts;
  // second-order (reservoir) meta-gradient
  float *GQ, *HQ, *s1_part, *hpart;
  float *ty1, *ty2, *ty3, *td4, *td3, *td2, *td1, *s1;
  uint8_t* x1;  // [4][84][84] the online transition's s_tm1 bytes (written by the theta' forward)
  float* dotp;  // [C][META_DOT_SLOTS] the tangent launch's dot-product partials (one chunk)
  int* arrive;  // kMetaWords hand-off words (layout.hpp MetaWord), read through word()
  int* word(MetaWord w) const { return arrive + w * Handoff::kStride; }
  unsigned spin_max = 1u << 24;  // polls before the Adam leader's entry wait gives up
  int nparts2;
  void* block;
};

extern "C" {

int dqz_meta_create(const dqz_meta_config* cfg, dqz_meta** out) {
  if (!cfg || !out) return fail(DQZ_ERR_INVALID, "null argument");
  if (cfg->meta_batch < 1 || cfg->meta_batch > (1 << 26))
    return fail(DQZ_ERR_INVALID, "meta_batch must be in [1, 2^26]");
  if (int rc = init_meta_attrs()) return rc;
  const int C = std::min(cfg->meta_batch, MAXB), K = (cfg->meta_batch + C - 1) / C;
  dqz_learner_config lc;
  lc.batch = C;
  lc.num_actions = cfg->num_actions;
  lc.algo = DQZ_ALGO_DQN;
  lc.learning_rate = cfg->learning_rate;
  lc.decay = cfg->decay;
  lc.eps = cfg->eps;
  lc.grad_error_bound = cfg->grad_error_bound;
  dqz_meta* H = new dqz_meta();
  H->cfg = *cfg;
  H->C = C;
  H->K = K;
  if (int rc = dqz_learner_create(&lc, &H->lm)) {
    delete H;
    return rc;
  }
  lc.batch = 1;
  if (int rc = dqz_learner_create(&lc, &H->l1)) {
    dqz_learner_destroy(H->lm);
    delete H;
    return rc;
  }
  const int M = cfg->meta_batch;
  const int64_t KC = (int64_t)K * C, multi = K > 1 ? 1 : 0;
  H->total = H->lm->total;
  H->nparts = (int)((H->total / 4 + 255) / 256);
  H->nparts2 = (int)((H->total + 255) / 256);
  const int64_t so = cfg->second_order ? 1 : 0;
  const int64_t T = H->total, np2 = H->nparts2;
  // the scratch buffers in allocation order, sizes in floats (layout.hpp carve)
  const Carve bufs[] = {
      {&H->G, T}, {&H->thp, T}, {&H->mu1, T}, {&H->nu1, T}, {&H->J, T},
      {&H->zv1, (int64_t)C * C1M * C1CO}, {&H->zv2, (int64_t)C * C2M * C2CO}, {&H->zv3, (int64_t)C * FLAT},
      {&H->zvp, (int64_t)H->lm->S_fc1 * C * HID},
      {&H->x, M}, {&H->p, KC}, {&H->s, KC}, {&H->dl, M}, {&H->loss, 1}, {&H->loss_part, np2}, {&H->td, KC},
      {&H->slots_pad, KC}, {&H->Gs, multi * T},
      {&H->GQ, so * T}, {&H->HQ, so * T}, {&H->s1_part, so * np2},
      {&H->ty1, so * C1M * C1CO}, {&H->ty2, so * C2M * C2CO}, {&H->ty3, so * FLAT}, {&H->td4, so * HID},
      {&H->td3, so * FLAT}, {&H->td2, so * C2M * C2CO}, {&H->td1, so * C1M * C1CO}, {&H->s1, so},
      {&H->hpart, so * HVP_T4_CHUNKS * HID},
      {&H->dotp, (int64_t)C * META_DOT_SLOTS}, {&H->arrive, kMetaWords * Handoff::kStride}, {&H->x1, so * FC * FB / 4}};
  const int64_t tot = carve(bufs, nullptr);
  if (hipMalloc(&H->block, tot * sizeof(float)) != hipSuccess || hipMemset(H->block, 0, tot * sizeof(float)) != hipSuccess) {
    if (H->block) (void)hipFree(H->block);
    dqz_learner_destroy(H->lm);
    dqz_learner_destroy(H->l1);
    delete H;
    return fail(DQZ_ERR_HIP, "hipMalloc of %lld bytes of meta scratch failed", (long long)(tot * 4));
  }
  carve(bufs, (float*)H->block);
  *out = H;
  return DQZ_OK;
}

int dqz_meta_destroy(dqz_meta* H) {
  if (!H) return DQZ_OK;
  dqz_learner_destroy(H->lm);
  dqz_learner_destroy(H->l1);
  if (H->block) (void)hipFree(H->block);
  delete H;
  return DQZ_OK;
}

// One dqz_meta_update call: the entry's arguments, then what the stages (DESIGN §4's, in its order) share.
struct MetaRun {
  dqz_meta* H;
  const dqz_params* P;
  const dqz_store *S, *S1;
  const int32_t *slots, *online_slot, *pos;
  float *logits, *adam_mu, *adam_nu;
  int32_t* adam_count;
  dqz_logit_buffer* logit_buf;
  void* stream;
  hipStream_t st = (hipStream_t)stream;
  const int32_t* mslots = H->K == 1 ? slots : H->slots_pad;  // padded to K C when K > 1
  // the meta stage the gradient epilogues apply (Rms::meta, set by each pass) and its buffers
  Rms epi{.thp = H->thp, .mu1 = H->mu1, .nu1 = H->nu1, .J = H->J, .sq_part = H->loss_part};
  dqz_params P1{H->thp, P->online, nullptr, nullptr};  // the theta' pass: online = theta', target = theta
  const float* v = H->cfg.second_order ? H->HQ : H->G;  // the tangent direction the theta' pass leaves
  // the theta' pass's partial sums of u'^2 (the fc1 dW blocks', then the update's) that the Adam stage folds
  const int A = H->cfg.num_actions;
  int nloss = 4 * (FLAT / 16) + (int)update_blocks(H->l1->sz, A, H->l1->shared_bias ? 1 : A);
};

// G = sum_i p_i g_i, p = softmax(logits[pos]): batched backwards with p-weighted cotangents, one per chunk of C
// samples, accumulated in chunk order (deterministic); K > 1 pads the slots to K C with slots[M - 1] (p = 0 there).
// One chunk: no padding, the head forms p itself (MetaSoftmax), and meta_rms1 runs in the backward's gradient
// epilogues (Rms::meta1); G itself is stored only for the second order (meta_second_kernel reads it).
static int meta_weighted_grad(MetaRun& m) {
  dqz_meta* H = m.H;
  const int M = H->cfg.meta_batch, C = H->C, K = H->K;
  if (K == 1) {
    m.epi.meta = 1;
    const MetaSoftmax msm{m.logits, m.pos, M, H->x, H->p};
    // (the batch learner's td stays current until the next update, dqz_meta_outputs copies it from there)
    return step_impl(H->lm, m.P, m.S, {.slots = m.mslots, .gout = H->cfg.second_order ? H->G : nullptr,
                                       .meta_p = H->p, .meta_epi = &m.epi, .meta_sm = &msm}, m.stream);
  }
  hipLaunchKernelGGL(meta_softmax_kernel, dim3(1 + (unsigned)((K * C + META_THREADS - 1) / META_THREADS)),
                     dim3(META_THREADS), 0, m.st, m.logits, m.pos, M, H->x, H->p, m.slots, K * C, H->slots_pad);
  DQZ_HIP(hipGetLastError());
  for (int64_t k = 0; k < K; ++k) {
    if (int rc = step_impl(H->lm, m.P, m.S, {.slots = H->slots_pad + k * C, .gout = H->G, .gacc = k > 0 ? 1 : 0,
                                             .meta_p = H->p + k * C}, m.stream))
      return rc;
    DQZ_HIP(hipMemcpyAsync(H->td + k * C, H->lm->td, sizeof(float) * C, hipMemcpyDeviceToDevice, m.st));
  }
  return DQZ_OK;
}

// K > 1: theta' = theta + u(G), mu', nu', J in a launch of its own
static int meta_rms1(const MetaRun& m) {
  const dqz_meta* H = m.H;
  const MetaRmsArgs ra{.lr = H->cfg.learning_rate, .decay = H->cfg.decay, .c1 = (float)(1.0 - (double)H->cfg.decay),
                       .eps = H->cfg.eps, .n4 = H->total / 4};
  hipLaunchKernelGGL(meta_rms1_kernel, dim3((unsigned)((ra.n4 + 255) / 256)), dim3(256), 0, m.st, ra,
                     (const float4*)H->G, (const float4*)m.P->online, (const float4*)m.P->mu, (const float4*)m.P->nu,
                     (float4*)H->thp, (float4*)H->mu1, (float4*)H->nu1, (float4*)H->J);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

// theta' pass, first order: g' = grad loss_fn(theta', online transition) is consumed where it is formed by
// meta_rms2 (Rms::meta2): v = -2 u' du/dG -> the G buffer (free in the first order), block sums of u'^2.
static int meta_theta_first(MetaRun& m) {
  m.epi.meta = 2;
  m.epi.vout = m.H->G;
  return step_impl(m.H->l1, &m.P1, m.S1, {.slots = m.online_slot, .meta_epi = &m.epi}, m.stream);
}

// theta' pass, second order: grad q[a] (unit cotangent) -> GQ, consumed where it is formed (Rms::meta3): v_dir ->
// mu1, w -> nu1, block sums of u'^2 and grad q . w.  The one-sample learner keeps the primal activations, the
// backward signals and td' for the HVP, whose epilogue combines v -> HQ.  Not -> thp: hvp_l3_kernel's b1 blocks read
// theta''s conv2 weights from thp while its conv2 row blocks store v's conv2 leaf, with no hand-off between them.
static int meta_theta_second(MetaRun& m) {
  dqz_meta* H = m.H;
  dqz_learner* L1 = H->l1;
  m.epi.meta = 3;
  m.epi.G2 = H->G;
  m.epi.td = L1->td;
  m.epi.bound = H->cfg.grad_error_bound;
  m.epi.s1_part = H->s1_part;
  if (int rc = step_impl(L1, &m.P1, m.S1, {.slots = m.online_slot, .gout = H->GQ, .unit = 1, .meta_epi = &m.epi,
                                           .xout = H->x1}, m.stream))
    return rc;
  // (vdir .. vout: meta_combine in hvp_g's epilogue, v = v_dir + J (alpha s1 grad q - clip(td') H w) -> HQ; hq, the
  // raw H_q w of a null vout, names the same buffer and is not written)
  HvpArgs hv{.x = H->x1, .rec = reinterpret_cast<const float4*>(L1->rec), .th = H->thp, .tw = H->nu1,
             .A = H->cfg.num_actions, .y1 = L1->y1, .y2 = L1->y2, .y3 = L1->y3, .h = L1->h1,
             .d1 = L1->dy1, .d2 = L1->dy2, .d3 = L1->dy3, .d4 = L1->dz1,
             .ty1 = H->ty1, .ty2 = H->ty2, .ty3 = H->ty3, .td4 = H->td4, .td3 = H->td3, .td2 = H->td2, .td1 = H->td1,
             .hq = H->HQ, .part = H->hpart, .s1_part = H->s1_part, .s1_nparts = m.nloss, .s1 = H->s1,
             .vdir = H->mu1, .J = H->J, .gq = H->GQ, .td = L1->td, .bound = H->cfg.grad_error_bound, .vout = H->HQ};
  for (int i = 0; i < 10; ++i) hv.off[i] = L1->off[i];
  // ddot1's in-launch hand-off; a timeout lands in the one-transition learner's error word
  hv.td1_pub = Handoff{H->word(kMetaDdot1Cnt), H->word(kMetaDdot1Ack), L1->sync + sync_of(L1).err(), HVP_B1, HVP_G_C1,
                       L1->spin_max};
  // three launches (hvp.hpp): the tangent forward and backward side by side, then the parameter blocks of H_q w
  hipLaunchKernelGGL(hvp_l1_kernel, dim3(HVP_L1_BLOCKS), dim3(256), 0, m.st, hv);
  hipLaunchKernelGGL(hvp_l2_kernel, dim3(HVP_L2_BLOCKS), dim3(256), 0, m.st, hv);
  hipLaunchKernelGGL(hvp_l3_kernel, dim3(HVP_L3_BLOCKS), dim3(256), 0, m.st, hv);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

// Tangent forward arguments (V * y + vb per layer, no ReLU) over the batch learner's activations, chunk at `ks`
static FwdArgs tangent_args(const MetaRun& m, const int32_t* ks) {
  const dqz_meta* H = m.H;
  const NetZ nv{{m.v, m.v, m.v}, {0, 0, 0}};
  FwdArgs t = make_fwd_args(H->lm, nv, 1, H->C, Conv1Src{m.S->frames, m.S->fidx, ks, nullptr, 0, UniformDraw{}});
  t.c1.linear = t.c2.linear = t.c3.linear = 1;
  t.c1.out = H->zv1;
  t.c2.out = H->zv2;
  t.c3.out = H->zv3;
  t.f1.part = H->zvp;
  return t;
}

// Tangent stage, one chunk (the batch learner still holds the first pass's activations and backward signals): the
// conv layers' dot products from the per-sample gradient slabs beside the fc1 tangent range (meta.hpp SlabDotArgs).
static int meta_tangent_one(const MetaRun& m) {
  const dqz_meta* H = m.H;
  const dqz_learner* L = H->lm;
  FwdArgs t = tangent_args(m, m.mslots);
  t.f1.dot = TangentDot{L->dz1, H->dotp, 12};
  const MetaExtra ex{L->dz1, L->h1, L->gq, L->ga, m.v, L->off[7], L->off[8], L->off[9], H->cfg.num_actions, H->dotp};
  const SlabDotArgs sd{.p1 = L->p1, .p2 = L->p2, .p3 = L->p3, .v = m.v, .off1 = L->off[0], .off2 = L->off[2],
                       .off3 = L->off[4], .part = H->dotp, .M = H->C};
  hipLaunchKernelGGL(tangent_slab_kernel, dim3((unsigned)tangent_slab_blocks(H->C, t.f1.MG)), dim3(256), 0, m.st, sd,
                     t.f1, ex);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

// Tangent stage, K > 1, chunk by chunk: the chunk's forward / backward is recomputed so the batch learner holds its
// activations and backward signals, then the four layers' tangent outputs (one launch) and their dot products -> s.
static int meta_tangent_chunks(const MetaRun& m) {
  const dqz_meta* H = m.H;
  dqz_learner* L = H->lm;
  const int C = H->C;
  for (int64_t k = 0; k < H->K; ++k) {
    const int32_t* ks = m.mslots + k * C;
    if (int rc = step_impl(L, m.P, m.S, {.slots = ks, .gout = H->Gs, .meta_p = H->p + k * C}, m.stream)) return rc;
    const FwdArgs t = tangent_args(m, ks);
    hipLaunchKernelGGL(tangent_fwd_kernel, dim3((unsigned)tangent_fwd_blocks(C, t.f1.MG)), dim3(256), kConv1FwdSmem,
                       m.st, t.c1, t.c2, t.c3, t.f1, MetaExtra{});
    DQZ_HIP(hipGetLastError());
    const MetaDotArgs md{.dy1 = L->dy1, .dy2 = L->dy2, .dy3 = L->dy3, .dz1 = L->dz1, .gq = L->gq, .ga = L->ga,
                         .zv1 = H->zv1, .zv2 = H->zv2, .zv3 = H->zv3, .zvp = H->zvp, .S = FC1_S, .M = C,
                         .A = H->cfg.num_actions, .v = m.v, .b1_off = L->off[7], .w2_off = L->off[8],
                         .b2_off = L->off[9], .h1 = L->h1, .s_out = H->s + k * C};
    hipLaunchKernelGGL(meta_dot_kernel, dim3(C), dim3(256), 0, m.st, md);
    DQZ_HIP(hipGetLastError());
  }
  return DQZ_OK;
}

// Adam on the M logits from s (K > 1) or the tangent launch's partials
static int meta_adam(const MetaRun& m) {
  const dqz_meta* H = m.H;
  dqz_logit_buffer* buf = m.logit_buf;
  // keep the buffer's running log-sum-exp current (the host keeps vouching for it: every write went through here)
  const bool keep = buf && buf->run_known;
  const MetaAdamArgs ad{.x = H->x, .p = H->p, .s = H->s, .dot_part = H->K == 1 ? H->dotp : nullptr, .s_out = H->s,
                        .M = H->cfg.meta_batch, .logits = m.logits, .pos = m.pos, .m = m.adam_mu, .v = m.adam_nu,
                        .count = m.adam_count, .lr = H->cfg.meta_learning_rate, .b1 = H->cfg.b1, .b2 = H->cfg.b2,
                        .eps = H->cfg.meta_eps, .loss_part = H->loss_part, .nparts = m.nloss, .loss = H->loss,
                        .dlogits = H->dl, .run = keep ? buf->run : nullptr, .dirty = keep ? buf->dirty : nullptr,
                        .n_logits = keep ? buf->capacity : 0};
  // (the fused form's re-seed path addresses the buffer with 32-bit byte offsets)
  if (keep && H->K == 1 && ad.M <= META_THREADS && buf->capacity * 4 <= INT32_MAX) {
    // Adam and the re-sums of the chunks it writes in one launch
    MetaAdamChunks ck{buf->csum, buf->nblocks, H->word(kMetaReseed), H->word(kMetaAdamEntry), H->word(kMetaErr),
                      H->spin_max};
    hipLaunchKernelGGL(meta_adam_chunks_kernel, dim3(buf->nblocks), dim3(META_THREADS), 0, m.st, ad, ck);
    DQZ_HIP(hipGetLastError());
    return DQZ_OK;
  }
  hipLaunchKernelGGL(meta_adam_kernel, dim3(1), dim3(META_THREADS), 0, m.st, ad);
  DQZ_HIP(hipGetLastError());
  if (keep) return chunk_sums(buf, m.logits, true, m.st);
  return DQZ_OK;
}

int dqz_meta_update(dqz_meta* H, const dqz_params* P, const dqz_store* S, const int32_t* slots,
                    const dqz_store* S1, const int32_t* online_slot, float* logits, const int32_t* pos,
                    float* adam_mu, float* adam_nu, int32_t* adam_count, dqz_logit_buffer* logit_buf,
                    void* stream) {
  if (!H || !P || !P->online || !P->target || !P->mu || !P->nu || !slots || !online_slot || !logits || !pos ||
      !adam_mu || !adam_nu || !adam_count)
    return fail(DQZ_ERR_INVALID, "null argument");
  if (int rc = check_store(S)) return rc;
  if (int rc = check_store(S1)) return rc;
  MetaRun m{.H = H, .P = P, .S = S, .S1 = S1, .slots = slots, .online_slot = online_slot, .pos = pos,
            .logits = logits, .adam_mu = adam_mu, .adam_nu = adam_nu, .adam_count = adam_count,
            .logit_buf = logit_buf, .stream = stream};
  const bool one = H->K == 1;
  if (int rc = meta_weighted_grad(m)) return rc;
  if (!one)
    if (int rc = meta_rms1(m)) return rc;
  if (int rc = H->cfg.second_order ? meta_theta_second(m) : meta_theta_first(m)) return rc;
  if (int rc = one ? meta_tangent_one(m) : meta_tangent_chunks(m)) return rc;
  return meta_adam(m);
}

int dqz_meta_sync_status(dqz_meta* H, int* status) {
  if (!H || !status) return fail(DQZ_ERR_INVALID, "null argument");
  int s_lm = 0, s_l1 = 0, s_own = 0;
  // (each learner's check clears that learner's words when its word is set)
  if (int rc = dqz_learner_sync_status(H->lm, &s_lm)) return rc;
  if (int rc = dqz_learner_sync_status(H->l1, &s_l1)) return rc;
  DQZ_HIP(hipMemcpy(&s_own, H->word(kMetaErr), sizeof(int), hipMemcpyDeviceToHost));
  *status = s_lm | s_l1 | s_own;
  if (*status != 0) {
    // a wait gave up somewhere in the meta-update: late arrivals may have
    // left counts behind after a reset, so clear every word the meta handle
    // owns (its learners' words are cleared just above only when their own
    // word is set: the HVP's ddot1 timeout lands in l1's word)
    DQZ_HIP(hipMemset(H->arrive, 0, sizeof(int) * kMetaWords * Handoff::kStride));
    for (dqz_learner* L : {H->lm, H->l1})
      DQZ_HIP(hipMemset(L->sync, 0, sizeof(int) * sync_of(L).ints()));
    DQZ_HIP(hipDeviceSynchronize());
  }
  return DQZ_OK;
}

int dqz_meta_debug_stall(dqz_meta* H, int poison, unsigned spin_max) {
  if (!H) return fail(DQZ_ERR_INVALID, "null meta handle");
  const unsigned sm = spin_max ? spin_max : 1u << 24;
  H->spin_max = sm;
  H->lm->spin_max = sm;
  H->l1->spin_max = sm;
  if (poison) {
    const int32_t p = -(1 << 30);
    DQZ_HIP(hipDeviceSynchronize());
    DQZ_HIP(hipMemcpy(H->word(kMetaDdot1Cnt), &p, sizeof(p), hipMemcpyHostToDevice));
    DQZ_HIP(hipMemcpy(H->word(kMetaAdamEntry), &p, sizeof(p), hipMemcpyHostToDevice));
  }
  return DQZ_OK;
}

int dqz_meta_debug_learner(dqz_meta* H, int which, dqz_learner** out) {
  if (!H || !out) return fail(DQZ_ERR_INVALID, "null argument");
  if (which != 0 && which != 1) return fail(DQZ_ERR_INVALID, "which must be 0 (batch) or 1 (one transition)");
  *out = which ? H->l1 : H->lm;
  return DQZ_OK;
}

static_assert(DQZ_META_ZVP_PARTS == FC1_S && DQZ_META_HPART_CHUNKS == HVP_T4_CHUNKS, "dqz.h restates the partial counts");

int dqz_meta_debug_stages(dqz_meta* H, const dqz_meta_stages* o, void* stream) {
  if (!H || !o) return fail(DQZ_ERR_INVALID, "null argument");
  hipStream_t st = (hipStream_t)stream;
  const int64_t T = H->total, C = H->C, KC = (int64_t)H->K * C;
  // kind 1: second-order buffers; kind 2: written by the chunked tangent stage only
  const struct {
    float* dst;
    const float* src;
    int64_t n;
    int kind;
    const char* name;
  } rows[] = {{o->G, H->G, T, 0, "G"},       {o->thp, H->thp, T, 0, "thp"},
              {o->mu1, H->mu1, T, 0, "mu1"}, {o->nu1, H->nu1, T, 0, "nu1"},
              {o->J, H->J, T, 0, "J"},       {o->GQ, H->GQ, T, 1, "GQ"},
              {o->HQ, H->HQ, T, 1, "HQ"},    {o->ty1, H->ty1, (int64_t)C1M * C1CO, 1, "ty1"},
              {o->ty2, H->ty2, (int64_t)C2M * C2CO, 1, "ty2"},
              {o->ty3, H->ty3, FLAT, 1, "ty3"},
              {o->hpart, H->hpart, (int64_t)HVP_T4_CHUNKS * HID, 1, "hpart"},
              {o->td4, H->td4, HID, 1, "td4"},
              {o->td3, H->td3, FLAT, 1, "td3"},
              {o->td2, H->td2, (int64_t)C2M * C2CO, 1, "td2"},
              {o->td1, H->td1, (int64_t)C1M * C1CO, 1, "td1"},
              {o->s1, H->s1, 1, 1, "s1"},    {o->p, H->p, KC, 0, "p"},
              {o->s, H->s, KC, 0, "s"},      {o->zv1, H->zv1, C * C1M * C1CO, 2, "zv1"},
              {o->zv2, H->zv2, C * C2M * C2CO, 2, "zv2"},
              {o->zv3, H->zv3, C * FLAT, 2, "zv3"},
              {o->zvp, H->zvp, (int64_t)FC1_S * C * HID, 2, "zvp"}};
  for (const auto& r : rows) {
    if (!r.dst) continue;
    if (r.kind == 1 && !H->cfg.second_order)
      return fail(DQZ_ERR_INVALID, "%s exists only in a second-order meta handle", r.name);
    if (r.kind == 2 && H->K == 1)
      return fail(DQZ_ERR_INVALID, "%s is written only by a meta batch of more than one chunk", r.name);
  }
  for (const auto& r : rows)
    if (r.dst) DQZ_HIP(hipMemcpyAsync(r.dst, r.src, sizeof(float) * r.n, hipMemcpyDeviceToDevice, st));
  return DQZ_OK;
}

int dqz_meta_outputs(dqz_meta* H, float* probs, float* dlogits, float* td, float* loss, void* stream) {
  if (!H) return fail(DQZ_ERR_INVALID, "null meta handle");
  hipStream_t st = (hipStream_t)stream;
  const int M = H->cfg.meta_batch;
  if (probs) DQZ_HIP(hipMemcpyAsync(probs, H->p, sizeof(float) * M, hipMemcpyDeviceToDevice, st));
  if (dlogits) DQZ_HIP(hipMemcpyAsync(dlogits, H->dl, sizeof(float) * M, hipMemcpyDeviceToDevice, st));
  if (td)
    DQZ_HIP(hipMemcpyAsync(td, H->K > 1 ? H->td : H->lm->td, sizeof(float) * M, hipMemcpyDeviceToDevice, st));
  if (loss) DQZ_HIP(hipMemcpyAsync(loss, H->loss, sizeof(float), hipMemcpyDeviceToDevice, st));
  return DQZ_OK;
}

}  // extern "C"

#ifdef DQZ_TRACE
// Diagnostic builds only (not part of include/dqz.h): copy / clear this
// code object's in-kernel timeline stamps (the HVP's; common.hpp DQZ_STAMP).
extern "C" int dqz_debug_trace_other(unsigned long long* host_out, int clear) {
  const size_t bytes = sizeof(unsigned long long) * TRACE_KERNELS * TRACE_BLOCKS * TRACE_SLOTS;
  if (host_out) DQZ_HIP(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_dqz_trace), bytes));
  if (clear) {
    void* p = nullptr;
    DQZ_HIP(hipGetSymbolAddress(&p, HIP_SYMBOL(g_dqz_trace)));
    DQZ_HIP(hipMemset(p, 0, bytes));
  }
  return DQZ_OK;
}
#endif

// ---------------------------------------------------------------------------
// Atari observation preprocessing (processors.py:488-497)

struct dqz_frame_plan {
  FramePlan p{};
  void* block;
};

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for the BILINEAR
// filter (support 1) on one axis with box (0, in_size): bounds[2 * o] =
// first source index, bounds[2 * o + 1] = count; k[o * ksize + i] = int32
// weights with 22 fractional bits.
static int pil_bilinear_coeffs(int in_size, int out_size, std::vector<int32_t>& bounds, std::vector<int32_t>& k) {
  const double scale = (double)((float)in_size - 0.0f) / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  const int ksize = (int)std::ceil(support) * 2 + 1;
  const double ss = 1.0 / filterscale;
  bounds.assign(2 * out_size, 0);
  k.assign((size_t)out_size * ksize, 0);
  std::vector<double> w(ksize);
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = 0.0 + (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
      double t = (x + xmin - center + 0.5) * ss;
      if (t < 0.0) t = -t;
      w[x] = t < 1.0 ? 1.0 - t : 0.0;
      ww += w[x];
    }
    for (int x = 0; x < xmax; ++x) {
      const double v = ww != 0.0 ? w[x] / ww : w[x];
      k[(size_t)xx * ksize + x] = v < 0 ? (int32_t)(-0.5 + v * (1 << FR_PREC)) : (int32_t)(0.5 + v * (1 << FR_PREC));
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
  }
  return ksize;
}

extern "C" {

int dqz_frame_plan_create(int in_h, int in_w, int out_h, int out_w, dqz_frame_plan** out) {
  if (!out) return fail(DQZ_ERR_INVALID, "null argument");
  if (in_h < 1 || in_w < 1 || out_h < 1 || out_w < 1 || in_h > 4096 || in_w > 4096 || out_h > 4096 || out_w > 4096)
    return fail(DQZ_ERR_INVALID, "frame sizes must be in [1, 4096]");
  std::vector<int32_t> hb, hk, vb, vk;
  const int kh = pil_bilinear_coeffs(in_w, out_w, hb, hk);
  const int kv = pil_bilinear_coeffs(in_h, out_h, vb, vk);
  int max_band = 0;
  for (int yy0 = 0; yy0 < out_h; yy0 += FR_ROWS) {
    const int yy1 = std::min(yy0 + FR_ROWS, out_h);
    max_band = std::max(max_band, vb[2 * (yy1 - 1)] + vb[2 * (yy1 - 1) + 1] - vb[2 * yy0]);
  }
  const size_t smem = (size_t)max_band * (in_w + out_w);
  if (smem > 64 * 1024) return fail(DQZ_ERR_INVALID, "frame too large for one workgroup's band (%zu B of LDS)", smem);
  const size_t n = hb.size() + hk.size() + vb.size() + vk.size();
  dqz_frame_plan* P = new dqz_frame_plan();
  if (hipMalloc(&P->block, n * sizeof(int32_t)) != hipSuccess) {
    delete P;
    return fail(DQZ_ERR_HIP, "hipMalloc of the resize tables failed");
  }
  std::vector<int32_t> all;
  all.reserve(n);
  all.insert(all.end(), hb.begin(), hb.end());
  all.insert(all.end(), hk.begin(), hk.end());
  all.insert(all.end(), vb.begin(), vb.end());
  all.insert(all.end(), vk.begin(), vk.end());
  if (hipMemcpy(P->block, all.data(), n * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(P->block);
    delete P;
    return fail(DQZ_ERR_HIP, "upload of the resize tables failed");
  }
  const int32_t* d = static_cast<const int32_t*>(P->block);
  P->p = FramePlan{in_h, in_w, out_h, out_w, kh, kv, max_band, d, d + hb.size(), d + hb.size() + hk.size(),
                   d + hb.size() + hk.size() + vb.size()};
  *out = P;
  return DQZ_OK;
}

int dqz_frame_plan_destroy(dqz_frame_plan* P) {
  if (!P) return DQZ_OK;
  if (P->block) (void)hipFree(P->block);
  delete P;
  return DQZ_OK;
}

int dqz_atari_frame(const dqz_frame_plan* P, const uint8_t* rgb, int n, uint8_t* out, void* stream) {
  if (!P || !rgb || !out) return fail(DQZ_ERR_INVALID, "null argument");
  if (n < 1 || n > 8) return fail(DQZ_ERR_INVALID, "n must be in [1, 8]");
  const void *drgb = nullptr, *dout = nullptr;
  if (int rc = device_view(rgb, &drgb, "rgb")) return rc;
  if (int rc = device_view(out, &dout, "out")) return rc;
  if (P->p.in_w % 4 == 0 && reinterpret_cast<uintptr_t>(drgb) % 4)
    return fail(DQZ_ERR_INVALID, "rgb must be 4-byte aligned");
  const int64_t stride = (int64_t)P->p.in_h * P->p.in_w * 3;
  const size_t smem = (size_t)P->p.max_band * (P->p.in_w + P->p.out_w);
  hipLaunchKernelGGL(atari_frame_kernel, dim3((P->p.out_h + FR_ROWS - 1) / FR_ROWS), dim3(256), smem,
                     (hipStream_t)stream, P->p, static_cast<const uint8_t*>(drgb), n, stride,
                     static_cast<uint8_t*>(const_cast<void*>(dout)));
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

}  // extern "C"

