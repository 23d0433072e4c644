// census.hpp — device side of the nonsense-transition experiment
// (dqn_mgsc_batched_nonsense_transitions/agent.py:277-310): composing one
// stored transition from five others (dqz_store_jumble) and the census of the
// learned logits by class (dqz_logits_census).
//
// The census is three launches over the live window of the FIFO, none of
// which waits for another workgroup:
//   census_scan_kernel   per chunk of 4096 window positions: max / min /
//                        count by class                      -> CensusScan
//   census_mass_kernel   m = max over the chunks' maxima, then per chunk the
//                        float64 sums of exp(x - m) by class -> CensusMass
//   census_final_kernel  one workgroup: the partials in a fixed order, the
//                        five probes, the update of the caller's dqz_census
// Min, max and counts are order-free; every float64 sum is taken lane by lane
// in a fixed order and then through the fixed shuffle tree of block_sum_f64,
// so equal inputs give equal bits.
#pragma once
#include "meta.hpp"  // block_max_f32
#include "sampling.hpp"

namespace dqz {

struct CensusScan {
  float mx[2], mn[2];
  int64_t cnt[2];
};
struct CensusMass {
  double s[2];
};

// absolute slot of window position i (left_head < capacity, i < size <= capacity)
__device__ __forceinline__ int64_t census_slot(int64_t left_head, int64_t i, int64_t capacity) {
  const int64_t a = left_head + i;
  return a >= capacity ? a - capacity : a;
}

__device__ __forceinline__ int64_t block_sum_i64(int64_t v, int64_t* sbuf) {
  for (int o = 32; o > 0; o >>= 1) v += (int64_t)__shfl_xor((long long)v, o, 64);
  if ((threadIdx.x & 63) == 0) sbuf[threadIdx.x >> 6] = v;
  __syncthreads();
  int64_t r = sbuf[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w) r += sbuf[w];
  __syncthreads();
  return r;
}

DQZ_OTHER_KERNEL __launch_bounds__(SM_THREADS) void census_scan_kernel(const float* __restrict__ x,
                                                                  const uint8_t* __restrict__ flags,
                                                                  int64_t capacity, int64_t left_head, int64_t size,
                                                                  CensusScan* __restrict__ part) {
  __shared__ float sf[SM_THREADS / 64];
  __shared__ int64_t si[SM_THREADS / 64];
  const int64_t base = (int64_t)blockIdx.x * SM_CHUNK;
  float mx[2] = {-INFINITY, -INFINITY}, mn[2] = {INFINITY, INFINITY};
  int64_t cnt[2] = {0, 0};
  for (int k = 0; k < SM_CHUNK / SM_THREADS; ++k) {
    const int64_t i = base + threadIdx.x + k * SM_THREADS;
    if (i >= size) break;
    const int64_t s = census_slot(left_head, i, capacity);
    const float v = x[s];
    const int c = flags[s] != 0;
    mx[c] = fmaxf(mx[c], v);
    mn[c] = fminf(mn[c], v);
    ++cnt[c];
  }
  CensusScan r;
  for (int c = 0; c < 2; ++c) {
    r.mx[c] = block_max_f32(mx[c], sf);
    r.mn[c] = -block_max_f32(-mn[c], sf);
    r.cnt[c] = block_sum_i64(cnt[c], si);
  }
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

DQZ_OTHER_KERNEL __launch_bounds__(SM_THREADS) void census_mass_kernel(const float* __restrict__ x,
                                                                  const uint8_t* __restrict__ flags,
                                                                  int64_t capacity, int64_t left_head, int64_t size,
                                                                  const CensusScan* __restrict__ scan, int nparts,
                                                                  CensusMass* __restrict__ part) {
  __shared__ float sf[SM_THREADS / 64];
  __shared__ double sd[SM_THREADS / 64];
  float m = -INFINITY;
  for (int k = threadIdx.x; k < nparts; k += SM_THREADS) m = fmaxf(m, fmaxf(scan[k].mx[0], scan[k].mx[1]));
  m = block_max_f32(m, sf);
  const int64_t base = (int64_t)blockIdx.x * SM_CHUNK;
  double acc[2] = {0.0, 0.0};
  for (int k = 0; k < SM_CHUNK / SM_THREADS; ++k) {
    const int64_t i = base + threadIdx.x + k * SM_THREADS;
    if (i >= size) break;
    const int64_t s = census_slot(left_head, i, capacity);
    acc[flags[s] != 0] += run_term(x[s], m);
  }
  CensusMass r;
  r.s[0] = block_sum_f64(acc[0], sd);
  r.s[1] = block_sum_f64(acc[1], sd);
  if (threadIdx.x == 0) part[blockIdx.x] = r;
}

DQZ_OTHER_KERNEL __launch_bounds__(SM_THREADS) void census_final_kernel(const float* __restrict__ x,
                                                                   const uint8_t* __restrict__ flags,
                                                                   int64_t capacity, int64_t left_head, int64_t size,
                                                                   const CensusScan* __restrict__ scan,
                                                                   const CensusMass* __restrict__ mass, int nparts,
                                                                   dqz_census* __restrict__ out) {
  __shared__ float sf[SM_THREADS / 64];
  __shared__ double sd[SM_THREADS / 64];
  __shared__ int64_t si[SM_THREADS / 64];
  float mx[2] = {-INFINITY, -INFINITY}, mn[2] = {INFINITY, INFINITY};
  int64_t cnt[2] = {0, 0};
  double sum[2] = {0.0, 0.0};
  for (int k = threadIdx.x; k < nparts; k += SM_THREADS) {
    for (int c = 0; c < 2; ++c) {
      mx[c] = fmaxf(mx[c], scan[k].mx[c]);
      mn[c] = fminf(mn[c], scan[k].mn[c]);
      cnt[c] += scan[k].cnt[c];
      sum[c] += mass[k].s[c];
    }
  }
  for (int c = 0; c < 2; ++c) {
    mx[c] = block_max_f32(mx[c], sf);
    mn[c] = -block_max_f32(-mn[c], sf);
    cnt[c] = block_sum_i64(cnt[c], si);
    sum[c] = block_sum_f64(sum[c], sd);
  }
  if (threadIdx.x != 0) return;
  const double all = sum[0] + sum[1];
  for (int c = 0; c < 2; ++c) {
    dqz_census_class& o = out->cls[c];
    o.max_seen = fmaxf(o.max_seen, mx[c]);
    o.min_seen = fminf(o.min_seen, mn[c]);
    o.count = cnt[c];
    o.mass = all > 0.0 ? sum[c] / all : 0.0;
  }
  out->calls += 1;
  if (size == 0) return;
  // the reference's elif chain: exit, 3rd_quarter, 2nd_quarter, 1st_quarter,
  // entry; a position counts for the first probe it matches.  Stored in the
  // order entry, 1st, 2nd, 3rd, exit.
  const int64_t pos[5] = {0, size / 4, size / 2, 3 * (size / 4), size - 1};
  for (int p = 0; p < 5; ++p) {
    bool taken = false;
    for (int e = 0; e < p; ++e) taken = taken || pos[e] == pos[p];
    if (taken) continue;
    const int64_t s = census_slot(left_head, pos[p], capacity);
    dqz_census_class& o = out->cls[flags[s] != 0];
    o.probe_sum[4 - p] += (double)x[s];
    o.probe_num[4 - p] += 1;
  }
}

// dqz_store_jumble: workgroup c copies the frame of channel c (441 x 16 B,
// pool row to pool row) and writes fidx[slot][c]; workgroup 0 also copies the
// three scalars and sets the flag.  Each workgroup reads its source fidx entry
// into a register before anybody writes, and writes only fidx[slot][c], so a
// destination that is also a source needs no ordering between workgroups.
DQZ_OTHER_KERNEL __launch_bounds__(256) void store_jumble_kernel(uint8_t* pool, int32_t* fidx, int32_t* action,
                                                            float* reward, float* discount, dqz_jumble j) {
  constexpr int Q = FB / 16;  // 441
  const int c = blockIdx.x;
  const int64_t src = c < 4 ? j.src_s_tm1 : j.src_s_t;
  const int32_t row = fidx[src * 8 + c];
  int32_t a = 0;
  float r = 0.f, d = 0.f;
  if (c == 0 && threadIdx.x == 0) {
    a = action[j.src_action];
    r = reward[j.src_reward];
    d = discount[j.src_discount];
  }
  __syncthreads();  // every lane holds `row` before lane 0 overwrites the entry (slot may be src)
  if (row >= 0) {
    const uint4* from = reinterpret_cast<const uint4*>(pool + (int64_t)row * FB);
    uint4* to = reinterpret_cast<uint4*>(pool + (int64_t)j.frame_rows[c] * FB);
    for (int k = threadIdx.x; k < Q; k += 256) to[k] = from[k];
  }
  if (threadIdx.x == 0) {
    fidx[j.slot * 8 + c] = row >= 0 ? j.frame_rows[c] : -1;
    if (c == 0) {
      action[j.slot] = a;
      reward[j.slot] = r;
      discount[j.slot] = d;
      if (j.flags) j.flags[j.slot] = 1;
    }
  }
}

}  // namespace dqz
