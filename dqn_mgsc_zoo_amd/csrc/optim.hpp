// optim.hpp — optimizers applied to a finished gradient (dqz_optimizer_*):
// optax.clip_by_global_norm, optax.adam and plain optax.rmsprop
// (optax 0.1.2: clipping.py clip_by_global_norm, transform.py scale_by_adam /
// scale_by_rms), the optimizer chain of c51 / qrdqn / iqn / rainbow
// (c51/run_atari.py:210-216).  Centered RMSProp stays fused into the learner
// step's own kernels (Rms::step); these kernels live in the other code object
// and run after a learner step in gradient-output mode.
//
//   opt_norm_kernel   sum g^2 over the leaves (padding excluded) as one
//                     float64 partial per workgroup.  Whoever needs the norm
//                     (the apply, dqz_optimizer_outputs) folds the partials
//                     itself in index order (opt_fold_norm): no float atomics,
//                     no arrival ticket, equal inputs give equal bits, and the
//                     norm never leaves the device.
//   opt_apply_kernel  one float4 pass over theta / m / v / g.  The arithmetic
//                     is float64 inside (IEEE division and square root, no
//                     approximate rcp / rsq) and every stored value is rounded
//                     to float32 once.  Padding lanes are never written.
//   opt_count_kernel  Adam's count (a device int32) advances in a one-thread
//                     launch behind the apply, so no workgroup of a step sees
//                     the advanced value and a captured graph of k steps
//                     replays.  (An arrival ticket in the apply instead costs
//                     one same-address atomic per workgroup, which a single
//                     word takes at about 88 per microsecond: measured, the
//                     800-workgroup apply took 17 us with it)
#pragma once
#include "sampling.hpp"  // block_sum_f64

namespace dqz {

constexpr int OPT_THREADS = 256;
constexpr int OPT_UNROLL = 2;  // float4s per thread and array, loaded before the first use

// The parameter layout in float4 units: leaf k holds floats [4 off4[k], end[k]),
// its padding runs to the next leaf's start (a multiple of 16 float4s).  NL
// leaves: ten for the DQN and the wide heads' networks (the kernels below, which
// are what they were), twenty for the Rainbow network (their _rb twins).
template <int NL>
struct OptLeavesT {
  int64_t off4[NL], end[NL];
  int64_t n4;  // total / 4
};
using OptLeaves = OptLeavesT<DQZ_NUM_LEAVES>;
using OptLeavesRb = OptLeavesT<DQZ_RAINBOW_NUM_LEAVES>;

// real (non-padding) floats of float4 i: 0..4
template <int NL>
__device__ __forceinline__ int opt_real(const OptLeavesT<NL>& lv, int64_t i) {
  int64_t end = lv.end[0];
#pragma unroll
  for (int k = 1; k < NL; ++k) end = i >= lv.off4[k] ? lv.end[k] : end;
  const int64_t r = end - 4 * i;
  return r < 0 ? 0 : r > 4 ? 4 : (int)r;
}

constexpr int OPT_NORM_UNROLL = 4;  // float4s per thread of the norm pass

// part[blockIdx.x] = sum of g^2 over this workgroup's float4s, padding excluded
template <int NL>
__device__ __forceinline__ void opt_norm_body(const float4* __restrict__ g, const OptLeavesT<NL>& lv,
                                              double* __restrict__ part) {
  __shared__ double sbuf[OPT_THREADS / 64];
  const int64_t i0 = (int64_t)blockIdx.x * (OPT_THREADS * OPT_NORM_UNROLL) + threadIdx.x;
  float4 v[OPT_NORM_UNROLL];
  int r[OPT_NORM_UNROLL];
#pragma unroll
  for (int u = 0; u < OPT_NORM_UNROLL; ++u) {
    const int64_t i = i0 + u * OPT_THREADS;
    r[u] = i < lv.n4 ? opt_real(lv, i) : 0;
    v[u] = r[u] > 0 ? g[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  double acc = 0.0;
#pragma unroll
  for (int u = 0; u < OPT_NORM_UNROLL; ++u) {  // x^2 is exact in float64; one rounding per add, in lane order
    const double x = v[u].x, y = v[u].y, z = v[u].z, w = v[u].w;
    if (r[u] > 0) acc += x * x;
    if (r[u] > 1) acc += y * y;
    if (r[u] > 2) acc += z * z;
    if (r[u] > 3) acc += w * w;
  }
  acc = block_sum_f64(acc, sbuf);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}
DQZ_OTHER_KERNEL __launch_bounds__(OPT_THREADS) void opt_norm_kernel(const float4* __restrict__ g, OptLeaves lv,
                                                                double* __restrict__ part) {
  opt_norm_body(g, lv, part);
}
DQZ_OTHER_KERNEL __launch_bounds__(OPT_THREADS) void opt_norm_rb_kernel(const float4* __restrict__ g, OptLeavesRb lv,
                                                                   double* __restrict__ part) {
  opt_norm_body(g, lv, part);
}

// sqrt of the partials' sum, the same bits in every workgroup that forms it:
// thread t adds parts t, t + 256, ... in order, then block_sum_f64's fixed tree.
__device__ __forceinline__ double opt_fold_norm(const double* __restrict__ part, int nparts, double* sbuf) {
  double s = 0.0;
  for (int k = threadIdx.x; k < nparts; k += OPT_THREADS) s += part[k];
  return sqrt(block_sum_f64(s, sbuf));
}

template <int NL>
struct OptArgsT {
  float4* th;
  float4* m;  // Adam's first moment (RMSProp: unused)
  float4* v;  // Adam's second moment / RMSProp's nu
  const float4* g;
  OptLeavesT<NL> lv;
  int kind;             // DQZ_OPT_*
  double lr, b1, b2, decay, eps;  // the config's floats, widened
  double clip;          // max_global_grad_norm (used when part != null)
  const double* part;   // opt_norm_kernel's partials of this gradient, or null: no clipping
  int nparts;
  const int32_t* count; // Adam's count (device), advanced by opt_count_kernel behind this launch
};
using OptArgs = OptArgsT<DQZ_NUM_LEAVES>;
using OptArgsRb = OptArgsT<DQZ_RAINBOW_NUM_LEAVES>;

struct OptScalars {
  double scale;       // clip_by_global_norm's factor (1 when inactive)
  double ibc1, ibc2;  // 1 / (1 - b^count), count already advanced
};

// One element.  optax 0.1.2, with the float32 state rounded once per step:
//   adam  m <- b1 m + (1 - b1) g;  v <- b2 v + (1 - b2) g^2
//         theta <- theta - lr (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps)
//   rms   nu <- d nu + (1 - d) g^2;  theta <- theta - lr g / sqrt(nu + eps)
template <bool ADAM, int NL>
__device__ __forceinline__ void opt_elem(const OptArgsT<NL>& a, const OptScalars& s, float gf, float& th, float& m,
                                         float& v) {
  const double g = (double)gf * s.scale;
  if (ADAM) {
    m = (float)__fma_rn(a.b1, (double)m, (1.0 - a.b1) * g);
    v = (float)__fma_rn(a.b2, (double)v, (1.0 - a.b2) * (g * g));
    const double u = a.lr * ((double)m * s.ibc1) / (sqrt((double)v * s.ibc2) + a.eps);
    th = (float)((double)th - u);
  } else {
    v = (float)__fma_rn(a.decay, (double)v, (1.0 - a.decay) * (g * g));
    const double u = a.lr * g / sqrt((double)v + a.eps);
    th = (float)((double)th - u);
  }
}

template <bool ADAM, int NL>
__device__ __forceinline__ void opt_apply_body(const OptArgsT<NL>& a) {
  __shared__ OptScalars s_sc;
  __shared__ double sbuf[OPT_THREADS / 64];
  // this thread's float4s first: the loads fly while the norm is folded
  const int64_t i0 = (int64_t)blockIdx.x * (OPT_THREADS * OPT_UNROLL) + threadIdx.x;
  float4 g[OPT_UNROLL], th[OPT_UNROLL], m[OPT_UNROLL], v[OPT_UNROLL];
  int r[OPT_UNROLL];
#pragma unroll
  for (int u = 0; u < OPT_UNROLL; ++u) {
    const int64_t i = i0 + u * OPT_THREADS;
    r[u] = i < a.lv.n4 ? opt_real(a.lv, i) : 0;
    if (r[u] > 0) {
      g[u] = a.g[i];
      th[u] = a.th[i];
      v[u] = a.v[i];
      if (ADAM) m[u] = a.m[i];
    }
  }
  double norm = 0.0;
  if (a.part) norm = opt_fold_norm(a.part, a.nparts, sbuf);  // uniform branch: every thread folds
  if (threadIdx.x == 0) {
    OptScalars sc{1.0, 1.0, 1.0};
    if (a.part && !(norm < a.clip)) sc.scale = a.clip / norm;  // (g / norm) * max_norm
    if (ADAM) {
      const int cnt = *a.count + 1;
      sc.ibc1 = 1.0 / (1.0 - pow(a.b1, (double)cnt));
      sc.ibc2 = 1.0 / (1.0 - pow(a.b2, (double)cnt));
    }
    s_sc = sc;
  }
  __syncthreads();
  const OptScalars sc = s_sc;
#pragma unroll
  for (int u = 0; u < OPT_UNROLL; ++u) {
    if (r[u] == 0) continue;  // a float4 of padding: not touched
    const int64_t i = i0 + u * OPT_THREADS;
    // padding lanes keep the bits they were loaded with
    if (r[u] > 0) opt_elem<ADAM>(a, sc, g[u].x, th[u].x, m[u].x, v[u].x);
    if (r[u] > 1) opt_elem<ADAM>(a, sc, g[u].y, th[u].y, m[u].y, v[u].y);
    if (r[u] > 2) opt_elem<ADAM>(a, sc, g[u].z, th[u].z, m[u].z, v[u].z);
    if (r[u] > 3) opt_elem<ADAM>(a, sc, g[u].w, th[u].w, m[u].w, v[u].w);
    a.th[i] = th[u];
    a.v[i] = v[u];
    if (ADAM) a.m[i] = m[u];
  }
}

DQZ_OTHER_KERNEL __launch_bounds__(OPT_THREADS) void opt_adam_kernel(OptArgs a) { opt_apply_body<true>(a); }
DQZ_OTHER_KERNEL __launch_bounds__(OPT_THREADS) void opt_rms_kernel(OptArgs a) { opt_apply_body<false>(a); }
DQZ_OTHER_KERNEL __launch_bounds__(OPT_THREADS) void opt_adam_rb_kernel(OptArgsRb a) { opt_apply_body<true>(a); }
DQZ_OTHER_KERNEL __launch_bounds__(OPT_THREADS) void opt_rms_rb_kernel(OptArgsRb a) { opt_apply_body<false>(a); }

// count <- count + 1, behind the apply that read it
DQZ_OTHER_KERNEL void opt_count_kernel(int32_t* count) {
  if (threadIdx.x == 0) *count = *count + 1;
}

// the norm as float32 for the caller (dqz_optimizer_outputs), one workgroup
DQZ_OTHER_KERNEL __launch_bounds__(OPT_THREADS) void opt_norm_out_kernel(const double* __restrict__ part, int nparts,
                                                                    float* __restrict__ out) {
  __shared__ double sbuf[OPT_THREADS / 64];
  const double norm = opt_fold_norm(part, nparts, sbuf);
  if (threadIdx.x == 0) *out = (float)norm;
}

}  // namespace dqz
