// rainbow.hpp — the noisy dueling categorical network of the Rainbow agent
// (rainbow/agent.py, networks.py rainbow_atari_network) around the learner
// step's torso and the categorical head's loss.  These kernels live in the
// other code object (learner.hip) and meet the step at launch boundaries only.
//
// A noisy layer is  x Wmu + bmu + ((e_in * x) Wsig + bsig) * e_out:  the noise
// scales activations, never weights, so each 3136 x 512 product is a plain
// GEMM that the step's own fc1 kernels perform (forward: four launches on y3
// and on its e_in-scaled copies; dX: four launches; dW: the backward launch's
// for A1-mu, rb_fc1_dw_kernel for the other three).  What is new is small:
//
//   rb_noise_kernel    e = sign(t) sqrt|t|, t a standard normal truncated to
//                      [-2, 2], by inverting the CDF on dqz_uniform_philox's
//                      uniforms.
//   rb_scale_kernel    the two scaled copies e_in[z] * y3[z] (A1's and V1's).
//   rb_hidden_kernel   h = relu(mu + bmu + (sig + bsig) e_out) of both streams
//                      from the four split-K partial buffers, each reduced in
//                      head_body's order (bias first, then s = 0 .. S - 1).
//   rb_logits_kernel   adv [Z][B][A N] and val [Z][B][N]: one k-ordered fma
//                      chain per output and per part (mu, sigma).
//   rb_combine_kernel  q_logits = val + adv - mean_a adv, the mean summed in
//                      action order.  c51_head_kernel<.. | WIDE_NO_DZ1> then
//                      forms the loss, a*, the priority and dl.
//   rb_dhidden_kernel  dadv = dl (delta(a, a_b) - 1 / A), dval = dl; dz_adv and
//                      dz_val through the noisy fc2 transposes and relu', and
//                      their e_out1-scaled copies.  A wave per W2 row.
//   rb_fc2_grad_kernel every element of the A2 / V2 leaves' gradients and of the
//                      fc1 biases' that the step's update does not own, summed
//                      in sample order by one thread per element.
//   rb_fc1_dw_kernel   V1-mu, A1-sigma and V1-sigma dW: x^T g over the batch,
//                      in sample order, a float4 of columns per thread.
//   rb_dx_combine_kernel  dy3 from the four dX products (e_in on the sigma ones).
//   rb_act_kernel      argmax_a q and its value per state (no epsilon).
// Every sum has a fixed order: equal inputs give equal bits.
#pragma once
#include "common.hpp"
#include "c51.hpp"       // C51_MAXOUT, C51_MAXN
#include "fwd.hpp"       // FC1_S
#include "sampling.hpp"  // philox_uniform

namespace dqz {

// Offsets (floats) of the fourteen fc leaves in the parameter buffer and of the eight noise vectors in one
// application's noise (the reference's draw order).
struct RbLeaves {
  int64_t a1w, a1b, a1sw, a1sb, a2w, a2sw, a2sb, v1w, v1b, v1sw, v1sb, v2w, v2sw, v2sb;
};
struct RbNoise {
  int a1_in, a1_out, a2_in, a2_out, v1_in, v1_out, v2_in, v2_out, len;
};
inline RbNoise rb_noise_layout(int A, int N) {
  const int AN = A * N;
  return RbNoise{0, FLAT, FLAT + HID, FLAT + 2 * HID, FLAT + 2 * HID + AN, 2 * FLAT + 2 * HID + AN,
                 2 * FLAT + 3 * HID + AN, 2 * FLAT + 4 * HID + AN, 2 * FLAT + 4 * HID + AN + N};
}

// One element per thread over ceil(n / 256) workgroups (a float64 erfinv each: one workgroup took longer than the
// rest of the step); every workgroup reads the counter, and the one-thread launch behind this one advances it, as
// opt_count_kernel does for Adam's count.
DQZ_OTHER_KERNEL __launch_bounds__(256) void rb_noise_kernel(uint64_t seed, const uint64_t* counter, int n,
                                                        float* out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double hi = erf(1.4142135623730951), lo = -hi;
  const double u = philox_uniform(seed, *counter, i);
  double t = 1.4142135623730951 * erfinv(lo + u * (hi - lo));
  t = fmin(fmax(t, -2.0), 2.0);
  const float r = (float)sqrt(fabs(t));
  out[i] = t < 0.0 ? -r : r;
}
DQZ_OTHER_KERNEL void rb_noise_advance_kernel(uint64_t* counter, int n) {
  if (threadIdx.x == 0) *counter = *counter + (uint64_t)n;
}

struct RbScaleArgs {
  const float* y3;     // [Z][B][3136]
  const float* noise;  // [Z][len]
  RbNoise nl;
  int Z, B;
  float* ys;  // [2][Z][B][3136]: A1's copy, V1's copy
};

DQZ_OTHER_KERNEL __launch_bounds__(256) void rb_scale_kernel(RbScaleArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // float4 index in [Z][B][3136 / 4]
  const int64_t per = (int64_t)a.B * (FLAT / 4);
  if (i >= a.Z * per) return;
  const int z = (int)(i / per), k4 = (int)(i % (FLAT / 4));
  const float4 y = reinterpret_cast<const float4*>(a.y3)[i];
  const float* e = a.noise + (int64_t)z * a.nl.len;
  const float* ea = e + a.nl.a1_in + 4 * k4;
  const float* ev = e + a.nl.v1_in + 4 * k4;  // not 16-byte aligned for every A N: scalar loads
  reinterpret_cast<float4*>(a.ys)[i] = make_float4(y.x * ea[0], y.y * ea[1], y.z * ea[2], y.w * ea[3]);
  reinterpret_cast<float4*>(a.ys)[a.Z * per + i] = make_float4(y.x * ev[0], y.y * ev[1], y.z * ev[2], y.w * ev[3]);
}

struct RbHiddenArgs {
  const float* part[4];  // split-K partials [Z][S][B][512] of A1-mu, V1-mu, A1-sigma, V1-sigma
  int S;
  NetZ nz;
  RbLeaves lf;
  const float* noise;
  RbNoise nl;
  int Z, B;
  float *h_adv, *h_val;  // [Z][B][512]
};

DQZ_OTHER_KERNEL __launch_bounds__(256) void rb_hidden_kernel(RbHiddenArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // [Z][B][512]
  if (i >= (int64_t)a.Z * a.B * HID) return;
  const int j = (int)(i % HID), b = (int)((i / HID) % a.B), z = (int)(i / ((int64_t)HID * a.B));
  const float* th = a.nz.p[z];
  const float* e = a.noise + (int64_t)z * a.nl.len;
  float acc[4] = {th[a.lf.a1b + j], th[a.lf.v1b + j], th[a.lf.a1sb + j], th[a.lf.v1sb + j]};
  for (int s = 0; s < a.S; ++s) {
    const int64_t o = (((int64_t)z * a.S + s) * a.B + b) * HID + j;
#pragma unroll
    for (int p = 0; p < 4; ++p) acc[p] += a.part[p][o];
  }
  a.h_adv[i] = relu(acc[0] + acc[2] * e[a.nl.a1_out + j]);
  a.h_val[i] = relu(acc[1] + acc[3] * e[a.nl.v1_out + j]);
}

struct RbLogitsArgs {
  const float *h_adv, *h_val;  // [Z][B][512]
  NetZ nz;
  RbLeaves lf;
  const float* noise;
  RbNoise nl;
  int Z, B, AN, N;
  float* adv;  // [Z][B][A N]
  float* val;  // [Z][B][N]
};

// Grid (ceil((A N + N) / 256), Z * B), 256 threads: thread c of the A N + N outputs of one sample of one copy (the
// advantage's first, then the value's).  The sample's two hidden rows and their e_in2-scaled copies are staged
// in LDS; the W2 reads are coalesced across the block's columns.  (Four samples per workgroup, each W2 operand
// loaded once for the four, measured slower: launches 2-8 of the step 65 -> 88 us at A = 6, a quarter of the
// workgroups on the same 512-step dependent chain)
DQZ_OTHER_KERNEL __launch_bounds__(256) void rb_logits_kernel(RbLogitsArgs a) {
  __shared__ float s_h[2][HID], s_he[2][HID];
  const int z = blockIdx.y / a.B, b = blockIdx.y % a.B;
  const float* th = a.nz.p[z];
  const float* e = a.noise + (int64_t)z * a.nl.len;
  for (int k = threadIdx.x; k < HID; k += 256) {
    const float ha = a.h_adv[((int64_t)z * a.B + b) * HID + k], hv = a.h_val[((int64_t)z * a.B + b) * HID + k];
    s_h[0][k] = ha;
    s_h[1][k] = hv;
    s_he[0][k] = ha * e[a.nl.a2_in + k];
    s_he[1][k] = hv * e[a.nl.v2_in + k];
  }
  __syncthreads();
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.AN + a.N) return;
  const int v = c >= a.AN, col = v ? c - a.AN : c, W = v ? a.N : a.AN;
  const float* wm = th + (v ? a.lf.v2w : a.lf.a2w) + col;
  const float* ws = th + (v ? a.lf.v2sw : a.lf.a2sw) + col;
  float m = 0.f, s = 0.f;
#pragma unroll 8
  for (int k = 0; k < HID; ++k) {
    m = __fmaf_rn(s_h[v][k], wm[(int64_t)k * W], m);
    s = __fmaf_rn(s_he[v][k], ws[(int64_t)k * W], s);
  }
  const float bs = th[(v ? a.lf.v2sb : a.lf.a2sb) + col], eo = e[(v ? a.nl.v2_out : a.nl.a2_out) + col];
  const float out = m + (s + bs) * eo;
  if (v)
    a.val[((int64_t)z * a.B + b) * a.N + col] = out;
  else
    a.adv[((int64_t)z * a.B + b) * a.AN + col] = out;
}

struct RbCombineArgs {
  const float *adv, *val;
  int Z, B, A, N;
  float* q_logits;  // [Z][B][A N]
};

DQZ_OTHER_KERNEL __launch_bounds__(256) void rb_combine_kernel(RbCombineArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // [Z B][N]
  if (i >= (int64_t)a.Z * a.B * a.N) return;
  const int n = (int)(i % a.N);
  const int64_t zb = i / a.N;
  const float* adv = a.adv + zb * a.A * a.N + n;
  float sum = 0.f;
  for (int k = 0; k < a.A; ++k) sum += adv[k * a.N];
  const float mean = sum / (float)a.A, v = a.val[i];
  for (int k = 0; k < a.A; ++k) a.q_logits[zb * a.A * a.N + k * a.N + n] = v + (adv[k * a.N] - mean);
}

struct RbDhiddenArgs {
  const float* dl;     // [B][N]
  const int32_t* ga;   // [B] taken actions
  const float *h_adv, *h_val;  // application 0's [B][512]
  const float* th;     // online parameters
  RbLeaves lf;
  const float* noise;  // application 0's
  RbNoise nl;
  int B, A, N;
  float *dz_adv, *dz_val, *dz_adv_e, *dz_val_e;  // [B][512]
};

// Grid (B, 512 / RB_DH_ROWS), 512 threads: a workgroup takes RB_DH_ROWS W2 rows of one sample (one workgroup per
// sample took 95 us at A = 6 and 272 us at A = 18, 32 workgroups on 256 CUs).  g = dadv (A N) and dval (N) and
// their e_out2-scaled copies go to LDS; wave w then takes the workgroup's rows w, w + 8, ...: lane l sums the
// row's columns l, l + 64, ... in order, wave_sum folds the 64 partials in its fixed order.
constexpr int RB_DH_ROWS = 64;
DQZ_OTHER_KERNEL __launch_bounds__(512) void rb_dhidden_kernel(RbDhiddenArgs a) {
  __shared__ float s_g[C51_MAXOUT + C51_MAXN], s_ge[C51_MAXOUT + C51_MAXN];
  const int b = blockIdx.x, AN = a.A * a.N, N = a.N;
  const int ab = min(max(a.ga[b], 0), a.A - 1);
  const float inv = 1.f / (float)a.A;
  for (int c = threadIdx.x; c < AN + N; c += 512) {
    float g, eo;
    if (c < AN) {
      g = a.dl[(int64_t)b * N + c % N] * ((c / N == ab ? 1.f : 0.f) - inv);
      eo = a.noise[a.nl.a2_out + c];
    } else {
      g = a.dl[(int64_t)b * N + (c - AN)];
      eo = a.noise[a.nl.v2_out + (c - AN)];
    }
    s_g[c] = g;
    s_ge[c] = g * eo;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = blockIdx.y * RB_DH_ROWS + wave; j < (blockIdx.y + 1) * RB_DH_ROWS; j += 8) {
    float am = 0.f, as = 0.f, vm = 0.f, vs = 0.f;
    const float* wm = a.th + a.lf.a2w + (int64_t)j * AN;
    const float* ws = a.th + a.lf.a2sw + (int64_t)j * AN;
    for (int c = lane; c < AN; c += 64) {
      am = __fmaf_rn(s_g[c], wm[c], am);
      as = __fmaf_rn(s_ge[c], ws[c], as);
    }
    if (lane < N) {
      vm = s_g[AN + lane] * a.th[a.lf.v2w + (int64_t)j * N + lane];
      vs = s_ge[AN + lane] * a.th[a.lf.v2sw + (int64_t)j * N + lane];
    }
    am = wave_sum(am);
    as = wave_sum(as);
    vm = wave_sum(vm);
    vs = wave_sum(vs);
    if (lane == 0) {
      const int64_t o = (int64_t)b * HID + j;
      const float da = a.h_adv[o] > 0.f ? am + a.noise[a.nl.a2_in + j] * as : 0.f;
      const float dv = a.h_val[o] > 0.f ? vm + a.noise[a.nl.v2_in + j] * vs : 0.f;
      a.dz_adv[o] = da;
      a.dz_val[o] = dv;
      a.dz_adv_e[o] = da * a.noise[a.nl.a1_out + j];
      a.dz_val_e[o] = dv * a.noise[a.nl.v1_out + j];
    }
  }
}

struct RbFc2GradArgs {
  const float* dl;
  const int32_t* ga;
  const float *h_adv, *h_val;                    // [B][512]
  const float *dz_val, *dz_adv_e, *dz_val_e;     // [B][512]
  const float* noise;
  RbNoise nl;
  RbLeaves lf;
  int B, A, N;
  float* g;  // the gradient buffer (parameter layout)
  int acc;   // 1: add into it
};

__host__ __device__ inline int64_t rb_fc2_grad_elems(int AN, int N) { return (int64_t)(2 * HID + 1) * (AN + N) + 3 * HID; }

// One thread per element, samples in order:
//   [0, 512 (AN + N))            dWmu of A2 then V2:   sum_b h[b][j] g[b][c]
//   [.., 2 x that)               dWsig:                sum_b (e_in2[j] h[b][j]) (g[b][c] e_out2[c])
//   [.., + AN + N)               dbsig:                sum_b g[b][c] e_out2[c]
//   [.., + 3 x 512)              A1 dbsig, V1 dbmu, V1 dbsig: sums of dz_adv_e, dz_val, dz_val_e
// with g = dl (delta(a, a_b) - 1 / A) for the advantage's columns and dl for the value's.
DQZ_OTHER_KERNEL __launch_bounds__(256) void rb_fc2_grad_kernel(RbFc2GradArgs u) {
  const int AN = u.A * u.N, N = u.N, W = AN + N;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= rb_fc2_grad_elems(AN, N)) return;
  const int64_t nw = (int64_t)HID * W;
  float sum = 0.f;
  float* dst;
  if (e >= 2 * nw + W) {  // the fc1 biases
    const int r = (int)(e - 2 * nw - W), which = r / HID, j = r % HID;
    const float* src = which == 0 ? u.dz_adv_e : which == 1 ? u.dz_val : u.dz_val_e;
    for (int b = 0; b < u.B; ++b) sum += src[(int64_t)b * HID + j];
    dst = u.g + (which == 0 ? u.lf.a1sb : which == 1 ? u.lf.v1b : u.lf.v1sb) + j;
  } else {
    const int kind = e < nw ? 0 : e < 2 * nw ? 1 : 2;  // mu w, sigma w, sigma b
    const int64_t r = e - kind * nw;
    const int j = kind == 2 ? 0 : (int)(r / W), c = (int)(r % W);
    const bool v = c >= AN;
    const int col = v ? c - AN : c, a = col / N, k = col % N;
    const float inv = 1.f / (float)u.A;
    const float eo = kind ? u.noise[(v ? u.nl.v2_out : u.nl.a2_out) + col] : 1.f;
    const float ei = kind == 1 ? u.noise[(v ? u.nl.v2_in : u.nl.a2_in) + j] : 1.f;
    const float* h = v ? u.h_val : u.h_adv;
    for (int b = 0; b < u.B; ++b) {
      float g = u.dl[(int64_t)b * N + k];
      if (!v) g *= (min(max(u.ga[b], 0), u.A - 1) == a ? 1.f : 0.f) - inv;
      if (kind) g *= eo;
      float x = kind == 2 ? 1.f : h[(int64_t)b * HID + j];
      if (kind == 1) x *= ei;
      sum = __fmaf_rn(x, g, sum);
    }
    const int64_t base = kind == 0 ? (v ? u.lf.v2w : u.lf.a2w) : kind == 1 ? (v ? u.lf.v2sw : u.lf.a2sw)
                                                                            : (v ? u.lf.v2sb : u.lf.a2sb);
    dst = u.g + base + (kind == 2 ? col : (int64_t)j * (v ? N : AN) + col);
  }
  *dst = u.acc ? *dst + sum : sum;
}

struct RbFc1DwArgs {
  const float* x[3];   // [B][3136]: y3, A1's scaled copy, V1's scaled copy (application 0)
  const float* g[3];   // [B][512]: dz_val, dz_adv_e, dz_val_e
  int64_t off[3];      // V1-mu w, A1-sigma w, V1-sigma w
  int B;
  float* grad;
  int acc;
};

// Grid (3136 * 128 / 256, 3): thread (k, j4) of product blockIdx.y sums x[b][k] g[b][4 j4 .. + 3] over b in order.
DQZ_OTHER_KERNEL __launch_bounds__(256) void rb_fc1_dw_kernel(RbFc1DwArgs a) {
  const int p = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // [3136][128]
  if (i >= (int64_t)FLAT * (HID / 4)) return;
  const int k = (int)(i / (HID / 4)), j4 = (int)(i % (HID / 4));
  const float* x = a.x[p] + k;
  const float4* g = reinterpret_cast<const float4*>(a.g[p]) + j4;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int b = 0; b < a.B; ++b) {
    const float xv = x[(int64_t)b * FLAT];
    const float4 gv = g[(int64_t)b * (HID / 4)];
    s.x = __fmaf_rn(xv, gv.x, s.x);
    s.y = __fmaf_rn(xv, gv.y, s.y);
    s.z = __fmaf_rn(xv, gv.z, s.z);
    s.w = __fmaf_rn(xv, gv.w, s.w);
  }
  float4* dst = reinterpret_cast<float4*>(a.grad + a.off[p]) + i;
  if (a.acc) {
    const float4 o = *dst;
    s = make_float4(o.x + s.x, o.y + s.y, o.z + s.z, o.w + s.w);
  }
  *dst = s;
}

struct RbDxCombineArgs {
  const float* dx;     // [4][B][3136]: A1-mu, V1-mu, A1-sigma, V1-sigma, each already times relu'(y3)
  const float* noise;  // application 0's
  RbNoise nl;
  int B;
  float* dy3;  // [B][3136]
};

DQZ_OTHER_KERNEL __launch_bounds__(256) void rb_dx_combine_kernel(RbDxCombineArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, n = (int64_t)a.B * FLAT;
  if (i >= n) return;
  const int k = (int)(i % FLAT);
  const float adv = a.dx[i] + a.noise[a.nl.a1_in + k] * a.dx[2 * n + i];
  const float val = a.dx[n + i] + a.noise[a.nl.v1_in + k] * a.dx[3 * n + i];
  a.dy3[i] = adv + val;
}

// action[b] = first argmax_a q[b][a], value[b] = that maximum
DQZ_OTHER_KERNEL void rb_act_kernel(const float* q, int n, int A, dqz_action* out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n) return;
  int am = 0;
  float best = q[(int64_t)b * A];
  for (int k = 1; k < A; ++k) {
    const float v = q[(int64_t)b * A + k];
    if (v > best) {
      best = v;
      am = k;
    }
  }
  out[b].action = am;
  out[b].value = best;
}

}  // namespace dqz
