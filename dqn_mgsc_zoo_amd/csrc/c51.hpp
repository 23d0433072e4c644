// c51.hpp — the categorical (C51) head: fc1 reduce + the A*N-wide fc2 on
// f32 MFMA, rlax.categorical_q_learning per sample, and the fc2 gradient
// (c51/agent.py:36-39,87-107; networks.py:316-335; rlax 0.1.2
// categorical_l2_project / categorical_q_learning).  These kernels live in the
// other code object (learner.hip) and talk to the learner step through launch
// boundaries only: no hand-off words, no spin-waits.
//
//   c51_logits_kernel  h1 = relu(b1 + sum_s partial) of 16 samples of one
//                      network copy into LDS (and to h1), then
//                      logits[16, 64] = h1[16, 512] W2[512, 64 of A*N] + b2 on
//                      v_mfma_f32_16x16x4_f32: exact f32, a k-ordered fma
//                      chain per output.  A sample alone is a GEMV (one MFMA
//                      row of sixteen), so the logits are batched here and the
//                      per-sample part is a launch of its own.
//   c51_head_kernel    one workgroup per sample: softmax and q_values of
//                      every action of every copy (a wave per distribution),
//                      a* = argmax_a q_target, the projection of r + d z under
//                      P[a*] onto the support, the cross-entropy, dlogits of
//                      the taken action and the dz1 row (four lanes per W2
//                      row).  Forward / actor mode stops after q_values (and
//                      the eps-greedy draw).  WIDE_DOUBLE: a* comes from a third
//                      copy, online(s_t) (rlax.categorical_double_q_learning);
//                      WIDE_WEIGHTED: the cotangent carries the sample's
//                      importance weight and clip(|loss_b|, 0, 100) is the
//                      sample's new priority (rainbow/agent.py:85-150,198).
//   c51_fc2_grad_kernel  dW2 / db2 from h1 and dlogits, every element written
//                      (zeros for actions absent from the batch), summed in
//                      sample order by one thread per element.
#pragma once
#include "common.hpp"
#include "fwd.hpp"   // FC1_S
#include "head.hpp"  // eps_greedy

namespace dqz {

constexpr int C51_MAXN = 64;      // atoms per action: one wave covers a distribution
constexpr int C51_MAXOUT = 1024;  // A * N: one sample's logits of one copy fit 4 KB of LDS
constexpr int C51_ROWS = 16;      // samples per logits workgroup (the MFMA's M)
constexpr int C51_COLS = 64;      // outputs per logits workgroup: 4 waves x 16
constexpr int C51_HS = HID + 4;   // LDS row stride of the h1 tile: 16-byte rows, rows r and r + 1 four banks apart

struct C51LogitsArgs {
  const float* fc1p;  // fc1 split-K partials [Z][S][B][512]
  int S;
  float* h1;  // [Z][B][512] (written)
  NetZ nz;
  int64_t b1_off, w2_off, b2_off;
  int Z, B, AN;
  float* logits;  // [Z][B][AN] (written)
};

// Grid (ceil(AN / 64), Z * ceil(B / 16)), 256 threads.  K runs in 32 groups of
// 16: lane (r = lane & 15, q = lane >> 4) reads the four h1 values k = 16 g +
// 4 q + i as one float4 and feeds them to four MFMAs whose B operand is
// W2[16 g + 4 q + i][col]; the MFMA sums over q, so every k is used once.  Two
// accumulators alternate (the 16x16x4 form's dependent latency is above its
// issue interval) and are added at the end: a fixed order, equal bits each run.
// Every global load is issued before its first use: the lane's 128 W2 operands
// at entry, the tile's fc1 partials in two halves of 28 float4 per thread (the
// first form looped over both with a few loads in flight and took 30 us at
// B = 32, a round trip per iteration).
DQZ_OTHER_KERNEL __launch_bounds__(256) void c51_logits_kernel(C51LogitsArgs a) {
  __shared__ __attribute__((aligned(16))) float s_h[C51_ROWS * C51_HS];
  constexpr int SMAX = FC1_S;
  const int tiles = (a.B + C51_ROWS - 1) / C51_ROWS;
  const int z = blockIdx.y / tiles, b0 = (blockIdx.y % tiles) * C51_ROWS;
  const int c0 = blockIdx.x * C51_COLS;
  const float* th = a.nz.p[z];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  // columns past AN repeat the last one and are never stored
  const int col = c0 + wave * 16 + r, colc = min(col, a.AN - 1);
  const float* w2 = th + a.w2_off + colc;
  float wv[HID / 4];
#pragma unroll
  for (int g = 0; g < HID / 16; ++g)
#pragma unroll
    for (int i = 0; i < 4; ++i) wv[4 * g + i] = w2[(int64_t)(16 * g + 4 * q + i) * a.AN];
  const float bias = th[a.b2_off + colc];
  // the h1 tile: thread t owns row t / 16, float4 columns 4 (t % 16) + 64 i; fc1 partials summed in head_body's
  // order (bias first, then s = 0 .. S - 1)
  {
    const int tr = threadIdx.x >> 4, cs = (threadIdx.x & 15) * 4, b = b0 + tr, bc = min(b, a.B - 1);
    const float* part = a.fc1p + ((int64_t)z * a.S * a.B + bc) * HID;
    const float* b1 = th + a.b1_off;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      float4 pv[SMAX][4], bv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = (4 * half + i) * 64 + cs;
        bv[i] = *reinterpret_cast<const float4*>(b1 + c);
#pragma unroll
        for (int sp = 0; sp < SMAX; ++sp)
          pv[sp][i] = *reinterpret_cast<const float4*>(part + (int64_t)min(sp, a.S - 1) * a.B * HID + c);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = (4 * half + i) * 64 + cs;
        float4 acc = bv[i];
#pragma unroll
        for (int sp = 0; sp < SMAX; ++sp)
          if (sp < a.S) {
            acc.x += pv[sp][i].x;
            acc.y += pv[sp][i].y;
            acc.z += pv[sp][i].z;
            acc.w += pv[sp][i].w;
          }
        float4 v = make_float4(relu(acc.x), relu(acc.y), relu(acc.z), relu(acc.w));
        if (b >= a.B) v = make_float4(0.f, 0.f, 0.f, 0.f);  // rows past the batch: zero, their products never stored
        else if (blockIdx.x == 0) *reinterpret_cast<float4*>(a.h1 + ((int64_t)z * a.B + b) * HID + c) = v;
        *reinterpret_cast<float4*>(&s_h[tr * C51_HS + c]) = v;
      }
    }
  }
  __syncthreads();
  if (c0 + wave * 16 >= a.AN) return;  // wave-uniform, after the only barrier
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int g = 0; g < HID / 16; ++g) {
    const float4 av = *reinterpret_cast<const float4*>(&s_h[r * C51_HS + 16 * g + 4 * q]);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, wv[4 * g + 0], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, wv[4 * g + 1], acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, wv[4 * g + 2], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, wv[4 * g + 3], acc1, 0, 0, 0);
  }
  if (col < a.AN) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // D[row 4 q + i][col r]
      const int b = b0 + 4 * q + i;
      if (b < a.B) a.logits[((int64_t)z * a.B + b) * a.AN + col] = (acc0[i] + acc1[i]) + bias;
    }
  }
}

// What a wide head's step does beyond rlax's plain rule (a head kernel's template argument, bits): the plain
// instantiation is the kernel as it was.
constexpr int WIDE_DOUBLE = 1;    // a* = argmax_a q_values of copy 2, online(s_t), instead of the target's own
constexpr int WIDE_WEIGHTED = 2;  // loss = mean_b(w_b loss_b): the cotangent times w_b; the priority clip(|loss_b|, 0, 100)
constexpr int WIDE_NO_DZ1 = 4;   // dz1 is not dl W2^T (the noisy dueling network, rainbow.hpp): W2 is not read, dz1 not written
constexpr float WIDE_MAX_PRIORITY = 100.f;  // rainbow/agent.py:198

struct C51HeadArgs {
  const float* logits;   // [Z][B][A N]
  const float* h1;       // [Z][B][512]; copy 0's ReLU decisions gate dz1
  const float* w2;       // online fc2 weights [512][A N]
  const float* support;  // [N], strictly increasing
  int Z, B, A, N, fwd_only;
  const float4* rec;  // batch records {a, r, d, 0} written by conv1 (learn mode)
  float* qv;          // [Z][B][A] q_values
  float* la;          // [B][N] online logits of the taken action
  float* dl;          // [B][N] d loss / d those logits
  int32_t* astar;     // [B] argmax_a q_target (WIDE_DOUBLE: of copy 2's q_values)
  float* loss_part;   // [B] what the update sums to the step's loss: loss_b (WIDE_WEIGHTED: w_b loss_b)
  float* gq;          // [B] <- 0 (the scalar head's cotangent: unused downstream, never stale)
  int32_t* ga;        // [B] <- a_b
  float* dz1;         // [B][512]
  // actor mode (fwd_only): eps-greedy draw per sample into act_out (or null)
  dqz_action* act_out;
  double eps;
  uint64_t act_seed, act_ctr;
  // WIDE_WEIGHTED alone (last, so that the plain kernels read their arguments where they always did)
  const float* weights;  // [B] importance weights
  float* loss_b;         // [B] the unweighted per-sample loss
  float* prio;           // [B] clip(|loss_b|, 0, 100): the learner's td buffer, which dqz_per_write_back reads
};

// Maximum of a wave's floats in every lane (exact in any order).
__device__ __forceinline__ float wave_max(float m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  return m;
}

// One workgroup (512 threads) per sample b.  A distribution is one wave's
// business (lane = atom, N <= 64): wave w takes rows w, w + 8, ... of the
// Z A (copy, action) rows, with wave_sum's fixed order, so equal inputs give
// equal bits.  The record is read by every thread through the same (uniform)
// address, and the W2 operands of dz1 (the taken action's N columns of every
// row) are requested as soon as the action is known, under everything else
// the workgroup does.  With WIDE_DOUBLE copy 2's logits never enter LDS: the
// wave that owns a row of it reads the row from global memory and leaves the
// action's q_value alone.  MODE = 0 compiles to the instructions the kernel had
// before it took a mode (a shared __device__ body behind thin kernels does not:
// the register allocation moves).
template <int MODE>
DQZ_OTHER_KERNEL __launch_bounds__(512) void c51_head_kernel(C51HeadArgs h) {
  constexpr bool DQ = MODE & WIDE_DOUBLE, WT = MODE & WIDE_WEIGHTED, DZ = !(MODE & WIDE_NO_DZ1);
  __shared__ float s_lg[2][C51_MAXOUT];
  __shared__ float s_z[C51_MAXN], s_p[C51_MAXN];
  __shared__ float s_dlp[3 + 16 * ((C51_MAXN + 3 + 15) / 16) + 1];  // dlogits at [3, 3 + N), zeros around them
  __shared__ float s_part[8][C51_MAXN];
  __shared__ float s_q[2][MAXA], s_mx[2][MAXA], s_se[2][MAXA];
  __shared__ float s_qs[DQ ? MAXA : 1];  // the selector's q_values (copy 2)
  const int b = blockIdx.x, n = threadIdx.x, lane = n & 63, wave = n >> 6;
  const int A = h.A, N = h.N, AN = A * N, B = h.B, Z = h.Z;
  const int ZL = DQ ? 2 : Z;  // copies held in LDS
  int a_tm1 = 0;
  float r = 0.f, d = 0.f, wt = 1.f;
  // dz1's operands: four lanes share a row of W2 (rows 128 p + n / 4, p = 0 .. 3), each loading the aligned
  // float4s sub + 4 j of the 16-byte window that holds the row's N weights of the taken action, which starts
  // `off` floats into it.  A thread per row would touch 64 cache lines per load instruction (rows are A N
  // floats apart) and took 15 us; see DESIGN section 4.  The window may run a few floats past the row (the next
  // row, or past the last row the fc2 bias leaf, 64 floats at least): those meet zeros of s_dlp.
  constexpr int DZ_P = HID / 128, DZ_J = (C51_MAXN + 3 + 15) / 16;  // 4 passes, at most 5 float4 per lane
  const int sub = n & 3, nj = (N + 3 + 15) / 16;
  float4 wq[DZ_P][DZ_J];
  float hv[DZ_P];
  int off[DZ_P];
  if (!h.fwd_only) {
    const float4 rv = h.rec[b];
    a_tm1 = min(max(__float_as_int(rv.x), 0), A - 1);  // a record outside [0, A) reads inside the buffers
    r = rv.y;
    d = rv.z;
    if (WT) wt = h.weights[b];
#pragma unroll
    for (int p = 0; DZ && p < DZ_P; ++p) {
      const int row = 128 * p + (n >> 2);
      const int64_t base = (int64_t)row * AN + a_tm1 * N;
      off[p] = (int)(base & 3);
      const float4* w4 = reinterpret_cast<const float4*>(h.w2 + (base - off[p]));
#pragma unroll
      for (int j = 0; j < DZ_J; ++j) wq[p][j] = w4[sub + 4 * min(j, nj - 1)];
      hv[p] = h.h1[(int64_t)b * HID + row];
    }
  }
  for (int e = n; e < ZL * AN; e += HID) {
    const int z = e / AN, c = e % AN;
    s_lg[z][c] = h.logits[((int64_t)z * B + b) * AN + c];
  }
  if (n < N) s_z[n] = h.support[n];
  if (n < (int)(sizeof(s_dlp) / sizeof(float))) s_dlp[n] = 0.f;
  __syncthreads();
  // softmax statistics and q_values[z][a] = sum_j softmax_j z_j
  for (int row = wave; row < Z * A; row += 8) {
    const int z = row / A, a = row % A;
    float x = -INFINITY;
    if (DQ && z == 2) {  // wave-uniform
      if (lane < N) x = h.logits[((int64_t)2 * B + b) * AN + a * N + lane];
    } else if (lane < N) {
      x = s_lg[z][a * N + lane];
    }
    const float mx = wave_max(x);
    const float e = lane < N ? expf(x - mx) : 0.f;
    const float se = wave_sum(e);
    const float qa = wave_sum(lane < N ? (e / se) * s_z[lane] : 0.f);
    if (lane == 0) {
      if (DQ && z == 2) {
        s_qs[a] = qa;
      } else {
        s_mx[z][a] = mx;
        s_se[z][a] = se;
        s_q[z][a] = qa;
      }
      h.qv[((int64_t)z * B + b) * A + a] = qa;
    }
  }
  __syncthreads();
  if (h.fwd_only) {
    if (h.act_out && n == 0) {  // eps-greedy draw b of call act_ctr (head_body's stream)
      const uint4 rr = philox4x32(make_uint4((unsigned)h.act_ctr, (unsigned)(h.act_ctr >> 32), (unsigned)b, 0xAC7u),
                                  make_uint2((unsigned)h.act_seed, (unsigned)(h.act_seed >> 32)));
      const double u = ((((uint64_t)rr.x << 32) | rr.y) >> 11) * 0x1.0p-53;
      h.act_out[b] = eps_greedy(s_q[0], A, h.eps, u);
    }
    return;
  }
  int am = 0;  // jnp.argmax: first maximum; every thread forms it from the same LDS values
  {
    const float* sel = DQ ? s_qs : s_q[1];
    float best = sel[0];
    for (int a = 1; a < A; ++a)
      if (sel[a] > best) {
        best = sel[a];
        am = a;
      }
  }
  if (n < N) s_p[n] = expf(s_lg[1][am * N + n] - s_mx[1][am]) / s_se[1][am];
  __syncthreads();
  {
    // m_k = sum_i clip(1 - dhat_{k,i}, 0, 1) p_i (categorical_l2_project): thread (k = lane, wave) sums the
    // terms i = wave, wave + 8, ... in order; the eight partials are added in wave order below.  The reciprocal
    // spacings of atom k are 0 where the roll-around makes the spacing non-positive (the outward side of an end atom).
    const int k = min(lane, N - 1);
    const float zk = s_z[k], z0 = s_z[0], zl = s_z[N - 1];
    const float sp = s_z[k + 1 < N ? k + 1 : 0] - zk, sn = zk - s_z[k > 0 ? k - 1 : N - 1];
    const float dpos = sp > 0.f ? 1.f / sp : 0.f, dneg = sn > 0.f ? 1.f / sn : 0.f;
    float m = 0.f;
    for (int i = wave; i < N; i += 8) {
      const float y = fminf(fmaxf(__fmaf_rn(d, s_z[i], r), z0), zl);
      const float dq = y - zk;
      const float dh = dq >= 0.f ? dq * dpos : -dq * dneg;
      m += fminf(fmaxf(1.f - dh, 0.f), 1.f) * s_p[i];
    }
    s_part[wave][lane] = m;
  }
  __syncthreads();
  if (wave == 0) {
    const int k = min(lane, N - 1);
    float m = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) m += s_part[w][lane];
    const float l = s_lg[0][a_tm1 * N + k], xs = l - s_mx[0][a_tm1], se = s_se[0][a_tm1];
    float g = (expf(xs) / se - m) / (float)B;
    if (WT) g = wt == 0.f ? 0.f : g * wt;  // a weight of 0: +0.0, whatever g's sign
    const float ce = wave_sum(lane < N ? m * (xs - logf(se)) : 0.f);
    if (lane < N) {
      s_dlp[3 + lane] = g;
      h.la[(int64_t)b * N + lane] = l;
      h.dl[(int64_t)b * N + lane] = g;
    }
    if (lane == 0) {
      if (WT) {
        h.loss_part[b] = wt * -ce;
        h.loss_b[b] = -ce;
        h.prio[b] = fminf(fabsf(ce), WIDE_MAX_PRIORITY);
      } else {
        h.loss_part[b] = -ce;
      }
      h.gq[b] = 0.f;
      h.ga[b] = a_tm1;
      h.astar[b] = am;
    }
  }
  __syncthreads();
  // dz1[b][row] = relu'(z1) sum_k dlogits[k] W2[row][a_b N + k]: window float f pairs with dlogits[f - off]
#pragma unroll
  for (int p = 0; DZ && p < DZ_P; ++p) {
    float dz = 0.f;
#pragma unroll
    for (int j = 0; j < DZ_J; ++j)
      if (j < nj) {
        const float* dq = &s_dlp[3 - off[p] + 4 * (sub + 4 * j)];
        dz = __fmaf_rn(dq[0], wq[p][j].x, dz);
        dz = __fmaf_rn(dq[1], wq[p][j].y, dz);
        dz = __fmaf_rn(dq[2], wq[p][j].z, dz);
        dz = __fmaf_rn(dq[3], wq[p][j].w, dz);
      }
    dz += dpp_f<0xB1>(dz);  // the row's four lanes: quad xor 1, xor 2
    dz += dpp_f<0x4E>(dz);
    if (sub == 0) h.dz1[(int64_t)b * HID + 128 * p + (n >> 2)] = hv[p] > 0.f ? dz : 0.f;
  }
}

struct C51GradArgs {
  const float* h1;    // [B][512] online copy
  const float* dl;    // [B][N]
  const int32_t* ga;  // [B]
  int B, A, N;
  float* gw;  // fc2/w gradient [512][A N]
  float* gb;  // fc2/b gradient [A N]
  int acc;    // 1: add into gw / gb
};

// One thread per element of dW2 (rows j < 512) and db2 (row j = 512):
//   dW2[j][a N + k] = sum_{b: a_b = a} h1[b][j] dlogits[b][k],  db2[a N + k] = sum_{b: a_b = a} dlogits[b][k]
// in sample order.  Sixteen samples' operands are loaded (unconditional, clamped
// to the last sample) before any is summed, so they are in flight together.
DQZ_OTHER_KERNEL __launch_bounds__(256) void c51_fc2_grad_kernel(C51GradArgs u) {
  const int AN = u.A * u.N;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)(HID + 1) * AN) return;
  const int j = (int)(e / AN), c = (int)(e % AN), a = c / u.N, k = c % u.N;
  float g = 0.f;
  constexpr int R = 16;
  for (int b0 = 0; b0 < u.B; b0 += R) {
    float hv[R], dv[R];
    int32_t av[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int b = min(b0 + i, u.B - 1);
      av[i] = u.ga[b];
      hv[i] = j < HID ? u.h1[(int64_t)b * HID + j] : 1.f;
      dv[i] = u.dl[(int64_t)b * u.N + k];
    }
#pragma unroll
    for (int i = 0; i < R; ++i)
      if (b0 + i < u.B && av[i] == a) g = __fmaf_rn(hv[i], dv[i], g);
  }
  float* dst = j < HID ? u.gw + (int64_t)j * AN + c : u.gb + c;
  *dst = u.acc ? *dst + g : g;
}

}  // namespace dqz
