// qr.hpp — the quantile (QR-DQN) head: rlax.quantile_q_learning per sample
// on outputs N * A wide, and the two batched products behind it
// (qrdqn/agent.py:36-39,88-110; networks.py:295-313; rlax 0.1.2
// quantile_regression_loss / quantile_q_learning).  The outputs of both copies
// are c51_logits_kernel's (c51.hpp: generic in the output width).  These
// kernels live in the other code object (learner.hip) and talk to the learner
// step through launch boundaries only: no hand-off words, no spin-waits.
//
// The layout is quantile-major: q_dist[b, i, a] = out[b, i A + a], so the
// taken action's N columns of a W2 row are A floats apart.  Nothing here walks
// them per sample: the head writes the dense cotangent dout [B][A N] (zeros
// but for column i A + a_b) and dz1 is a batched product over it.
//
//   qr_head_kernel     one workgroup per sample: both copies' outputs into
//                      LDS, q_values[z][a] = mean_i x[z][i][a], a* = argmax_a
//                      q_target, theta_i = x_o[i][a_b], t_j = r + d x_t[j][a*],
//                      the N x N quantile-Huber sum (thread (i, s) walks the
//                      s-th quarter of j in order), dtheta, the loss and dout.
//                      Forward / actor mode stops after q_values (and the
//                      eps-greedy draw).  WIDE_DOUBLE (c51.hpp): a* comes from
//                      a third copy, online(s_t) (rlax.quantile_q_learning
//                      with dist_q_t_selector = online(s_t)); WIDE_WEIGHTED:
//                      dtheta carries the sample's importance weight and
//                      clip(|loss_b|, 0, 100) is its new priority.  The
//                      reference has no prioritized QR-DQN: the quantile
//                      priority is this project's definition, Rainbow's rule
//                      (rainbow/agent.py:198) on the quantile loss.
//   qr_dz1_kernel      dz1[16 samples][16 rows] = dout[16][A N] W2^T[A N][16]
//                      on v_mfma_f32_16x16x4_f32, K dealt to the workgroup's
//                      eight waves and added in wave order, then copy 0's ReLU
//                      mask: W2 is read once per 16 samples.
//   qr_fc2_grad_kernel dW2 = h1^T dout and db2 = 1^T dout on the same MFMA with
//                      K = B, every element written (zeros for actions absent
//                      from the batch), summed in sample order.
#pragma once
#include "common.hpp"
#include "c51.hpp"   // WIDE_DOUBLE, WIDE_WEIGHTED, WIDE_MAX_PRIORITY
#include "head.hpp"  // eps_greedy

namespace dqz {

constexpr int QR_MAXN = 256;      // quantiles per action: thread i of a quarter owns quantile i
constexpr int QR_MAXOUT = 4096;   // A * N: both copies' outputs of a sample fit 32 KB of LDS
constexpr int QR_JS = 4;          // j ranges per quantile in the pairwise sum (head at A = 6: 11.2 us with 1, 8.8 with 2, 8.2 with 4)
constexpr int QR_THREADS = QR_MAXN * QR_JS;      // 1024
constexpr int QR_LOADS = 2 * QR_MAXOUT / QR_THREADS;  // 8 outputs per thread
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct QrHeadArgs {
  const float* out;  // [Z][B][A N], quantile-major
  const float* tau;  // [N], each strictly inside (0, 1)
  float kappa;       // huber_param > 0
  int Z, B, A, N, fwd_only;
  const float4* rec;  // batch records {a, r, d, 0} written by conv1 (learn mode)
  float* qv;          // [Z][B][A] q_values
  float* theta;       // [B][N] online outputs of the taken action
  float* dtheta;      // [B][N] d loss / d those outputs
  float* dout;        // [B][A N] the dense cotangent: dtheta at column i A + a_b, zeros elsewhere
  int32_t* astar;     // [B] argmax_a q_target (WIDE_DOUBLE: of copy 2's q_values)
  float* loss_part;   // [B] what the update sums to the step's loss: loss_b (WIDE_WEIGHTED: w_b loss_b)
  float* gq;          // [B] <- 0 (the scalar head's cotangent: unused downstream, never stale)
  int32_t* ga;        // [B] <- a_b
  // actor mode (fwd_only): eps-greedy draw per sample into act_out (or null)
  dqz_action* act_out;
  double eps;
  uint64_t act_seed, act_ctr;
  // WIDE_WEIGHTED alone (last, so that the plain kernels read their arguments where they always did)
  const float* weights;  // [B] importance weights
  float* loss_b;         // [B] the unweighted per-sample loss
  float* prio;           // [B] clip(|loss_b|, 0, 100): the learner's td buffer, which dqz_per_write_back reads
};

// One workgroup (1024 threads) per sample b.  Every global load (the record,
// the thread's quantile, its eight outputs) is issued before the first is
// used.  Thread n = 256 s + i owns quantile i and the s-th of four j ranges
// (2 ceil(N / 8) long): it walks it in order, the four partial sums of a
// quantile are added in s order, the loss rows in i order, so equal inputs give
// equal bits.  The target t_j is a broadcast LDS read.  The N^2 pairs are the
// launch's arithmetic: about six instructions a pair on one CU's four SIMDs.
// With WIDE_DOUBLE copy 2's outputs never enter LDS (the two copies there fill
// its 32 KB): the wave that owns an action of it sums the action's quantiles
// from global memory, in the order the other copies' are summed.  MODE = 0
// compiles to the instructions the kernel had before it took a mode.
template <int MODE>
DQZ_OTHER_KERNEL __launch_bounds__(QR_THREADS) void qr_head_kernel(QrHeadArgs h) {
  constexpr bool DQ = MODE & WIDE_DOUBLE, WT = MODE & WIDE_WEIGHTED;
  __shared__ float s_x[2 * QR_MAXOUT];  // copy z's outputs at [z A N, (z + 1) A N)
  __shared__ __attribute__((aligned(8))) float s_t[QR_MAXN];
  __shared__ float s_th[QR_MAXN], s_g[QR_MAXN];
  __shared__ float s_lp[QR_JS][QR_MAXN], s_gp[QR_JS][QR_MAXN];
  __shared__ float s_q[DQ ? 3 : 2][MAXA];
  const int b = blockIdx.x, n = threadIdx.x, lane = n & 63, wave = n >> 6;
  const int A = h.A, N = h.N, AN = A * N, B = h.B, Z = h.Z, tot = (DQ ? 2 : Z) * AN;  // tot: the copies held in LDS
  const int qi = n & (QR_MAXN - 1), qic = min(qi, N - 1);
  const int qs = __builtin_amdgcn_readfirstlane(n / QR_MAXN);  // a wave lies inside one j range: scalar loop bounds
  int a_tm1 = 0;
  float r = 0.f, d = 0.f, tau = 0.5f, wt = 1.f;
  if (!h.fwd_only) {
    const float4 rv = h.rec[b];
    a_tm1 = min(max(__float_as_int(rv.x), 0), A - 1);  // a record outside [0, A) reads inside the buffers
    r = rv.y;
    d = rv.z;
    tau = h.tau[qic];
    if (WT) wt = h.weights[b];
  }
  {
    float v[QR_LOADS];
#pragma unroll
    for (int k = 0; k < QR_LOADS; ++k) {
      const int e = min(n + QR_THREADS * k, tot - 1), z = e >= AN, c = e - z * AN;
      v[k] = h.out[((int64_t)z * B + b) * AN + c];
    }
#pragma unroll
    for (int k = 0; k < QR_LOADS; ++k)
      if (n + QR_THREADS * k < tot) s_x[n + QR_THREADS * k] = v[k];
  }
  __syncthreads();
  // q_values[z][a] = mean_i x[z][i][a]: a wave per (copy, action), lane l sums i = l, l + 64, ... in order
  for (int row = wave; row < Z * A; row += QR_THREADS / 64) {
    const int z = row / A, a = row % A;
    float acc = 0.f;
    if (DQ && z == 2) {  // wave-uniform
      const float* x2 = h.out + ((int64_t)2 * B + b) * AN + a;
      for (int i = lane; i < N; i += 64) acc += x2[i * A];
    } else {
      for (int i = lane; i < N; i += 64) acc += s_x[z * AN + i * A + a];
    }
    const float q = wave_sum(acc) / (float)N;
    if (lane == 0) {
      s_q[z][a] = q;
      h.qv[((int64_t)z * B + b) * A + a] = q;
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
    const float* sel = s_q[DQ ? 2 : 1];
    float best = sel[0];
    for (int a = 1; a < A; ++a)
      if (sel[a] > best) {
        best = sel[a];
        am = a;
      }
  }
  if (n < N) {
    s_th[n] = s_x[n * A + a_tm1];
    s_t[n] = __fmaf_rn(d, s_x[AN + n * A + am], r);
  }
  __syncthreads();
  {
    // row i of delta_ij = t_j - theta_i, two j at a time on the packed f32 pipe: c = clip(delta, -k, k) is the
    // slope of H_k and H_k(delta) = c (delta - c / 2) (c has delta's sign and |c| = min(|delta|, k));
    // w_ij = |tau_i - 1[delta < 0]|.  The even and the odd j of the range accumulate apart and are added at the
    // end, then an odd range's last j.
    const float k = h.kappa, th = s_th[qic], w0 = tau, w1 = fabsf(tau - 1.f);
    const int jn = 2 * ((N + 2 * QR_JS - 1) / (2 * QR_JS)), j0 = min(qs * jn, N), j1 = min(N, j0 + jn);
    f32x2 ls2 = {0.f, 0.f}, gs2 = {0.f, 0.f};
    int j = j0;
#pragma unroll 4
    for (; j + 1 < j1; j += 2) {
      const f32x2 t2 = {s_t[j], s_t[j + 1]};
      const f32x2 delta = t2 - th;
      const f32x2 c = {__builtin_amdgcn_fmed3f(delta.x, -k, k), __builtin_amdgcn_fmed3f(delta.y, -k, k)};
      const f32x2 w = {delta.x < 0.f ? w1 : w0, delta.y < 0.f ? w1 : w0};
      ls2 += w * (c * (delta - 0.5f * c));
      gs2 += w * c;
    }
    float ls = ls2.x + ls2.y, gs = gs2.x + gs2.y;
    if (j < j1) {
      const float delta = s_t[j] - th, c = __builtin_amdgcn_fmed3f(delta, -k, k), w = delta < 0.f ? w1 : w0;
      ls += w * (c * (delta - 0.5f * c));
      gs += w * c;
    }
    s_lp[qs][qi] = ls;
    s_gp[qs][qi] = gs;
  }
  __syncthreads();
  if (n < N) {
    float ls = s_lp[0][n], gs = s_gp[0][n];
#pragma unroll
    for (int s = 1; s < QR_JS; ++s) {
      ls += s_lp[s][n];
      gs += s_gp[s][n];
    }
    float g = -(gs / (float)(N * B));
    if (WT) g = wt == 0.f ? 0.f : g * wt;  // a weight of 0: +0.0, whatever g's sign
    s_g[n] = g;
    s_lp[0][n] = ls / (float)N;  // the row's mean over j; this thread alone reads and writes column n
    h.theta[(int64_t)b * N + n] = s_th[n];
    h.dtheta[(int64_t)b * N + n] = g;
  }
  __syncthreads();
  for (int c = n; c < AN; c += QR_THREADS) {
    const int i = c / A, a = c - i * A;
    h.dout[(int64_t)b * AN + c] = a == a_tm1 ? s_g[i] : 0.f;
  }
  if (n == 0) {
    float loss = 0.f;
    for (int i = 0; i < N; ++i) loss += s_lp[0][i];
    if (WT) {
      h.loss_part[b] = wt * loss;
      h.loss_b[b] = loss;
      h.prio[b] = fminf(fabsf(loss), WIDE_MAX_PRIORITY);
    } else {
      h.loss_part[b] = loss;
    }
    h.gq[b] = 0.f;
    h.ga[b] = a_tm1;
    h.astar[b] = am;
  }
}

constexpr int QR_DZ_ROWS = 16;   // W2 rows per workgroup (the MFMA's N)
constexpr int QR_DZ_WAVES = 8;   // K is dealt to the workgroup's waves in groups of 16
constexpr int QR_DZ_PG = 10;     // K groups of a wave whose operands are in flight together
constexpr int QR_PAD = 16;       // floats readable behind dout [B][A N]: the last K group's 16-byte loads run past A N

// A 16-byte global load from a 4-byte-aligned address (rows are A N floats apart, any A N).
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

struct QrDz1Args {
  const float* dout;  // [B][A N] (+ QR_PAD readable floats)
  const float* w2;    // online fc2 weights [512][A N]; the fc2 bias leaf follows them
  const float* h1;    // [B][512] online copy: its ReLU decisions gate dz1
  int B, AN;
  float* dz1;  // [B][512]
};

// dz1[b][row] = relu'(h1[b][row]) sum_c dout[b][c] W2[row][c].  Grid (512 / 16,
// ceil(B / 16)), 512 threads.  K = A N runs in groups of 16 dealt round-robin to
// the eight waves (wave w: groups w, w + 8, ...): lane (r = lane & 15, q =
// lane >> 4) reads dout[b0 + r][16 g + 4 q ..+ 3] and W2[row0 + r][the same] as
// one 16-byte load each and feeds them to four MFMAs (the MFMA sums over q).
// Ten groups' twenty loads are issued before the first MFMA of a pass (A = 6:
// one pass, A = 18: three).  Two accumulators alternate and are added at the
// end; the eight waves' partials meet in LDS and are added in wave order: a
// fixed order, equal bits each run.  A group past the wave's last repeats it
// and a column past A N reads on into the next row (behind the last row: the
// fc2 bias leaf, QR_PAD): both meet zeros in the dout operand.  Rows past the
// batch repeat the last sample and are never stored.
DQZ_OTHER_KERNEL __launch_bounds__(64 * QR_DZ_WAVES) void qr_dz1_kernel(QrDz1Args a) {
  __shared__ float s_p[QR_DZ_WAVES][16][QR_DZ_ROWS + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
  const int row0 = blockIdx.x * QR_DZ_ROWS, b0 = blockIdx.y * 16, AN = a.AN;
  const int fb = b0 + (threadIdx.x >> 4), fr = row0 + (threadIdx.x & 15);  // the element threads 0 .. 255 finish
  float hv = 0.f;
  if (threadIdx.x < 256) hv = a.h1[(int64_t)min(fb, a.B - 1) * HID + fr];
  const int G = (AN + 15) / 16;
  const float* wrow = a.w2 + (int64_t)(row0 + r) * AN + 4 * q;
  const float* drow = a.dout + (int64_t)min(b0 + r, a.B - 1) * AN + 4 * q;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  for (int g0 = wave; g0 < G; g0 += QR_DZ_WAVES * QR_DZ_PG) {  // wave-uniform: every MFMA runs with the whole wave
    f32x4 wv[QR_DZ_PG], dv[QR_DZ_PG];
#pragma unroll
    for (int p = 0; p < QR_DZ_PG; ++p) {
      const int c = 16 * min(g0 + QR_DZ_WAVES * p, G - 1);
      wv[p] = *reinterpret_cast<const f32x4u*>(wrow + c);
      dv[p] = *reinterpret_cast<const f32x4u*>(drow + c);
    }
    // without this the scheduler sinks each pair of loads to its MFMAs (a round trip per group)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int p = 0; p < QR_DZ_PG; ++p) {
      const int g = g0 + QR_DZ_WAVES * p, left = g < G ? AN - (16 * g + 4 * q) : 0;  // columns of this lane's four inside A N
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i >= left) dv[p][i] = 0.f;
    }
#pragma unroll
    for (int p = 0; p < QR_DZ_PG; ++p) {
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[p][0], wv[p][0], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[p][1], wv[p][1], acc1, 0, 0, 0);
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[p][2], wv[p][2], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[p][3], wv[p][3], acc1, 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) s_p[wave][4 * q + i][r] = acc0[i] + acc1[i];  // D[sample 4 q + i][row r]
  __syncthreads();
  if (threadIdx.x < 256 && fb < a.B) {
    const int sm = threadIdx.x >> 4, rr = threadIdx.x & 15;
    float dz = s_p[0][sm][rr];
#pragma unroll
    for (int w = 1; w < QR_DZ_WAVES; ++w) dz += s_p[w][sm][rr];
    a.dz1[(int64_t)fb * HID + fr] = hv > 0.f ? dz : 0.f;
  }
}

constexpr int QR_FG_TILES = 4;  // 16-column tiles per wave of the fc2 gradient
constexpr int QR_FG_KS = 8;     // MFMA steps per pass over the batch: 32 samples

struct QrGradArgs {
  const float* h1;    // [B][512] online copy
  const float* dout;  // [B][A N]: zeros in the columns of every action but the sample's own
  int B, AN;
  float* gw;  // fc2/w gradient [512][A N]
  float* gb;  // fc2/b gradient [A N]
  int acc;    // 1: add into gw / gb
};

// dW2[j][c] = sum_b h1[b][j] dout[b][c] (row blocks 0 .. 31) and db2[c] = sum_b
// dout[b][c] (row block 32: a row of ones) on v_mfma_f32_16x16x4_f32 with K = B:
// grid (33, ceil(A N / 256)), 256 threads; a wave owns sixteen rows j and four
// 16-column tiles.  Lane (r, q) feeds h1[4 s + q][j0 + r] and dout[4 s + q][c0 +
// r] to step s, so an output is an fma chain over the samples in order, four at
// a time, in one accumulator: equal bits each run.  The 8 + 32 operands of 32
// samples are loaded before the first MFMA.  Every element is written; a column
// whose dout is all zeros (an action absent from the batch) sums to +0.0.
// Samples past the batch feed zeros, columns past A N are never stored.
DQZ_OTHER_KERNEL __launch_bounds__(256) void qr_fc2_grad_kernel(QrGradArgs u) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, q = lane >> 4;
  const int AN = u.AN, j0 = blockIdx.x * 16, bias = j0 >= HID;
  const int c0 = (blockIdx.y * 4 + wave) * 16 * QR_FG_TILES;
  if (c0 >= AN) return;  // wave-uniform; no barrier below
  f32x4 acc[QR_FG_TILES];
#pragma unroll
  for (int t = 0; t < QR_FG_TILES; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < u.B; k0 += 4 * QR_FG_KS) {
    float hv[QR_FG_KS], dv[QR_FG_TILES][QR_FG_KS];
#pragma unroll
    for (int s = 0; s < QR_FG_KS; ++s) {
      const int b = k0 + 4 * s + q, bc = min(b, u.B - 1);
      hv[s] = bias ? 0.f : u.h1[(int64_t)bc * HID + j0 + r];
#pragma unroll
      for (int t = 0; t < QR_FG_TILES; ++t) dv[t][s] = u.dout[(int64_t)bc * AN + min(c0 + 16 * t + r, AN - 1)];
    }
#pragma unroll
    for (int s = 0; s < QR_FG_KS; ++s) {
      const bool in = k0 + 4 * s + q < u.B;
      if (bias) hv[s] = r == 0 ? 1.f : 0.f;
      if (!in) hv[s] = 0.f;
#pragma unroll
      for (int t = 0; t < QR_FG_TILES; ++t)
        if (!in) dv[t][s] = 0.f;
    }
#pragma unroll
    for (int s = 0; s < QR_FG_KS; ++s)
#pragma unroll
      for (int t = 0; t < QR_FG_TILES; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(hv[s], dv[t][s], acc[t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < QR_FG_TILES; ++t) {
    const int c = c0 + 16 * t + r;
    if (c >= AN) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {  // D[row 4 q + i][col r]
      const int j = j0 + 4 * q + i;
      if (j > HID) continue;
      float* dst = j < HID ? u.gw + (int64_t)j * AN + c : u.gb + c;
      *dst = u.acc ? *dst + acc[t][i] : acc[t][i];
    }
  }
}

}  // namespace dqz
