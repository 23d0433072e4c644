// learner_step.hip — the MI355X-native DQN learner step behind the dqz C ABI,
// in a code object of its own (common.hpp, "Two translation units").
//
// One step (dqn/agent.py:109-119, prioritized/agent.py:115-127), in launch order:
//   0 conv1 -> conv2 -> conv3 fwd as one hand-off launch (fwd_conv_kernel;
//     frame gather fused; z = online(s_tm1), target(s_t) [, online(s_t) for
//     double-Q])                                                  conv1.hpp, fwd.hpp
//   3 fc1 fwd (split-K)                                           fwd.hpp
//   4 head: fc1 reduce + fc2 + TD loss + dq + dz1, per sample    head.hpp
//   5 fc1 dX -> dy3 (+ the dX-ordered W3 / W2 copies)            bwd.hpp
//   6 the rest of the backward in one launch (bwd_bc_kernel): conv3 dX ->
//     conv2 dX -> conv1 dW hand-offs, fc1 dW + fused RMSProp, conv3 / conv2
//     dW partials                                                 bwd.hpp
//   7 reduce of every cross-sample / split-K gradient + centered RMSProp
// With StepRequest::wide the launches of the categorical or the quantile head
// (c51.hpp, qr.hpp, the other code object; wide_launch) stand in for 4, and the
// fc2 gradient follows 7 in one of its own.  The Rainbow network (rainbow.hpp)
// also stands in for 5: its dy3 is the sum of four fc1 dX products, which it
// launches through fc1_dx below, as it launches its other three fc1 forwards
// through fc1_forward.
// What a step is asked to do (batch source, gradient mode, PER write-back,
// MGSC meta mode, a wide head, profiling) is a StepRequest
// (learner_impl.hpp), whose fields carry the modes' documentation; the
// hand-off words are named in layout.hpp.
#define DQZ_STEP_TU 1
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "learner_impl.hpp"

using namespace dqz;

static int g_attr_done = 0;

static int init_kernel_attrs() {
  if (g_attr_done) return DQZ_OK;
  const void* fwd_kernels[] = {(const void*)fwd_conv_kernel<0>, (const void*)fwd_conv_kernel<1>,
                               (const void*)fwd_conv_kernel<2>, (const void*)fwd_conv_kernel<3>,
                               (const void*)fwd_conv_kernel<4>};
  for (const void* k : fwd_kernels)
    DQZ_HIP(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kConv1FwdSmem));
  g_attr_done = 1;
  return DQZ_OK;
}

extern "C" {

int dqz_param_layout(int num_actions, int shared_bias, int64_t offsets[10], int64_t sizes[10], int64_t* total) {
  if (num_actions < 1 || num_actions > MAXA) return fail(DQZ_ERR_INVALID, "num_actions must be in [1, %d]", MAXA);
  if (!offsets || !sizes || !total) return fail(DQZ_ERR_INVALID, "null output pointer");
  param_layout(num_actions, shared_bias, offsets, sizes, total);
  return DQZ_OK;
}

int dqz_learner_create(const dqz_learner_config* cfg, dqz_learner** out) {
  if (!cfg || !out) return fail(DQZ_ERR_INVALID, "null argument");
  if (cfg->batch < 1 || cfg->batch > MAXB) return fail(DQZ_ERR_INVALID, "batch must be in [1, %d]", MAXB);
  if (cfg->num_actions < 1 || cfg->num_actions > MAXA)
    return fail(DQZ_ERR_INVALID, "num_actions must be in [1, %d]", MAXA);
  if (cfg->algo < DQZ_ALGO_DQN || cfg->algo > DQZ_ALGO_PER) return fail(DQZ_ERR_INVALID, "unknown algo %d", cfg->algo);
  if (int rc = init_kernel_attrs()) return rc;
  dqz_learner* L = new dqz_learner();
  L->cfg = *cfg;
  L->Z = cfg->algo == DQZ_ALGO_DQN ? 2 : 3;
  L->shared_bias = cfg->algo == DQZ_ALGO_DQN ? 0 : 1;
  param_layout(cfg->num_actions, L->shared_bias, L->off, L->sz, &L->total);
  const int64_t B = cfg->batch, Z = L->Z, A = cfg->num_actions;
  L->S_fc1 = FC1_S;
  L->S2 = L->S3 = cfg->batch;  // per-sample conv2 / conv3 dW partials (bwd_bc_kernel)
  // the scratch buffers in allocation order, sizes in floats (layout.hpp carve)
  const Carve bufs[] = {
      {&L->y1, Z * B * C1M * C1CO}, {&L->y2, Z * B * C2M * C2CO}, {&L->y3, Z * B * FLAT},
      {&L->fc1p, Z * L->S_fc1 * B * HID}, {&L->h1, Z * B * HID}, {&L->q, Z * B * A},
      {&L->dz1, B * HID}, {&L->dy3, B * FLAT}, {&L->dy2, B * C2M * C2CO}, {&L->dy1, B * C1M * C1CO},
      {&L->p1, B * C1_BLOCKS * (C1KK + 1) * C1CO}, {&L->p2, B * (C2KK + 1) * C2CO}, {&L->p3, B * (C3KK + 1) * C3CO},
      {&L->td, B}, {&L->loss, 1}, {&L->loss_part, B}, {&L->gq, B}, {&L->ga, B}, {&L->rec, 4 * B},
      {&L->sync, SyncLayout{B}.ints()}, {&L->w3p, W3P_N}, {&L->w2p, W2P_N}, {&L->per_wb, 2 * B}};
  const int64_t total = carve(bufs, nullptr);
  if (hipMalloc(&L->block, total * sizeof(float)) != hipSuccess) {
    delete L;
    return fail(DQZ_ERR_HIP, "hipMalloc of %lld bytes failed", (long long)(total * 4));
  }
  if (hipMemset(L->block, 0, total * sizeof(float)) != hipSuccess) {
    (void)hipFree(L->block);
    delete L;
    return fail(DQZ_ERR_HIP, "hipMemset of learner scratch failed");
  }
  carve(bufs, (float*)L->block);
  *out = L;
  return DQZ_OK;
}

int dqz_learner_destroy(dqz_learner* L) {
  if (!L) return DQZ_OK;
  if (L->block) (void)hipFree(L->block);
  delete L;
  return DQZ_OK;
}

}  // extern "C"

#define DQZ_PHASE(i, ...)                                                   \
  do {                                                                      \
    if (!pe.on()) {                                                         \
      __VA_ARGS__;                                                          \
    } else {                                                                \
      /* best of three trials: a stalled launching thread lets the queue */ \
      /* drain, and the idle device time would count as the phase's      */ \
      float best_ = 0.f;                                                    \
      for (int t_ = 0; t_ < 3; ++t_) {                                      \
        DQZ_HIP(hipEventRecord(pe.e0, st));                                 \
        for (int r_ = 0; r_ < pe.reps; ++r_) {                              \
          __VA_ARGS__;                                                      \
        }                                                                   \
        DQZ_HIP(hipEventRecord(pe.e1, st));                                 \
        DQZ_HIP(hipEventSynchronize(pe.e1));                                \
        float ms_ = 0.f;                                                    \
        (void)hipEventElapsedTime(&ms_, pe.e0, pe.e1);                      \
        if (t_ == 0 || ms_ < best_) best_ = ms_;                            \
      }                                                                     \
      pe.ms[i] = best_ / (float)pe.reps;                                    \
    }                                                                       \
  } while (0)

// conv1..fc1 forward of Z network copies (phases 0-3): conv1 -> conv2 ->
// conv3 as one hand-off launch (fwd_conv_kernel; since conv1 runs on bf16
// MFMA: 15,590 -> 16,050 steps/s against three launches), then the split-K
// fc1.  Used by the learner step and the actor.
// alternatives measured: DESIGN §4 "Tried in round 5"
static int forward_impl(dqz_learner* L, const NetZ& nz, int Z, int B, const Conv1Src& src, hipStream_t st,
                        PhaseEvents pe) {
  FwdArgs a = make_fwd_args(L, nz, Z, B, src);
  Conv1FwdArgs& c1 = a.c1;
  LayerFwdArgs &c2 = a.c2, &c3 = a.c3;
  // y1 / y2 hand-offs: 4 producer and `jobs` consumer blocks per sample
  const int jobs = fwd_conv_jobs(Z * B);
  c2.jobs = c3.jobs = jobs;
  c1.pub = c2.wait = handoff(L, sync_of(L).fwd_y1(jobs));
  c2.pub = c3.wait = handoff(L, sync_of(L).fwd_y2(jobs));
  const dim3 grid(xcd_grid(4, Z * B).x + 2 * xcd_grid(jobs, Z * B).x);
  DQZ_PHASE(0, switch (src.fused) {
    case 1: hipLaunchKernelGGL(fwd_conv_kernel<1>, grid, dim3(256), kConv1FwdSmem, st, c1, c2, c3); break;
    case 2: hipLaunchKernelGGL(fwd_conv_kernel<2>, grid, dim3(256), kConv1FwdSmem, st, c1, c2, c3); break;
    case 3: hipLaunchKernelGGL(fwd_conv_kernel<3>, grid, dim3(256), kConv1FwdSmem, st, c1, c2, c3); break;
    case 4: hipLaunchKernelGGL(fwd_conv_kernel<4>, grid, dim3(256), kConv1FwdSmem, st, c1, c2, c3); break;
    default: hipLaunchKernelGGL(fwd_conv_kernel<0>, grid, dim3(256), kConv1FwdSmem, st, c1, c2, c3); break;
  } DQZ_HIP(hipGetLastError()));
  if (pe.on()) pe.ms[1] = pe.ms[2] = 0.f;

  const Fc1FwdArgs& f1 = a.f1;
  DQZ_PHASE(3, if (B <= FC1_GEMV_MAXB)
                 hipLaunchKernelGGL(fc1_gemv_kernel, dim3(fc1_fwd_blocks(Z, 1)), dim3(256), 0, st, f1);
               else
                 hipLaunchKernelGGL(fc1_fwd32_kernel, dim3(fc1_fwd_blocks(Z, f1.MG)), dim3(256), 0, st, f1);
            DQZ_HIP(hipGetLastError()));
  return DQZ_OK;
}

static HeadArgs make_head(dqz_learner* L, const NetZ& nz, int Z, int B) {
  HeadArgs h{};
  memset(&h, 0, sizeof(h));
  h.fc1p = L->fc1p;
  h.S = L->S_fc1;
  h.h1 = L->h1;
  h.nz = nz;
  h.b1_off = L->off[7];
  h.w2_off = L->off[8];
  h.b2_off = L->off[9];
  h.Z = Z;
  h.B = B;
  h.A = L->cfg.num_actions;
  h.algo = L->cfg.algo;
  h.shared_bias = L->shared_bias;
  h.q = L->q;
  return h;
}

// The one place that decodes a request's batch source: the slots every kernel after conv1 reads and, for an
// in-launch draw, Conv1Src::fused, the draw in fsrc's union (when fsrc is given) and the counter the head advances.
struct Batch {
  int fused;
  const int32_t* slots;
  uint64_t* advance;
};
static Batch decode_batch(const StepRequest& r, Conv1Src* fsrc) {
  if (r.draw) {
    if (fsrc) fsrc->draw = *r.draw;
    return {1, r.draw->slots_out, r.draw->counter};
  }
  if (r.sm) {
    if (fsrc) fsrc->sm = *r.sm;
    return {2, r.sm->slots_out, r.sm->counter};
  }
  if (r.pd) {
    if (fsrc) fsrc->per = *r.pd;
    return {3, r.pd->out_slots, r.pd->inj_u ? nullptr : r.pd->counter};  // injected uniforms: no counter is read
  }
  if (r.smx) {
    if (fsrc) fsrc->smx = *r.smx;
    return {4, r.smx->slots_out, r.smx->counter};
  }
  return {0, r.slots, nullptr};
}

int dqz::check_step(const dqz_learner* L, const dqz_params* P, const dqz_store* S, const StepRequest& r) {
  if (!L || !P || !P->online || !P->target || !decode_batch(r, nullptr).slots)
    return fail(DQZ_ERR_INVALID, "null argument");
  if (!r.gout && !r.meta_epi && (!P->mu || !P->nu)) return fail(DQZ_ERR_INVALID, "null optimizer state");
  if (r.meta_epi && r.meta_epi->meta == 1 && (!P->mu || !P->nu)) return fail(DQZ_ERR_INVALID, "null optimizer state");
  if (int rc = check_store(S)) return rc;
  if (L->cfg.algo == DQZ_ALGO_PER && !r.is_weights && !r.pd) return fail(DQZ_ERR_INVALID, "PER step needs is_weights");
  if (!!r.draw + !!r.sm + !!r.smx + !!r.pd > 1) return fail(DQZ_ERR_INVALID, "a step takes at most one batch draw");
  if (r.wide) {  // a wide head: what it does not take, each by name (kWide words what the two say differently)
    const WideDesc& d = kWide[r.wide->kind];
    if (r.is_weights && !r.wide->weighted)
      return fail(DQZ_ERR_INVALID, "the %s head takes no importance weights", d.noun);
    if (r.wide->weighted && !r.is_weights)
      return fail(DQZ_ERR_INVALID, "a weighted %s step needs is_weights", d.noun);
    if (r.pd) return fail(DQZ_ERR_INVALID, "the %s head takes no prioritized draw", d.noun);
    if (r.draw || r.sm || r.smx) return fail(DQZ_ERR_INVALID, "the %s head takes no in-launch batch draw", d.noun);
    if (r.meta_p || r.meta_epi || r.meta_sm) return fail(DQZ_ERR_INVALID, "%s", d.no_meta);
    if (r.unit) return fail(DQZ_ERR_INVALID, "%s", d.no_unit);
    if (r.wb) return fail(DQZ_ERR_INVALID, "%s", d.no_wb);
    if (!r.gout) return fail(DQZ_ERR_INVALID, "%s", d.no_fused);
    if (L->cfg.batch == 1) return fail(DQZ_ERR_INVALID, "the %s head needs batch >= 2", d.noun);
    // a double_q head's inner learner is the three-copy one; no other algo stands behind a wide head
    if (L->cfg.algo != (r.wide->double_q ? DQZ_ALGO_DOUBLE : DQZ_ALGO_DQN))
      return fail(DQZ_ERR_INVALID, "the %s head runs on a DQN learner", d.noun);
  }
  return DQZ_OK;
}

// One learner step as the request describes it (learner_impl.hpp StepRequest), already checked.
int dqz::step_enqueue(dqz_learner* L, const dqz_params* P, const dqz_store* S, const StepRequest& r, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const PhaseEvents pe = r.pe;
  const PerSampleArgs* const pd = r.pd;
  const int B = L->cfg.batch, Z = L->Z, A = L->cfg.num_actions;
  const NetZ nz{{P->online, P->target, P->online}, {0, 1, 1}};  // online(s_tm1), target(s_t), online(s_t)
  Conv1Src fsrc{S->frames, S->fidx, nullptr, nullptr, 0, UniformDraw{}};  // the forward's, draw included
  fsrc.action = S->action;
  fsrc.reward = S->reward;
  fsrc.discount = S->discount;
  fsrc.rec = reinterpret_cast<float4*>(L->rec);
  fsrc.xout = r.xout;
  Conv1Src src = fsrc;  // conv1 dW's: the published slots, no draw
  const Batch batch = decode_batch(r, &fsrc);
  fsrc.fused = batch.fused;
  fsrc.slots = src.slots = batch.slots;
  if (pd) fsrc.per.out_wb = L->per_wb;
  if (int rc = forward_impl(L, nz, Z, B, fsrc, st, pe)) return rc;

  // an MGSC meta stage applied in the gradient epilogues (Rms), or plain
  // RMSProp / gradient output: every field set (value-initialised first)
  Rms rms{};
  if (r.meta_epi) rms = *r.meta_epi;
  rms.lr = L->cfg.learning_rate;
  rms.decay = L->cfg.decay;
  rms.c1 = (float)(1.0 - (double)L->cfg.decay);
  rms.eps = L->cfg.eps;
  rms.gout = r.gout;
  rms.gacc = r.gacc;
  rms.sq_off = 0;

  HeadArgs h = make_head(L, nz, Z, B);
  h.fwd_only = 0;
  h.slots = batch.slots;
  h.action = S->action;
  h.reward = S->reward;
  h.discount = S->discount;
  h.weights = L->cfg.algo == DQZ_ALGO_PER && !pd ? r.is_weights : nullptr;
  if (pd) {
    h.per_wb = L->per_wb;
    h.per_normalize = pd->normalize;
    h.per_w_out = pd->out_weights;
  }
  h.meta_p = r.meta_p;
  if (const MetaSoftmax* m = r.meta_sm) {
    h.meta_logits = m->logits;
    h.meta_pos = m->pos;
    h.meta_M = m->M;
    h.meta_x_out = m->x_out;
    h.meta_p_out = m->p_out;
  }
  h.rec = reinterpret_cast<const float4*>(L->rec);
  h.advance = batch.advance;
  h.unit = r.unit;
  h.bound = L->cfg.grad_error_bound;
  h.td = L->td;
  h.loss_part = L->loss_part;
  h.gq = L->gq;
  h.ga = L->ga;
  h.dz1 = L->dz1;

  // Backward: fc1 dX, then the merged launch that pairs the dX chain with the
  // independent dW job sets (bwd.hpp).
  Fc1BwdArgs fb{};
  fb.dz1 = L->dz1;
  fb.y3 = L->y3;
  fb.th = P->online;
  fb.mu = P->mu;
  fb.nu = P->nu;
  fb.w_off = L->off[6];
  fb.rms = rms;
  fb.B = B;
  fb.dy3 = L->dy3;
  fb.w3 = P->online + L->off[4];
  fb.w2 = P->online + L->off[2];
  fb.w3p = L->w3p;
  fb.w2p = L->w2p;
  if (r.wide) {
    // a wide head (c51.hpp, qr.hpp, the other code object): the outputs of both copies, then the per-sample loss
    // head, which writes dz1 itself (categorical) or a dense cotangent that a batched product turns into dz1
    // (quantile; slot 2 is one the other steps leave at 0); behind them the backward reads dz1 as from the
    // scalar head
    DQZ_PHASE(4, if (int rc = wide_launch(WIDE_OUTPUTS, L, P, r, st)) return rc);
    DQZ_PHASE(8, if (int rc = wide_launch(WIDE_HEAD, L, P, r, st)) return rc);
    const bool rb = r.wide->kind == WIDE_RB;
    if (r.wide->dout || rb) DQZ_PHASE(2, if (int rc = wide_launch(WIDE_DZ1, L, P, r, st)) return rc);
    if (rb)  // dy3 is the sum of four products (the noisy layers' mu and sigma of both streams)
      DQZ_PHASE(5, if (int rc = wide_launch(WIDE_FC1_DX, L, P, r, st)) return rc);
    else
      DQZ_PHASE(5, hipLaunchKernelGGL(fc1_dx_kernel, dim3(fc1_dx_blocks(B)), dim3(256), 0, st, fb);
                DQZ_HIP(hipGetLastError()));
  } else if (B == 1 && !pe.on()) {
    // one sample (the MGSC pass at theta', the HVP's unit-cotangent pass):
    // the head and fc1 dX in one launch, every block forming the head itself
    DQZ_HIP(launch_head_dx1(h, fb, st));
  } else {
    DQZ_PHASE(4, DQZ_HIP(launch_head(h, B, st)));
    DQZ_PHASE(5, hipLaunchKernelGGL(fc1_dx_kernel, dim3(fc1_dx_blocks(B)), dim3(256), 0, st, fb);
              DQZ_HIP(hipGetLastError()));
  }

  Conv3BwdArgs c3b{};
  c3b.dy3 = L->dy3;
  c3b.y2 = L->y2;
  c3b.w3 = P->online + L->off[4];
  c3b.w3p = L->w3p;
  c3b.dy2 = L->dy2;
  c3b.part = L->p3;
  c3b.B = B;
  c3b.sync = handoff(L, sync_of(L).dy2());
  Conv2BwdArgs c2b{};
  c2b.dy2 = L->dy2;
  c2b.y1 = L->y1;
  c2b.w2 = P->online + L->off[2];
  c2b.w2p = L->w2p;
  c2b.dy1 = L->dy1;
  c2b.part = L->p2;
  c2b.B = B;
  c2b.sync = c3b.sync;
  Conv1DwArgs c1dw{};
  c1dw.src = src;
  c1dw.src.rec = nullptr;
  c1dw.src.xout = nullptr;
  c1dw.which = 0;
  c1dw.B = B;
  c1dw.dy1 = L->dy1;
  c1dw.part = L->p1;
  c1dw.sync1 = handoff(L, sync_of(L).dy1());
  c2b.sync1 = c1dw.sync1;
  PerWbArgs wbk{};
  const bool wb = r.wb != nullptr;
  if (wb) {
    wbk = *r.wb;
    wbk.td = L->td;
    wbk.n = B;
  }
  const bool chain = bwd_chain_active(L);
  const dim3 grid(bwd_bc_blocks(B, wb, chain));
  auto* const bwd = wb ? (chain ? bwd_bc_kernel<true, true> : bwd_bc_kernel<true, false>)
                       : (chain ? bwd_bc_kernel<false, true> : bwd_bc_kernel<false, false>);
  DQZ_PHASE(6, hipLaunchKernelGGL(bwd, grid, dim3(256), 0, st, c3b, fb, c2b, c1dw, wbk);
            DQZ_HIP(hipGetLastError()));
  const bool wide = r.wide != nullptr;  // a head of the other code object owns the fc2 leaves
  if (pe.on() && !wide) pe.ms[7] = pe.ms[8] = 0.f;

  UpdArgs u{};
  u.th = P->online;
  u.mu = P->mu;
  u.nu = P->nu;
  for (int i = 0; i < 10; ++i) {
    u.off[i] = L->off[i];
    u.sz[i] = L->sz[i];
  }
  u.p1 = L->p1;
  u.p2 = L->p2;
  u.p3 = L->p3;
  u.S1 = B * C1_BLOCKS;
  u.S2 = L->S2;  // one dW partial slab per sample
  u.S3 = L->S3;
  u.h1 = L->h1;
  u.dz1 = L->dz1;
  u.gq = L->gq;
  u.ga = L->ga;
  u.loss_part = L->loss_part;
  u.loss = L->loss;
  u.status = L->sync + sync_of(L).err();
  // a wide head owns the fc2 leaves (WIDE_FC2_GRAD below): with A = nb2 = 0 the small head
  // leaves are fc1/b alone, update_blocks counts 8 blocks for them and no range of small_grad reaches fc2
  u.A = wide ? 0 : A;
  u.B = B;
  u.nb2 = wide ? 0 : L->shared_bias ? 1 : A;
  u.rms = rms;
  u.rms.sq_off = 4 * (FLAT / 16);  // meta_rms2 partials: the fc1 dW blocks' first, then the update's
  const unsigned nblk = update_blocks(L->sz, u.A, u.nb2);
  DQZ_PHASE(9, hipLaunchKernelGGL(update_kernel, dim3(nblk), dim3(256), 0, st, u);
            DQZ_HIP(hipGetLastError()));
  if (wide) DQZ_PHASE(7, if (int rc = wide_launch(WIDE_FC2_GRAD, L, P, r, st)) return rc);
  return DQZ_OK;
}

int dqz::fc1_forward(const Fc1FwdArgs& f, int Z, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (f.B <= FC1_GEMV_MAXB)
    hipLaunchKernelGGL(fc1_gemv_kernel, dim3(fc1_fwd_blocks(Z, 1)), dim3(256), 0, st, f);
  else
    hipLaunchKernelGGL(fc1_fwd32_kernel, dim3(fc1_fwd_blocks(Z, f.MG)), dim3(256), 0, st, f);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

int dqz::fc1_dx(const Fc1BwdArgs& f, void* stream) {
  hipLaunchKernelGGL(fc1_dx_kernel, dim3(fc1_dx_blocks(f.B)), dim3(256), 0, (hipStream_t)stream, f);
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

int dqz::forward_torso(dqz_learner* L, const float* params, const Conv1Src& src, int which, int n, void* stream) {
  const NetZ nz{{params, params, params}, {which, which, which}};
  return forward_impl(L, nz, 1, n, src, (hipStream_t)stream, PhaseEvents{});
}

extern "C" {

int dqz_learner_step(dqz_learner* L, const dqz_params* P, const dqz_store* S, const int32_t* slots,
                     const float* is_weights, void* stream) {
  return step_impl(L, P, S, {.slots = slots, .is_weights = is_weights}, stream);
}

int dqz_learner_step_per(dqz_learner* L, const dqz_params* P, const dqz_store* S, const int32_t* slots,
                         const float* is_weights, double* tree, int64_t cap, const int32_t* indices, double alpha,
                         double* max_seen_dev, void* stream) {
  if (!L || !tree || !indices || !max_seen_dev) return fail(DQZ_ERR_INVALID, "null argument");
  if (L->cfg.batch > 64) return fail(DQZ_ERR_INVALID, "the fused write-back takes batch <= 64 (use dqz_per_write_back)");
  if (cap < 1 || (cap & (cap - 1))) return fail(DQZ_ERR_INVALID, "cap must be a power of two");
  PerWbArgs wb;
  if (!per_wb_args(L, tree, cap, indices, alpha, max_seen_dev, &wb))
    return fail(DQZ_ERR_INVALID, "cap must be <= 2^%d for the fused write-back", PWB_LEVELS);
  return step_impl(L, P, S, {.slots = slots, .is_weights = is_weights, .wb = &wb}, stream);
}

int dqz_learner_step_uniform(dqz_learner* L, const dqz_params* P, const dqz_store* S, int64_t base, int64_t size,
                             int64_t capacity, uint64_t seed, uint64_t* counter_dev, int32_t* slots_out,
                             void* stream) {
  UniformDraw d;
  if (int rc = uniform_draw_args(L, base, size, capacity, seed, counter_dev, slots_out, &d)) return rc;
  return step_impl(L, P, S, {.draw = &d}, stream);
}

int dqz_learner_grad(dqz_learner* L, const dqz_params* P, const dqz_store* S, const int32_t* slots,
                     const float* is_weights, float* grad_out, void* stream) {
  if (!grad_out) return fail(DQZ_ERR_INVALID, "null grad_out");
  return step_impl(L, P, S, {.slots = slots, .is_weights = is_weights, .gout = grad_out}, stream);
}

int dqz_learner_profile(dqz_learner* L, const dqz_params* P, const dqz_store* S, const int32_t* slots,
                        const float* is_weights, int iters, float* phase_ms, void* stream) {
  return profile_step(L, P, S, {.slots = slots, .is_weights = is_weights}, iters, phase_ms, stream);
}

int dqz_learner_sync_status(dqz_learner* L, int* status) {
  if (!L || !status) return fail(DQZ_ERR_INVALID, "null argument");
  DQZ_HIP(hipDeviceSynchronize());
  DQZ_HIP(hipMemcpy(status, L->sync + sync_of(L).err(), sizeof(int), hipMemcpyDeviceToHost));
  if (*status != 0) {
    // A wait gave up: its consumers ran on partial payloads and producers may
    // have arrived after the last consumer reset the words, which would let
    // later launches pass their waits early.  Clear every hand-off word (and
    // the error word) so the next step starts clean; the caller must treat
    // the steps since the previous check as invalid.
    DQZ_HIP(hipMemset(L->sync, 0, sizeof(int) * sync_of(L).ints()));
    DQZ_HIP(hipDeviceSynchronize());
  }
  return DQZ_OK;
}

int dqz_learner_debug_stall(dqz_learner* L, int sample, unsigned spin_max) {
  if (!L) return fail(DQZ_ERR_INVALID, "null learner");
  if (sample >= L->cfg.batch) return fail(DQZ_ERR_INVALID, "sample out of range");
  L->spin_max = spin_max ? spin_max : 1u << 24;
  if (sample >= 0) {  // sample's dy2 arrival counter far below its 8 arrivals: its waits run out
    const int32_t poison = -(1 << 30);
    const SyncLayout at = sync_of(L);
    DQZ_HIP(hipDeviceSynchronize());
    DQZ_HIP(hipMemcpy(L->sync + at.dy2().cnt + at.word(sample), &poison, sizeof(poison), hipMemcpyHostToDevice));
  }
  return DQZ_OK;
}

int dqz_learner_debug_backward(dqz_learner* L, int chain, int* active) {
  if (!L) return fail(DQZ_ERR_INVALID, "null learner");
  if (chain < -1 || chain > 1) return fail(DQZ_ERR_INVALID, "chain must be -1, 0 or 1");
  L->bwd_chain = chain;
  if (active) *active = bwd_chain_active(L) ? 1 : 0;
  return DQZ_OK;
}

int dqz_learner_debug_sync_words(dqz_learner* L, int32_t* out, int64_t n, int64_t* total) {
  if (!L) return fail(DQZ_ERR_INVALID, "null learner");
  const int64_t ints = sync_of(L).ints();
  if (total) *total = ints;
  if (n < 0 || n > ints) return fail(DQZ_ERR_INVALID, "n must be in [0, %lld]", (long long)ints);
  if (n > 0 && !out) return fail(DQZ_ERR_INVALID, "null out");
  if (n == 0) return DQZ_OK;
  DQZ_HIP(hipDeviceSynchronize());
  DQZ_HIP(hipMemcpy(out, L->sync, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  return DQZ_OK;
}

int dqz_learner_outputs(dqz_learner* L, float* q_tm1, float* td, float* loss, void* stream) {
  if (!L) return fail(DQZ_ERR_INVALID, "null learner");
  hipStream_t st = (hipStream_t)stream;
  const int B = L->cfg.batch, A = L->cfg.num_actions;
  if (q_tm1) DQZ_HIP(hipMemcpyAsync(q_tm1, L->q, sizeof(float) * B * A, hipMemcpyDeviceToDevice, st));
  if (td) DQZ_HIP(hipMemcpyAsync(td, L->td, sizeof(float) * B, hipMemcpyDeviceToDevice, st));
  if (loss) DQZ_HIP(hipMemcpyAsync(loss, L->loss, sizeof(float), hipMemcpyDeviceToDevice, st));
  return DQZ_OK;
}

// q_values of n states through one copy: the torso, then the head in forward mode (the actor's: with its draw)
static int forward_q(dqz_learner* L, const float* params, const Conv1Src& src, int which, int n, float* q_out,
                     const ActorDraw* act, hipStream_t st) {
  if (int rc = forward_torso(L, params, src, which, n, st)) return rc;
  HeadArgs h = make_head(L, NetZ{{params, params, params}, {which, which, which}}, 1, n);
  h.fwd_only = 1;
  h.q = q_out;
  if (act) {
    h.act_out = act->out;
    h.eps = act->eps;
    h.act_seed = act->seed;
    h.act_ctr = act->counter;
  }
  DQZ_HIP(launch_head(h, n, st));
  DQZ_HIP(hipGetLastError());
  return DQZ_OK;
}

int dqz_forward(dqz_learner* L, const float* params, const uint8_t* states, int n, float* q_out, void* stream) {
  Conv1Src src;
  if (int rc = forward_src(L, params, n, {.states = states, .q_out = q_out}, &src)) return rc;
  return forward_q(L, params, src, 0, n, q_out, nullptr, (hipStream_t)stream);
}

int dqz_forward_slots(dqz_learner* L, const float* params, const dqz_store* S, const int32_t* slots, int n, int which,
                      float* q_out, void* stream) {
  Conv1Src src;
  const ForwardInput in{.from_store = true, .store = S, .slots = slots, .which = which, .q_out = q_out};
  if (int rc = forward_src(L, params, n, in, &src)) return rc;
  return forward_q(L, params, src, which, n, q_out, nullptr, (hipStream_t)stream);
}

int dqz_act(dqz_learner* L, const float* params, const uint8_t* states, int n, double epsilon, uint64_t seed,
            uint64_t counter, dqz_action* out, void* stream) {
  ActorDraw act{epsilon, seed, counter, out};
  Conv1Src src;
  if (int rc = forward_src(L, params, n, {.states = states, .act = &act}, &src)) return rc;
  return forward_q(L, params, src, 0, n, L->q, &act, (hipStream_t)stream);
}

}  // extern "C"

#ifdef DQZ_TRACE
// Diagnostic builds only (not part of include/dqz.h): copy / clear the
// in-kernel timeline stamps (common.hpp DQZ_STAMP).
extern "C" int dqz_debug_trace(unsigned long long* host_out, int clear) {
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

