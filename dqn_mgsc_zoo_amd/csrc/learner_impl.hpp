// learner_impl.hpp — host-side internals shared by libdqz's two translation
// units (common.hpp, "Two translation units, two code objects"): the learner
// handle, its parameter layout and hand-off words (layout.hpp), argument
// checks and the builders of the fused draws' kernel arguments, the forward's
// argument builder, the front half of both heads' forward and actor entries
// (forward_src), and the learner step's request (StepRequest) and entry
// (step_impl; its two halves are learner_step.hip's) that the MGSC meta-update and the
// fused samplers in learner.hip call.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>

#include "common.hpp"
#include "layout.hpp"
#include "conv1.hpp"
#include "fwd.hpp"
#include "head.hpp"
#include "bwd.hpp"
#include "sampling.hpp"

namespace dqz {

inline void param_layout(int A, int shared_bias, int64_t off[10], int64_t sz[10], int64_t* total) {
  const int64_t sizes[10] = {C1KK * C1CO, C1CO, C2KK * C2CO, C2CO, C3KK * C3CO, C3CO,
                             (int64_t)FLAT * HID, HID, (int64_t)HID * A, shared_bias ? 1 : A};
  int64_t o = 0;
  for (int i = 0; i < 10; ++i) {
    off[i] = o;
    sz[i] = sizes[i];
    o += (sizes[i] + 63) / 64 * 64;
  }
  *total = o;
}

}  // namespace dqz

struct dqz_learner {
  dqz_learner_config cfg;
  int Z, shared_bias;
  int64_t off[10], sz[10], total;
  int S_fc1, S2, S3;
  float *y1, *y2, *y3, *fc1p, *h1, *q, *dz1, *dy3, *dy2, *dy1, *p1, *p2, *p3, *td, *loss, *loss_part, *gq, *rec;
  float *w3p, *w2p;  // dX-ordered weight copies written by fc1_dx_kernel each step
  double* per_wb;    // [B] the fused PER draw's unnormalised IS weights (conv1 -> head)
  int32_t* ga;
  int32_t* sync;  // hand-off words and the error word: read them through sync_of / handoff (below)
  unsigned spin_max = 1u << 24;  // hand-off polls before a wait gives up
  int bwd_chain = -1;            // bwd_bc_kernel's grid: -1 the default, 0 / 1 forced (dqz_learner_debug_backward)
  void* block;
};

namespace dqz {

static_assert(Handoff::kStride == kWordStride, "layout.hpp's word stride is Handoff's");

// dqz_learner::sync by name (layout.hpp): the layout, and one of its hand-offs as the kernels' argument
inline SyncLayout sync_of(const dqz_learner* L) { return SyncLayout{L->cfg.batch}; }
inline Handoff handoff(const dqz_learner* L, const HandoffWords& w) {
  Handoff h{L->sync + w.cnt, L->sync + w.ack, L->sync + sync_of(L).err(), w.need, w.consumers};
  if (w.learner_spin) h.spin_max = L->spin_max;  // dqz_learner_debug_stall shortens the backward's waits only
  return h;
}

// Whether the learner's next backward launch runs bwd_bc_kernel's chain grid (bwd.hpp): legal up to
// BWD_CHAIN_MAXB samples (the termination argument above the kernel), and there the default, except for the
// one-sample learner: nothing queues for a slot on an empty chip, and the MGSC meta-update's B = 1 passes measured
// 1 % slower chained (DESIGN §4 "Round 7").
inline bool bwd_chain_active(const dqz_learner* L) {
  if (L->cfg.batch > BWD_CHAIN_MAXB) return false;
  return L->bwd_chain < 0 ? L->cfg.batch > 1 : L->bwd_chain != 0;
}

inline int check_store(const dqz_store* S) {
  if (!S || !S->frames || !S->fidx || !S->action || !S->reward || !S->discount)
    return fail(DQZ_ERR_INVALID, "store has a null buffer");
  if (S->capacity < 1) return fail(DQZ_ERR_INVALID, "store capacity must be positive");
  return DQZ_OK;
}

// Device address of p: device memory as is, pinned host memory through its
// mapped device pointer.  Pageable host memory is refused (a kernel access
// would fault).
inline int device_view(const void* p, const void** out, const char* what) {
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();
    return fail(DQZ_ERR_INVALID, "%s must be device memory or pinned host memory", what);
  }
  if (attr.type == hipMemoryTypeHost) {
    void* d = attr.devicePointer;
    if (!d && hipHostGetDevicePointer(&d, const_cast<void*>(p), 0) != hipSuccess) {
      (void)hipGetLastError();
      return fail(DQZ_ERR_INVALID, "%s: pinned host memory without a device mapping", what);
    }
    *out = d;
  } else if (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged ||
             attr.type == hipMemoryTypeUnified) {
    *out = p;
  } else {
    return fail(DQZ_ERR_INVALID, "%s must be device memory or pinned host memory", what);
  }
  return DQZ_OK;
}

inline int check_which(int which) {
  if (which != 0 && which != 1) return fail(DQZ_ERR_INVALID, "which must be 0 (s_tm1) or 1 (s_t)");
  return DQZ_OK;
}

// The actor's eps-greedy draw in a forward's head (dqz_act, dqz_c51_act): draw `counter` of Philox stream `seed`.
struct ActorDraw {
  double eps;
  uint64_t seed, counter;
  dqz_action* out;  // [n]
};

// The front half of both heads' forward and actor entries (dqz_forward, dqz_forward_slots, dqz_act and their
// dqz_c51_* twins): every argument check, in the order the entries have always refused, then conv1's source.  The
// n inputs are `states` [n][84][84][4] or, with from_store, stack `which` of `store`'s `slots` [n].  The result
// goes to q_out, or with `act` (the actor's call) to act->out; the actor's states and act->out may be pinned host
// memory and are replaced by their device views.
struct ForwardInput {
  const uint8_t* states;
  bool from_store;
  const dqz_store* store;
  const int32_t* slots;
  int which;
  const float* q_out;
  ActorDraw* act;
};
inline int forward_src(const dqz_learner* L, const float* params, int n, ForwardInput in, Conv1Src* src) {
  if (!L || !params || !(in.from_store ? (const void*)in.slots : in.states) ||
      !(in.act ? (const void*)in.act->out : in.q_out))
    return fail(DQZ_ERR_INVALID, "null argument");
  if (in.from_store)
    if (int rc = check_store(in.store)) return rc;
  if (n < 1 || n > L->cfg.batch) return fail(DQZ_ERR_INVALID, "n must be in [1, %d]", L->cfg.batch);
  if (in.from_store) {
    if (int rc = check_which(in.which)) return rc;
    *src = Conv1Src{in.store->frames, in.store->fidx, in.slots, nullptr, 0, UniformDraw{}};
    return DQZ_OK;
  }
  if (ActorDraw* a = in.act) {
    if (!(a->eps >= 0.0 && a->eps <= 1.0)) return fail(DQZ_ERR_INVALID, "epsilon must be in [0, 1]");
    const void *dstates = nullptr, *dout = nullptr;
    if (int rc = device_view(in.states, &dstates, "states")) return rc;
    if (int rc = device_view(a->out, &dout, "out")) return rc;
    in.states = static_cast<const uint8_t*>(dstates);
    a->out = static_cast<dqz_action*>(const_cast<void*>(dout));
  }
  if (reinterpret_cast<uintptr_t>(in.states) % 16) return fail(DQZ_ERR_INVALID, "states must be 16-byte aligned");
  *src = Conv1Src{nullptr, nullptr, nullptr, in.states, 0, UniformDraw{}};
  return DQZ_OK;
}

// dqz_learner_profile: each phase's launch is repeated `reps` times back to
// back between two events on the launch stream, so ms[i] is that kernel's
// average duration in a saturated stream (what rocprofv3's kernel trace
// reports), not a single launch plus its dispatch gap.
struct PhaseEvents {
  hipEvent_t e0, e1;
  int reps;
  float* ms;
  bool on() const { return ms != nullptr; }
};

inline int tree_levels(int64_t cap) {
  int l = 0;
  while ((int64_t(1) << l) < cap) ++l;
  return l;
}

// The in-launch uniform draw's checks (L may be null: the step refuses that itself), then *d.
inline int uniform_draw_args(const dqz_learner* L, int64_t base, int64_t size, int64_t capacity, uint64_t seed,
                             uint64_t* counter_dev, int32_t* slots_out, UniformDraw* d) {
  if (!counter_dev || !slots_out) return fail(DQZ_ERR_INVALID, "null argument");
  if (size < 1) return fail(DQZ_ERR_INVALID, "cannot sample from an empty replay (size=%lld)", (long long)size);
  if (capacity < size || base < 0) return fail(DQZ_ERR_INVALID, "bad replay geometry");
  if (L && L->cfg.algo == DQZ_ALGO_PER) return fail(DQZ_ERR_INVALID, "PER samples by priority, not uniformly");
  *d = UniformDraw{base % capacity, size, capacity, seed, counter_dev, slots_out};
  return DQZ_OK;
}

// The PER write-back fused into the backward launch (one wave: batch <= 64, at most PWB_LEVELS tree levels):
// fills *wb (the step sets td and n) and says whether the geometry fits; the callers word their own refusals.
inline bool per_wb_args(const dqz_learner* L, double* tree, int64_t cap, const int32_t* indices, double alpha,
                        double* max_seen_dev, PerWbArgs* wb) {
  *wb = PerWbArgs{tree, cap, tree_levels(cap), indices, nullptr, alpha, 0, max_seen_dev};
  return L->cfg.batch <= 64 && wb->levels <= PWB_LEVELS;
}

// conv1 .. fc1 forward arguments of Z network copies on L's activations: every layer field.  forward_impl adds
// the in-launch hand-offs; the MGSC tangent stage overrides linear, out, part and dot.
struct FwdArgs {
  Conv1FwdArgs c1;
  LayerFwdArgs c2, c3;
  Fc1FwdArgs f1;
};
inline FwdArgs make_fwd_args(const dqz_learner* L, const NetZ& nz, int Z, int B, const Conv1Src& src) {
  FwdArgs a{};
  a.c1.src = src;
  a.c1.nz = a.c2.nz = a.f1.nz = nz;
  a.c1.w_off = L->off[0];
  a.c1.b_off = L->off[1];
  a.c1.B = a.c2.B = a.f1.B = B;
  a.c1.Z = a.c2.Z = Z;
  a.c2.in = a.c1.out = L->y1;
  a.c2.w_off = L->off[2];
  a.c2.b_off = L->off[3];
  a.c2.out = L->y2;
  a.c3 = a.c2;
  a.c3.in = L->y2;
  a.c3.w_off = L->off[4];
  a.c3.b_off = L->off[5];
  a.f1.in = a.c3.out = L->y3;
  a.f1.w_off = L->off[6];
  a.f1.MG = (B + 31) / 32;
  a.f1.part = L->fc1p;
  return a;
}

// The meta batch's softmax formed by the batch learner's head (one meta chunk; HeadArgs::meta_logits):
// p = softmax(logits[pos[0..M)]), block b writes x_out[b] = logits[pos[b]] and p_out[b].
struct MetaSoftmax {
  const float* logits;
  const int32_t* pos;
  int M;
  float *x_out, *p_out;
};

// A wide head in place of the scalar one (StepRequest::wide): the categorical (C51; c51.hpp) or the quantile
// (QR-DQN; qr.hpp) one.  The learner's parameter layout then ends in fc2 leaves A * N wide (wide_param_layout;
// the quantile head's columns are quantile-major, i A + a), the step runs in gradient mode, and the head's and
// the fc2 gradient's launches, which live in the other code object, are made by wide_launch.
// WIDE_RB is the categorical head behind the noisy dueling network of the Rainbow agent (rainbow.hpp): its loss,
// projection, a* and priorities are the categorical head's with double_q and weighted both set, and the launches
// around it (the other three fc1 products, both noisy fc2 layers, the dueling combine and their backward) are
// wide_launch's as well.  They read the request's noise (StepRequest::noise) and the network's own leaves and
// scratch, RbNet (learner.hip), which the head's handle owns.
enum WideKind { WIDE_C51, WIDE_QR, WIDE_RB };
struct RbNet;
struct WideHead {
  WideKind kind;
  int N;              // atoms / quantiles per action
  const float* grid;  // [N] device: the support, strictly increasing / tau, each strictly inside (0, 1)
  float kappa;        // huber_param > 0 (quantile head only)
  float* out;         // [Z][B][A N] online(s_tm1), target(s_t) and, with double_q, online(s_t): logits / quantile
                      // outputs (Z is the inner learner's: 2, or 3 with double_q)
  float* taken;       // [B][N] online outputs of the taken action (la / theta)
  float* dtaken;      // [B][N] d loss / d those outputs (dl / dtheta)
  float* dout;        // [B][A N] (+ QR_PAD) the dense cotangent of the online outputs; null for the categorical
                      // head, whose head kernel writes dz1 itself
  float* qv;          // [Z][B][A] q_values
  int32_t* astar;     // [B] argmax_a q_values of the target copy (double_q: of the third copy, the selector)
  // dqz_c51_create_opt / dqz_qr_create_opt (dqz_wide_options); both 0 in a head of the plain creates
  int double_q;       // the inner learner runs three copies (DQZ_ALGO_DOUBLE's Z) and copy 2 selects a*
  int weighted;       // every step takes is_weights [B]; the head writes clip(|loss_b|, 0, 100) to the learner's td
  float* loss_b;      // [B] the unweighted per-sample loss of a weighted head (the learner's loss_part then holds
                      // w_b loss_b, what the update sums); null otherwise
  const RbNet* rb;    // WIDE_RB alone: the noisy dueling network in front of the head; null otherwise
};
constexpr int C51_MAX_ATOMS = 64, C51_MAX_OUT = 1024;     // c51.hpp's C51_MAXN / C51_MAXOUT
constexpr int QR_MAX_QUANTILES = 256, QR_MAX_OUT = 4096;  // qr.hpp's QR_MAXN / QR_MAXOUT

// What the host says differently for the two kinds (indexed by WideKind): the limits of N and A * N, and the
// words of the refusals; the four whole messages are those the heads word differently beyond the noun.
struct WideDesc {
  const char *noun, *count, *grid;  // "the <noun> head", "<count> must be in ...", "copy of the <grid> failed"
  int min_n, max_n, max_out;
  const char *no_meta, *no_unit, *no_wb, *no_fused;
};
inline constexpr WideDesc kWide[3] = {
    {"categorical", "num_atoms", "support", 2, C51_MAX_ATOMS, C51_MAX_OUT,
     "the categorical head has no MGSC meta mode", "the categorical head has no unit-cotangent pass",
     "the categorical head has no TD error to write back as a priority",
     "the categorical head runs in gradient mode only (no fused centered RMSProp)"},
    {"quantile", "num_quantiles", "quantiles", 1, QR_MAX_QUANTILES, QR_MAX_OUT,
     "the quantile head takes no MGSC meta mode", "the quantile head takes no unit-cotangent pass",
     "the quantile head takes no PER priority write-back",
     "the quantile head takes no fused centered RMSProp (it runs in gradient mode only)"},
    {"rainbow", "num_atoms", "support", 2, C51_MAX_ATOMS, C51_MAX_OUT,
     "the rainbow head has no MGSC meta mode", "the rainbow head has no unit-cotangent pass",
     "the rainbow head writes its priorities back through dqz_per_write_back (no fused write-back)",
     "the rainbow head runs in gradient mode only (no fused centered RMSProp)"}};

inline void wide_param_layout(int A, int N, int64_t off[10], int64_t sz[10], int64_t* total) {
  param_layout(A * N, 0, off, sz, total);  // leaves 0-7 are any DQN network's; fc2 is [512, A N] + [A N]
}
enum WideLaunch { WIDE_OUTPUTS, WIDE_HEAD, WIDE_DZ1, WIDE_FC2_GRAD, WIDE_FC1_DX };

// What one learner step is asked to do, set by name ({.slots = ..., .gout = ...}).  Everything left out is the
// plain step: centered RMSProp on P->online / mu / nu over the batch `slots`.
struct StepRequest {
  // The batch: `slots` [B], or exactly one in-launch draw (more are refused): conv1 draws the batch itself and
  // publishes the slots to the draw's own output, which the later kernels read; the head advances its counter.
  const int32_t* slots;
  const float* is_weights;      // [B] PER importance weights when the batch comes as `slots`
  const UniformDraw* draw;      // uniform over the live window (dqz_learner_step_uniform)
  const SoftmaxDraw* sm;        // learned logits, running state (dqz_learner_step_logits)
  const SoftmaxDrawExact* smx;  // learned logits, numpy-exact (dqz_learner_step_logits_exact)
  const PerSampleArgs* pd;      // prioritized: the head also forms the IS weights (dqz_learner_step_per_draw)
  // Gradient mode: the full gradient is written to gout (dqz parameter layout; gacc = 1 adds into it: meta-batch
  // chunks) and P->online / mu / nu are left untouched.
  float* gout;
  int gacc;
  const PerWbArgs* wb;  // the PER priority write-back fused into the backward launch (per_wb_args)
  // MGSC meta mode (dqz_meta_update)
  const float* meta_p;         // [B] per-sample cotangents p_b * (-clip(td_b))
  int unit;                    // 1: unit cotangent on q[a] (the HVP's pass)
  const Rms* meta_epi;         // a meta stage applied in the gradient epilogues (Rms::meta, its buffers)
  const MetaSoftmax* meta_sm;  // the head forms p itself; meta_p is then its p_out
  uint8_t* xout;               // conv1 copies sample 0's s_tm1 bytes here (Conv1Src::xout)
  PhaseEvents pe;              // dqz_learner_profile: per-phase timing instead of one pass
  // A wide head (C51, QR-DQN or Rainbow): gradient mode only, batch from `slots`; check_step words what it refuses.
  const WideHead* wide;
  const float* noise;  // [3][len] a WIDE_RB head's noise, one vector per network copy (rb_noise_layout's len);
                       // the caller's for this call alone, read by no other head and not checked by check_step
};

// One of a wide head's launches of a learner step (learner.hip): the outputs of both copies (c51_logits_kernel,
// generic in the output width), the per-sample loss head (batch record from L->rec; the quantile one writes the
// dense cotangent), the quantile head's dz1 as a batched product (only with WideHead::dout), the fc2 gradient
// into gout's fc2 leaves.  WIDE_RB: the outputs are the noisy dueling network's q_logits, WIDE_DZ1 forms both
// streams' dz, WIDE_FC1_DX stands in for the step's fc1 dX launch (four products into dy3), and WIDE_FC2_GRAD
// writes every fc leaf but A1-mu, which sits where fc1 does and is the step's own.
int wide_launch(WideLaunch which, dqz_learner* L, const dqz_params* P, const StepRequest& r, void* stream);

// The step's fc1 kernels with other arguments, for a head of the other code object (WIDE_RB: the noisy layers'
// other three 3136 x 512 products): the split-K forward of Z copies (the kernel forward_impl would choose for
// f.B) and fc1 dX of f.B samples.
int fc1_forward(const Fc1FwdArgs& f, int Z, void* stream);
int fc1_dx(const Fc1BwdArgs& f, void* stream);

// conv1 .. fc1 forward of one network copy on n states (learner_step.hip's forward_impl, Z = 1): the fc1 split-K
// partials are left in L->fc1p for a head of the other code object.
int forward_torso(dqz_learner* L, const float* params, const Conv1Src& src, int which, int n, void* stream);

// One learner step (learner_step.hip): check_step, what a step checks before anything is enqueued, then
// step_enqueue, its launches.  A caller with launches of its own in front runs the two halves itself.
int check_step(const dqz_learner* L, const dqz_params* P, const dqz_store* S, const StepRequest& r);
int step_enqueue(dqz_learner* L, const dqz_params* P, const dqz_store* S, const StepRequest& r, void* stream);
inline int step_impl(dqz_learner* L, const dqz_params* P, const dqz_store* S, const StepRequest& r, void* stream) {
  if (int rc = check_step(L, P, S, r)) return rc;
  return step_enqueue(L, P, S, r, stream);
}

// dqz_learner_profile / dqz_c51_profile: the request's step with every phase timed into phase_ms (PhaseEvents).
inline int profile_step(dqz_learner* L, const dqz_params* P, const dqz_store* S, StepRequest r, int iters,
                        float* phase_ms, void* stream) {
  if (!phase_ms || iters < 1) return fail(DQZ_ERR_INVALID, "phase_ms must be non-null and iters >= 1");
  for (int i = 0; i < DQZ_NUM_PHASES; ++i) phase_ms[i] = 0.f;
  r.pe = PhaseEvents{nullptr, nullptr, iters, phase_ms};
  DQZ_HIP(hipEventCreate(&r.pe.e0));
  DQZ_HIP(hipEventCreate(&r.pe.e1));
  const int rc = step_impl(L, P, S, r, stream);
  (void)hipEventDestroy(r.pe.e0);
  (void)hipEventDestroy(r.pe.e1);
  return rc;
}

}  // namespace dqz
