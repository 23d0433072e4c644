/*
 * dqz.h — C ABI of the MI355X-native DQN learner step (libdqz.so).
 *
 * Plain C: raw pointers, sizes and a hipStream_t passed as void*.  No torch
 * types cross this boundary.  Every function returns DQZ_OK (0) on success or
 * a negative status; dqz_last_error() returns a thread-local message.
 *
 * Ownership: the caller owns every device buffer that holds
 * state (parameters, optimizer moments, frame pool, transition table, sampled
 * slot buffers).  The library borrows those pointers for the duration of an
 * enqueue and owns only the opaque learner handle and its scratch.  All work
 * is enqueued on the given stream; no call synchronises the device except
 * where it documents a host output.
 *
 * Each entry point names the reference interface it replaces (file:line in
 * Stalfoes/dqn_mgsc_zoo).
 */
#ifndef DQZ_H_
#define DQZ_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DQZ_OK 0
#define DQZ_ERR_INVALID (-1)
#define DQZ_ERR_HIP (-2)
#define DQZ_ERR_UNSUPPORTED (-3)

/* Learner algorithm: which TD loss and which network head.
 *  DQN     : rlax.q_learning, dqn_atari_network          (dqn/agent.py:85-107)
 *  DOUBLE  : rlax.double_q_learning, double_dqn_atari_network (shared bias)
 *            (double_q/agent.py:85-107, networks.py:338-349)
 *  PER     : DOUBLE + importance weights, |td| returned   (prioritized/agent.py:86-127)
 */
#define DQZ_ALGO_DQN 0
#define DQZ_ALGO_DOUBLE 1
#define DQZ_ALGO_PER 2

/* Frame geometry (processors.py:488-505): 84x84 grayscale frames, 4-stack,
 * HWC layout, channel order oldest -> newest, trailing zero padding. */
#define DQZ_FRAME_H 84
#define DQZ_FRAME_W 84
#define DQZ_STACK 4
#define DQZ_FRAME_BYTES (DQZ_FRAME_H * DQZ_FRAME_W)
#define DQZ_NUM_LEAVES 10

/* Thread-local message for the last failing call on this thread. */
const char* dqz_last_error(void);

/* Source hash this library was compiled from: the first 16 hex digits of the
 * SHA-256 over csrc/ (every .hip / .hpp) and include/dqz.h, baked in at build
 * time (__graft_entry__.build()).  The Python loader refuses a library whose
 * id differs from the sources beside it, so a GPU run proves which kernels it
 * tested.  "unset" when built without the id. */
const char* dqz_build_id(void);

/* Flat parameter layout of the NatureQNetwork (networks.py:181-221,352-363):
 * leaves in Haiku order
 *   0 conv2_d/w [8,8,4,32]   1 conv2_d/b [32]
 *   2 conv2_d_1/w [4,4,32,64] 3 conv2_d_1/b [64]
 *   4 conv2_d_2/w [3,3,64,64] 5 conv2_d_2/b [64]
 *   6 linear/w [3136,512]    7 linear/b [512]
 *   8 linear_1/w [512,A]     9 linear_1/b [A]   (shared_bias: [1])
 * Each leaf starts on a 64-float boundary; padding stays zero.
 * offsets/sizes are in floats; total is the padded buffer length. */
int dqz_param_layout(int num_actions, int shared_bias, int64_t offsets[DQZ_NUM_LEAVES],
                     int64_t sizes[DQZ_NUM_LEAVES], int64_t* total);

/* Replay storage in HBM (replaces the snappy-compressed per-transition
 * storage of replay.py:163-206 / replay_circular.py:90-146).
 *   frames   uint8 [num_frames][84*84]         frame pool
 *   fidx     int32 [capacity][8]               frame index of each stack
 *                                              channel: 0..3 = s_tm1, 4..7 = s_t,
 *                                              -1 = zero padding
 *   action   int32 [capacity]   reward f32 [capacity]   discount f32 [capacity]
 * A transition lives in a slot; slots are what the samplers return. */
typedef struct dqz_store {
  const uint8_t* frames;
  const int32_t* fidx;
  const int32_t* action;
  const float* reward;
  const float* discount;
  int64_t capacity;
  int64_t num_frames;
} dqz_store;

/* Online/target parameters and centered-RMSProp moments, all [total] f32
 * in the dqz_param_layout order (optax.rmsprop(centered=True) state,
 * dqn/run_atari.py:208-213). */
typedef struct dqz_params {
  float* online;
  float* target;
  float* mu;
  float* nu;
} dqz_params;

typedef struct dqz_learner_config {
  int batch;            /* B (replay.sample(batch_size)), 1..256 */
  int num_actions;      /* A, 1..32 */
  int algo;             /* DQZ_ALGO_* */
  float learning_rate;  /* dqn/run_atari.py:81 */
  float decay;          /* 0.95 */
  float eps;            /* dqn/run_atari.py:82 */
  float grad_error_bound; /* dqn/run_atari.py:80 (rlax.clip_gradient bound) */
} dqz_learner_config;

typedef struct dqz_learner dqz_learner;

/* Allocates the learner's scratch (activations, split-K partials). */
int dqz_learner_create(const dqz_learner_config* cfg, dqz_learner** out);
int dqz_learner_destroy(dqz_learner* learner);

/* One learner step = jitted `update` of dqn/agent.py:109-119
 * (prioritized/agent.py:115-127 for PER): forward online(s_tm1),
 * target(s_t) [+ online(s_t)], TD loss with clip_gradient, backward,
 * centered RMSProp, in place on params->online / mu / nu.
 * slots: device int32 [B] replay slots of the minibatch (from a sampler or
 * injected by the caller).  is_weights: device f32 [B] or NULL (PER only). */
int dqz_learner_step(dqz_learner* learner, const dqz_params* params, const dqz_store* store,
                     const int32_t* slots, const float* is_weights, void* stream);

/* Sampling fused into the step: the batch is `size` uniform draws
 * (base + floor(u * size)) mod capacity with Philox(counter, i; seed), as
 * dqz_sample_uniform would draw them, computed inside the conv1 kernel (no
 * separate sampler launch); the drawn slots are written to slots_out (device
 * int32 [B]) and *counter_dev advances by one.  Uniform FIFO / reservoir
 * replays (replay.py:119-125, 246-296). */
int dqz_learner_step_uniform(dqz_learner* learner, const dqz_params* params, const dqz_store* store,
                             int64_t base, int64_t size, int64_t capacity, uint64_t seed,
                             uint64_t* counter_dev, int32_t* slots_out, void* stream);

/* PER learner step with the priority write-back folded in
 * (prioritized/agent.py:187-206): dqz_learner_step on `slots` with the IS
 * weights, then — inside the same backward launch, in its first workgroup,
 * beside the backward pass — what dqz_per_write_back(tree, cap, indices,
 * alpha, max_seen_dev) does after it: p = |td|, *max_seen_dev = max(...,
 * max p), leaf[indices[i]] = p^alpha with the last draw of a repeated index
 * winning, ancestors rebuilt (bit-identical sums).  indices: device int32
 * [B] tree indices (dqz_per_sample's out_indices).  cap: a power of two <=
 * 2^24; batch <= 64.  Saves the write-back's own launch. */
int dqz_learner_step_per(dqz_learner* learner, const dqz_params* params, const dqz_store* store,
                         const int32_t* slots, const float* is_weights, double* tree, int64_t cap,
                         const int32_t* indices, double alpha, double* max_seen_dev, void* stream);

/* MGSC learner step with the batch drawn inside the learner's forward
 * launch (dqn_mgsc_batched/agent.py:341-360: replay.sample(batch) from
 * softmax(logits), then the DQN update): the draw is exactly
 * dqz_logits_sample_slots(buf, logits, seed, counter_dev, NULL, B,
 * slots_out, ...) — Philox uniform b of step *counter_dev (or uniforms[b]
 * when `uniforms`, device f64 [B], is given: the replay Generator's own
 * draws), the CDF search of dqz_logits_sample — computed by each of the
 * forward's conv1 workgroups before its frame gather (no sampler launch);
 * slots_out (device int32 [B]) receives the slots and *counter_dev advances
 * by one (Philox mode).  buf / logits: the replay's learned-logit buffer. */
typedef struct dqz_logit_buffer dqz_logit_buffer;
int dqz_learner_step_logits(dqz_learner* learner, const dqz_params* params, const dqz_store* store,
                            dqz_logit_buffer* buf, const float* logits, uint64_t seed, uint64_t* counter_dev,
                            const double* uniforms, int32_t* slots_out, void* stream);

/* The same step with the reference's own draw, bit for bit: the exact mode
 * of dqz_logits_sample_exact inside the forward launch.  Replaces
 * `self._rng_state.choice(self._capacity, size=size, p=self.as_probs())` with
 * p = probabilities_from_logits(logits) (replay_circular.py:69-76, 205-217,
 * 540-545) and the learner update that follows it
 * (dqn_mgsc_batched/agent.py:341-360).  Three preparation launches form c,
 * the float32 logsumexp and the chunk sums of p = exp(x - lse) as numpy does;
 * then each conv1 workgroup of sample b searches the CDF for uniforms[b]
 * (device f64 [B], the replay Generator's random(B)) or for Philox uniform b
 * of step *counter_dev, which then advances by one.  Exactly one of
 * counter_dev / uniforms is given.  slots_out: device int32 [B].  Independent
 * of the running log-sum-exp state; no host synchronisation, no allocation,
 * capturable in a graph.  Calls that share one dqz_logit_buffer
 * (dqz_logits_sample_exact and dqz_logits_add_exact included) must be ordered
 * on one stream: they share its scratch. */
int dqz_learner_step_logits_exact(dqz_learner* learner, const dqz_params* params, const dqz_store* store,
                                  dqz_logit_buffer* buf, const float* logits, uint64_t seed,
                                  uint64_t* counter_dev, const double* uniforms, int32_t* slots_out,
                                  void* stream);

/* Gradient only: d loss / d params of the same step into grad_out (device
 * f32, dqz_param_layout order, padding untouched); params->online / mu / nu
 * are not modified and mu / nu may be NULL.  = jax.grad(loss_fn) at
 * dqn/agent.py:112-116. */
int dqz_learner_grad(dqz_learner* learner, const dqz_params* params, const dqz_store* store,
                     const int32_t* slots, const float* is_weights, float* grad_out, void* stream);

/* Phases of one learner step, in launch order (dqz_learner_profile):
 *  0 conv1 fwd (uniform draw + frame gather fused)   1 conv2 fwd
 *  2 conv3 fwd   3 fc1 fwd (split-K)
 *  4 head: fc1 reduce + fc2 + TD loss + dq + dz1 (one workgroup per sample);
 *    with DQZ_FUSED_HEAD=1 also fc1 dX behind an in-launch dz1 hand-off
 *    (one launch, head_dx_kernel) and 5 reports 0
 *  5 fc1 dX
 *  6 conv3 dX -> conv2 dX -> conv1 dW and conv3 dX -> conv2 dW (in-launch
 *    per-sample hand-offs of dy2 / dy1) + fc1 dW and RMSProp of fc1/w +
 *    conv3 dW partials (one launch, bwd_bc_kernel)
 *  7 0 (merged into 6); in the DQZ_FUSED_BWD=0 debug layout 6 is conv3 dX +
 *    fc1 dW and 7 is conv2 dX + conv3 dW partials
 *  8 0 (merged into 6); with DQZ_FUSED_BWD=0 or DQZ_DW_LATE=1: conv1 dW
 *    partials (frame gather fused) + conv2 dW partials
 *  9 gradient reductions + RMSProp (all leaves but fc1/w) */
#define DQZ_NUM_PHASES 10

/* Per-phase kernel time: runs one learner step in which every phase's
 * launch is repeated `iters` times back to back between two hipEvents on
 * `stream`, three times; phase_ms[i] = the best trial's average
 * milliseconds per launch (the kernel's duration in a saturated stream,
 * comparable to rocprofv3 --kernel-trace; the best of three drops a trial
 * whose launching thread stalled and let the device idle).  Phases that
 * update state (4, 6, 9) apply their update 3 x `iters` times: call it on a
 * scratch copy or after the timed work.  Synchronises the stream. */
int dqz_learner_profile(dqz_learner* learner, const dqz_params* params, const dqz_store* store,
                        const int32_t* slots, const float* is_weights, int iters, float* phase_ms,
                        void* stream);

/* Device-to-device copies of the last step's outputs (any may be NULL):
 * q_tm1 [B][A] online Q(s_tm1), td [B] TD errors, loss [1] mean loss. */
int dqz_learner_outputs(dqz_learner* learner, float* q_tm1, float* td, float* loss, void* stream);

/* Health word of the learner since the previous check: *status = 0 when
 * every in-launch hand-off wait of the backward pass completed and every
 * batch loss was finite; bit 0 (1): a wait gave up (a bounded spin expired;
 * the step's results are then invalid); bit 1 (2): a step's mean loss was
 * NaN or infinite (the update still ran, as the reference's jitted update
 * would).  Synchronises the device.  A non-zero status also clears every
 * hand-off word and the status, so the next step starts clean; callers treat
 * the steps since their previous check as invalid. */
int dqz_learner_sync_status(dqz_learner* learner, int* status);

/* Diagnostic (tests): the bounded hand-off spin gives up after `spin_max`
 * polls from the next step on (0 restores the default 2^24), and if sample
 * >= 0 that sample's dy2 arrival counter is poisoned so the next step's
 * waits on it run out — the timeout path of dqz_learner_sync_status,
 * exercised.  Synchronises the device. */
int dqz_learner_debug_stall(dqz_learner* learner, int sample, unsigned spin_max);

/* Diagnostic (tests, A/B timing): which grid the backward launch
 * (bwd_bc_kernel) uses from the next enqueued step on.  chain = 1 forces the
 * chain grid (one resident workgroup carries a job through conv3 dX, conv2
 * dX and conv1 dW) where it is legal (batch <= 64), 0 forces the grid of
 * separate block ranges, -1 restores the default (the chain grid for
 * 2 <= batch <= 64).  Both compute the same
 * bits.  *active (may be NULL) returns what the next step will use: 1 the
 * chain grid, 0 the separate ranges.  A captured graph keeps the grid it was
 * captured with. */
int dqz_learner_debug_backward(dqz_learner* learner, int chain, int* active);

/* Diagnostic (tests): the learner's in-launch hand-off words, read back.
 * *total (may be NULL) returns how many ints the learner keeps: the arrival
 * and acknowledgement words of every hand-off (64 ints apart) and the error
 * word of dqz_learner_sync_status.  With n > 0 the device is synchronised
 * and the first n <= *total ints are copied to the host array `out`; n = 0
 * only reports *total.  Between launches every int is zero (a wait that gave
 * up leaves the error word set until dqz_learner_sync_status reads it). */
int dqz_learner_debug_sync_words(dqz_learner* learner, int32_t* out, int64_t n, int64_t* total);

/* Diagnostic (tests): device-to-device copies of the intermediates the
 * learner's scratch holds after its most recent learner step, gradient call
 * or forward (any output may be NULL; no kernel is launched; the copies are
 * ordered on `stream`).  Every array is plain f32, sample-major, NHWC.
 * Forward, network copy z — 0 online(s_tm1), 1 target(s_t), 2 online(s_t)
 * (double-Q and PER only); z outside [0, Z) is DQZ_ERR_INVALID:
 *   y1 [B][20][20][32], y2 [B][9][9][64], y3 [B][7][7][64] (= [B][3136], the
 *   flatten order of fc1), h1 [B][512]: the post-ReLU activations;
 *   q [B][A].
 * Backward, of copy 0 only (the one differentiated pass):
 *   dz1 [B][512], dy3 [B][3136], dy2 [B][9][9][64], dy1 [B][20][20][32]:
 *   d loss / d pre-activation of fc1, conv3, conv2, conv1, i.e. each already
 *   multiplied by its own layer's ReLU mask (y > 0), which is where the
 *   backward kernels take their masks from.  In a gradient call or a step
 *   the cotangent at q is -clip(w td / B); the MGSC meta passes weight it
 *   per sample instead.
 * After dqz_forward / dqz_forward_slots / dqz_act of n <= B states only
 * copy 0 is current, packed as [n][...] at the start of each array; q is
 * written by dqz_act alone (the other two write the caller's q_out), and the
 * backward arrays keep the last step's values. */
int dqz_learner_debug_activations(dqz_learner* learner, int z, float* y1, float* y2, float* y3, float* h1,
                                  float* q, float* dz1, float* dy3, float* dy2, float* dy1, void* stream);

/* Q-values of the NatureQNetwork for uint8 HWC states [n][84][84][4]
 * (network.apply(...).q_values, networks.py:352-363; used by select_action,
 * dqn/agent.py:121-131).  q_out: device f32 [n][A]. n <= learner batch. */
int dqz_forward(dqz_learner* learner, const float* params, const uint8_t* states, int n,
                float* q_out, void* stream);

/* Q-values for replay slots without materialising stacks:
 * which = 0 -> s_tm1, 1 -> s_t. */
int dqz_forward_slots(dqz_learner* learner, const float* params, const dqz_store* store,
                      const int32_t* slots, int n, int which, float* q_out, void* stream);

/* ---- actor path (dqn/agent.py:121-131, 169-177) -------------------------
 * select_action on device: q = Q(params, states[i]), v = max_a q,
 * a ~ distrax.EpsilonGreedy(q, epsilon): P(a) = (1 - eps) [q_a == v] / #ties
 * + eps / A (fp64, as parts.epsilon_greedy_probs), drawn by inverting the
 * CDF the way numpy's Generator.choice does (cumsum, normalised by its last
 * entry, first entry > u) with u = Philox4x32-10(key = seed, counter =
 * (counter, i)).  `states` (uint8 [n][84][84][4]) and `out` may be device
 * memory or pinned (hipHostMalloc / torch pin_memory) host memory, which
 * the kernels read and write in place: one call, no staging copies.  Host
 * results are valid after the stream is synchronised.  n <= learner batch. */
typedef struct dqz_action {
  int32_t action;
  float value; /* max_a q: the agent's statistics['state_value'] */
} dqz_action;
int dqz_act(dqz_learner* learner, const float* params, const uint8_t* states, int n, double epsilon,
            uint64_t seed, uint64_t counter, dqz_action* out, void* stream);

/* One replay add into the HBM store in one launch (TransitionReplay.add,
 * replay.py:182-192): copies `num_frames` new frames (uint8 [num_frames][7056]
 * at `frames`, device or pinned host memory) into pool rows frame_rows[i],
 * then writes the transition record {fidx, a, r, d} at `slot`.  Writes
 * through the store's (caller-owned, writable) buffers. */
typedef struct dqz_transition_put {
  int64_t slot;
  int32_t fidx[8];       /* pool rows of s_tm1 / s_t channels, -1 = zero padding */
  int32_t action;
  float reward, discount;
  int32_t num_frames;    /* <= 8 */
  int32_t frame_rows[8]; /* destination pool row of each new frame */
} dqz_transition_put;
int dqz_store_put(const dqz_store* store, const dqz_transition_put* t, const uint8_t* frames,
                  void* stream);

/* One replay add composed from stored transitions, device to device, in one
 * launch (the jumbled transition of
 * dqn_mgsc_batched_nonsense_transitions/agent.py:277-286: s_tm1, a_tm1, r_t,
 * discount_t and s_t each taken from another stored item).  For channel c in
 * 0..3 the source pool row is fidx[src_s_tm1][c], for c in 4..7 it is
 * fidx[src_s_t][c]; a source row >= 0 is copied (7,056 bytes) into pool row
 * frame_rows[c] and fidx[slot][c] = frame_rows[c]; a source row of -1 (zero
 * padding) gives fidx[slot][c] = -1 and leaves frame_rows[c] unused.
 * action[slot] = action[src_action], reward[slot] = reward[src_reward],
 * discount[slot] = discount[src_discount]; flags[slot] = 1 when `flags`
 * (device uint8 [capacity]) is given.  The copies are needed because a FIFO
 * frame ring recycles the sources' rows long before the composed item leaves
 * the replay.  `slot` may equal any source (on a full ring it is the s_tm1
 * source): every workgroup reads and writes only its own channel's fidx
 * entry.  frame_rows must be fresh rows: pairwise distinct and none of them a
 * row the sources reference (the allocator's job, store.FrameAllocator.reserve).
 * Writes through the store's (caller-owned, writable) buffers. */
typedef struct dqz_jumble {
  int64_t slot;
  int64_t src_s_tm1, src_action, src_reward, src_discount, src_s_t;
  int32_t frame_rows[8];
  uint8_t* flags;
} dqz_jumble;
int dqz_store_jumble(const dqz_store* store, const dqz_jumble* j, void* stream);

/* Uniform sampling with replacement over live transitions, on device
 * (UniformDistribution.sample, replay.py:119-125; replay_circular.py:283-289).
 * Live slots are (base + j) mod capacity for j in [0, size).  FIFO replay:
 * base = t - size; reservoir replay: base = 0.  Philox4x32-10 keyed by seed,
 * counter = (*counter_dev, lane); *counter_dev is incremented on device, so
 * the call is hipGraph-replayable. */
int dqz_sample_uniform(int64_t base, int64_t size, int64_t capacity, int n, uint64_t seed,
                       uint64_t* counter_dev, int32_t* out_slots, void* stream);

/* Materialise stacked uint8 states [n][84][84][4] for the given slots
 * (the np.stack of TransitionReplay.sample, replay.py:200-206).
 * which = 0 -> s_tm1, 1 -> s_t. */
int dqz_gather_stacks(const dqz_store* store, const int32_t* slots, int n, int which,
                      uint8_t* out, void* stream);

/* ---- learned-logit replay sampling (dqn_mgsc_batched replays) ----------
 * logits: device f32 [capacity], -inf marks an empty slot
 * (CircularLogitBuffer / MGSCReservoirDistribution, replay_circular.py:148-248,
 * 500-565).  A dqz_logit_buffer owns the running log-sum-exp state and one
 * float64 sum of the sampling terms per chunk of 4096 slots, both kept
 * current by every write through the library (capacity <= 2^42). */
int dqz_logit_buffer_create(int64_t capacity, int max_queries, dqz_logit_buffer** out);
int dqz_logit_buffer_destroy(dqz_logit_buffer* buf);

/* Default logit of an added item (replay_circular.py:166-179, :518-533):
 * if clear_pos >= 0, logits[clear_pos] = -inf first (the reservoir
 * `replace`); then logits[write_pos] = size == 0 ? 0
 *   : logsumexp(logits[0:capacity]) - log(size).  lse_out (device f32) may be NULL.
 * The buffer keeps a running float64 sum of exp(x - c), so an add is O(1);
 * it is re-seeded by a full scan after dqz_logits_invalidate, every 4096
 * running adds, or when a removal would cancel most of it.  Every write to
 * `logits` must go through dqz_logits_add / dqz_logits_write, or be followed
 * by dqz_logits_invalidate. */
int dqz_logits_add(dqz_logit_buffer* buf, float* logits, int64_t clear_pos, int64_t write_pos,
                   int64_t size, float* lse_out, void* stream);

/* logits[positions[i]] = values[i] for i in order (a repeated position keeps
 * its last value), keeping the running sum (popleft's -inf, __setitem__,
 * update_priorities: replay_circular.py:180-215).  positions: device int64
 * [n], values: device f32 [n]. */
int dqz_logits_write(dqz_logit_buffer* buf, float* logits, const int64_t* positions, const float* values, int n,
                     void* stream);

/* One write logits[position] = value (by value: popleft's -inf), keeping the
 * running sum and the chunk sum. */
int dqz_logits_put(dqz_logit_buffer* buf, float* logits, int64_t position, float value, void* stream);

/* Running log-sum-exp state of a logit buffer, for checkpoints
 * (parts.py:517-561): S = float64 sum of exp(x - c) over the buffer, the
 * shift c, the device-side valid flag, and the host bookkeeping (known: every
 * write since the last scan went through the library; adds: running adds
 * since that scan).  get synchronises `stream`; set restores all five and
 * recomputes the chunk sums from `logits` about c (they are a function of
 * the two), so a restored buffer continues with the saver's bits (no re-scan
 * on either side). */
int dqz_logits_run_get(dqz_logit_buffer* buf, double* S, float* c, int* valid, int* known, int* adds,
                       void* stream);
int dqz_logits_run_set(dqz_logit_buffer* buf, const float* logits, double S, float c, int valid, int known,
                       int adds, void* stream);

/* The logits were written outside the library (e.g. the meta-update's Adam
 * step, a state restore): the next dqz_logits_add re-scans the buffer. */
int dqz_logits_invalidate(dqz_logit_buffer* buf);

/* Softmax sampling with replacement (CircularLogitBuffer.sample,
 * replay_circular.py:205-217 = Generator.choice(capacity, n, p=softmax)):
 * terms t = expf(x - c) about the running shift c (softmax up to f32
 * rounding of the exponent), cdf = cumsum(float64 t) / total, out_idx[i] =
 * first slot with cdf > uniforms[i].  Reads the chunk sums and one chunk of
 * 4096 logits per query.  uniforms: device f64 [n] in [0,1) (host Generator
 * draws for parity, or dqz_uniform_philox). */
int dqz_logits_sample(dqz_logit_buffer* buf, const float* logits, const double* uniforms, int n,
                      int64_t* out_idx, void* stream);

/* Learner-batch draw in one launch: n uniforms — the caller's `uniforms`
 * (device f64, NULL for Philox) or Philox4x32 (seed, *counter_dev, q), the
 * stream dqz_uniform_philox produces, *counter_dev then advanced on device —
 * and the softmax-CDF choice of dqz_logits_sample, written as int32 slots
 * (out_slots, for dqz_learner_step) and/or int64 (out_idx); either may be
 * NULL.  Replaces Generator.choice(C, n, p=softmax(logits)) +
 * the batch's slot lookup (replay_circular.py:205-217, 540-545) without the
 * uniform launch or an int64 -> int32 copy. */
int dqz_logits_sample_slots(dqz_logit_buffer* buf, const float* logits, uint64_t seed, uint64_t* counter_dev,
                            const double* uniforms, int n, int32_t* out_slots, int64_t* out_idx, void* stream);

/* Diagnostic: the sampling probability of every slot, p = t / total as f32
 * (p_out: device f32 [capacity]; probabilities_from_logits,
 * replay_circular.py:69-76) and the running log-sum-exp (lse_out: device
 * f32, may be NULL). */
/* Exact mode of the learned-logit draw: the reference's own float32
 * probabilities p = probabilities_from_logits(logits) (replay_circular.py:69-76,
 * numpy's float32 exp / log / sum operation for operation, bit for bit) into
 * p_out (capacity floats, or NULL), and n draws for the caller's uniforms
 * (the Generator's random() stream) as Generator.choice(C, n, p) makes them
 * (replay_circular.py:205-217, :540-545): searchsorted(cumsum(p) / total, u,
 * 'right'), the cumsum in float64 in chunk order (a draw can differ from
 * numpy's sequential cumsum only for a uniform within float64 rounding of a
 * CDF step).  Four launches (three preparation passes over the buffer, then
 * the draws); independent of the running state.  Calls that share one
 * dqz_logit_buffer must be ordered on one stream: they share its scratch.
 * n = 0: p_out only.  Replaces the reference's `self._rng_state.choice(
 * self._capacity, size=size, p=self.as_probs())` (replay_circular.py:208). */
int dqz_logits_sample_exact(dqz_logit_buffer* buf, const float* logits, const double* uniforms, int n,
                            int64_t* out_idx, float* p_out, void* stream);
/* Exact mode of the default-logit add (replay_circular.py:166-179 add, :518-533
 * add / replace): logits[clear_pos] = -inf first when clear_pos >= 0, then
 * logits[write_pos] = 0 for size 0, else float32(logsumexp(logits) -
 * log(size)) with numpy's float32 logsumexp (as dqz_logits_sample_exact forms
 * it) and a float64 log.  Three small launches (four with a clear), two
 * passes over the buffer;
 * the running state is left unknown (the next default-mode call re-seeds). */
int dqz_logits_add_exact(dqz_logit_buffer* buf, float* logits, int64_t clear_pos, int64_t write_pos, int64_t size,
                         void* stream);
int dqz_logits_probs(dqz_logit_buffer* buf, const float* logits, float* p_out, float* lse_out, void* stream);

/* Diagnostic: the exact terms a draw's CDF is built from, t = expf(x - c)
 * (t_out: device f32 [capacity]), the chunk sums (csum_out: device f64
 * [ceil(capacity / 4096)], may be NULL) and c (c_out: device f32, may be
 * NULL).  Lets a checker separate the index search (bit-exact against numpy's
 * sequential-cumsum choice given the same t) from the last-ulp differences of
 * f32 exp between numpy and the device. */
int dqz_logits_terms(dqz_logit_buffer* buf, const float* logits, float* t_out, double* csum_out, float* c_out,
                     void* stream);

/* Census of the learned logits by class of transition: one pass of the
 * per-timestep walk of dqn_mgsc_batched_nonsense_transitions/agent.py:290-310
 * over the live window (left_head + i) mod capacity, i < size, on device.
 * flags: device uint8 [capacity], class 1 (nonsense) where non-zero, class 0
 * (real) otherwise (dqz_store_jumble sets them).  acc_dev: a dqz_census in
 * device memory owned by the caller, who initialises it (max_seen = -inf,
 * min_seen = +inf, the rest 0).  Per class:
 *   max_seen / min_seen  over the live logits of every call so far;
 *   probe_sum / probe_num  the logit at five positions of the window, added
 *     once per call to the class of the slot found there: [0] entry
 *     (i = size - 1), [1] 1st_quarter (3 (size / 4)), [2] 2nd_quarter
 *     (size / 2), [3] 3rd_quarter (size / 4), [4] exit (0).  A position that
 *     matches several probes counts once, for the first of exit, 3rd, 2nd,
 *     1st, entry (the reference's elif chain).  Sums are float64, one add
 *     per call (the reference accumulates in float32);
 *   count  live slots of the class, this call;
 *   mass   the class's share of the sampling probability, this call:
 *     sum_class exp((double)x - (double)m) / sum_all, m the largest live
 *     logit (0 when nothing is live).
 * calls advances by one.  size == 0: counts and masses become 0, the running
 * fields stay.  Slots outside the window are ignored whatever they hold.
 * Three small launches, no float atomics (every sum has a fixed order: equal
 * inputs give equal bits), no host synchronisation; the partials live in
 * scratch of `buf`, allocated by the first call.  Calls that share one
 * dqz_logit_buffer must be ordered on one stream. */
typedef struct dqz_census_class {
  float max_seen, min_seen;
  double probe_sum[5];
  int64_t probe_num[5];
  int64_t count;
  double mass;
} dqz_census_class;
typedef struct dqz_census {
  dqz_census_class cls[2]; /* 0 real, 1 nonsense */
  int64_t calls;
} dqz_census;
int dqz_logits_census(dqz_logit_buffer* buf, const float* logits, const uint8_t* flags, int64_t left_head,
                      int64_t size, dqz_census* acc_dev, void* stream);

/* n uniform doubles in [0,1) from Philox4x32-10 (counter advanced on device). */
int dqz_uniform_philox(uint64_t seed, uint64_t* counter_dev, int n, double* out, void* stream);

/* Priority write-back of the learner's last step (prioritized/agent.py:201-206,
 * replay.py:620-630): p = |td| (fp64 of the f32 TD errors), *max_seen_dev =
 * max(*max_seen_dev, max p), leaf[slots[i]] = p^alpha (0 -> 0) with the sum
 * tree's ancestors rebuilt (a tree index drawn twice keeps its last draw;
 * `slots` holds tree indices, dqz_per_sample's out_indices).  All
 * device pointers; one launch, no host synchronisation.  Batch <= 256. */
int dqz_per_write_back(dqz_learner* learner, double* tree, int64_t cap, const int32_t* slots, double alpha,
                       double* max_seen_dev, void* stream);

/* ---- prioritized replay: fp64 sum tree in HBM (replay.py:379-559) -------
 * tree: device f64 [2*cap], cap a power of two, node i has children 2i, 2i+1,
 * root at 1, leaves at [cap, 2cap) -- the layout of the host SumTree.
 * set: leaves idx[k] = values[k] (k < n <= 65536), ancestors recomputed as
 * left + right (bit-identical to SumTree.set).  query: SumTree._query_single
 * per target; out = -1 when target is outside [0, root). */
int dqz_sumtree_set(double* tree, int64_t cap, const int64_t* idx, const double* values, int n,
                    void* stream);
int dqz_sumtree_query(const double* tree, int64_t cap, const double* targets, int n, int64_t* out,
                      void* stream);

/* PrioritizedDistribution.sample + importance_sampling_weights on device
 * (replay.py:680-716, 344-376).  Draws: injected_u == NULL -> device Philox
 * (seed, *counter_dev; the counter is advanced), tree leaf index = replay
 * slot, uniform picks over the live window (live_base + j) mod capacity.
 * injected_u != NULL -> the caller's RandomState draws in the reference's
 * order: injected_uniform[i] = active_indices[randint(size)[i]] (a tree
 * index), injected_u[i] = uniform target fraction, injected_u[n + i] = the
 * usp-mix uniform; counter_dev is ignored.  index_to_slot (device int32
 * [cap], or NULL for identity) maps tree indices to replay slots.
 * out_indices (tree indices) and out_probs (f64) may be NULL.  n <= 1024. */
int dqz_per_sample(const double* tree, int64_t cap, int64_t live_base, int64_t size, int64_t capacity,
                   int n, double uniform_sample_probability, double importance_exponent,
                   int normalize_weights, uint64_t seed, uint64_t* counter_dev,
                   const int32_t* injected_uniform, const double* injected_u, const int32_t* index_to_slot,
                   int32_t* out_indices, int32_t* out_slots, float* out_weights, double* out_probs,
                   void* stream);

/* A whole prioritized learn (prioritized/agent.py:187-206) in one learner
 * step: the draw of dqz_per_sample (same streams: Philox (seed,
 * *counter_dev) or the caller's RandomState draws injected, same node
 * sequence, same fp64 probabilities) computed by the forward's conv1
 * workgroups, the IS weights (importance_sampling_weights, normalised by the
 * batch maximum if normalize_weights) formed by the head, the double-Q step
 * with them, and the |td|^alpha write-back inside the backward launch
 * (dqz_learner_step_per).  Outputs: out_indices (tree indices), out_slots,
 * out_probs (f64), out_weights (f32, may be NULL), all device [B].  Batch
 * <= 64, cap a power of two <= 2^24. */
typedef struct dqz_per_draw {
  double* tree;
  int64_t cap;
  int64_t live_base, size, capacity;
  double uniform_sample_probability;
  double importance_sampling_exponent;
  int normalize_weights;
  uint64_t seed;
  uint64_t* counter_dev;
  const int32_t* injected_uniform;
  const double* injected_u;
  const int32_t* index_to_slot;
  double alpha;
  double* max_seen_dev;
  int32_t* out_indices;
  int32_t* out_slots;
  double* out_probs;
  float* out_weights;
} dqz_per_draw;
int dqz_learner_step_per_draw(dqz_learner* learner, const dqz_params* params, const dqz_store* store,
                              const dqz_per_draw* draw, void* stream);

/* ---- optimizers on a finished gradient -----------------------------------
 * optax.adam, plain optax.rmsprop(centered=False) and
 * optax.clip_by_global_norm in front of either (optax 0.1.2; the chain of
 * c51/run_atari.py:210-216, qrdqn, iqn and rainbow).  Centered RMSProp is not
 * here: it is fused into dqz_learner_step's own kernels.
 *   clip_by_global_norm(c): g <- g if |g| < c else (g / |g|) c, |g| the
 *     global norm over the ten leaves (padding excluded), summed in float64 in
 *     a fixed order (equal gradients give equal bits);
 *   DQZ_OPT_ADAM (scale_by_adam, eps_root = 0; scale(-lr)):
 *     m <- b1 m + (1 - b1) g;  v <- b2 v + (1 - b2) g^2;  count <- count + 1;
 *     theta <- theta - lr (m / (1 - b1^count)) / (sqrt(v / (1 - b2^count)) + eps)
 *   DQZ_OPT_RMSPROP (scale_by_rms; scale(-lr)):
 *     nu <- decay nu + (1 - decay) g^2;  theta <- theta - lr g / sqrt(nu + eps)
 * The arithmetic is float64 inside with IEEE division and square root; theta
 * and the moments are float32, rounded once per step.  Padding of every leaf
 * is never written. */
#define DQZ_OPT_ADAM 0
#define DQZ_OPT_RMSPROP 1

typedef struct dqz_optimizer_config {
  int kind;             /* DQZ_OPT_* */
  float learning_rate;
  float b1, b2;         /* Adam (0.9, 0.999) */
  float decay;          /* RMSProp (0.9) */
  float eps;
  float max_global_grad_norm; /* <= 0: no clipping */
  int num_actions;      /* the parameter layout, as dqz_param_layout */
  int shared_bias;
} dqz_optimizer_config;

typedef struct dqz_optimizer dqz_optimizer;

/* The handle owns a gradient scratch [total] (zeroed once: the learner's
 * gradient mode leaves padding untouched) and the norm's float64 partials.
 * Calls on one handle must be ordered on one stream. */
int dqz_optimizer_create(const dqz_optimizer_config* cfg, dqz_optimizer** out);
int dqz_optimizer_destroy(dqz_optimizer* opt);

/* The optimizer on a caller-supplied gradient (device f32 [total], dqz
 * parameter layout; its padding is ignored): the norm launch when clipping,
 * then one apply launch, in place on params_online and the moments.
 *   Adam: mu = m, nu = v (device f32 [total]); count: device int32 [1]
 *     (ScaleByAdamState.count), advanced on the device exactly once, by a
 *     one-thread launch behind the apply whose workgroups read it.
 *   RMSProp: nu (ScaleByRmsState.nu); mu and count are ignored (may be NULL).
 * No host synchronisation, no allocation, capturable in a graph. */
int dqz_optimizer_apply(dqz_optimizer* opt, float* params_online, const float* grad, float* mu, float* nu,
                        int32_t* count, void* stream);

/* *gnorm (device f32 [1]) = the global norm, before clipping, of the gradient
 * of the handle's most recent step or apply.  With clipping it is a copy of
 * the value that step used; without, it is computed now from that gradient
 * (the handle's scratch after a step; after a stand-alone apply the caller's
 * buffer, which must still hold the gradient). */
int dqz_optimizer_outputs(dqz_optimizer* opt, float* gnorm, void* stream);

/* dqz_learner_step, dqz_learner_step_uniform and dqz_learner_step_per_draw
 * with one of the optimizers above in place of centered RMSProp: the same
 * step in gradient mode into the handle's scratch (forward, TD loss, health
 * word, the fused draw, the PER weights and write-back as in the plain call;
 * the learner config's learning_rate / decay / eps are unused), then
 * dqz_optimizer_apply on params->online / mu / nu and `count`.  The optimizer
 * must have the learner's num_actions and bias shape.  Same stream, no
 * allocation, capturable in a graph. */
int dqz_learner_step_opt(dqz_learner* learner, const dqz_params* params, const dqz_store* store,
                         const int32_t* slots, const float* is_weights, dqz_optimizer* opt, int32_t* count,
                         void* stream);
int dqz_learner_step_opt_uniform(dqz_learner* learner, const dqz_params* params, const dqz_store* store,
                                 int64_t base, int64_t size, int64_t capacity, uint64_t seed,
                                 uint64_t* counter_dev, int32_t* slots_out, dqz_optimizer* opt, int32_t* count,
                                 void* stream);
int dqz_learner_step_opt_per_draw(dqz_learner* learner, const dqz_params* params, const dqz_store* store,
                                  const dqz_per_draw* draw, dqz_optimizer* opt, int32_t* count, void* stream);

/* ---- the categorical (C51) agent (c51/agent.py:36-39,87-129) --------------
 * networks.c51_atari_network (networks.py:316-335): the NatureQNetwork torso
 * with a last layer A * N wide, N atoms per action on a fixed support z [N]
 * (strictly increasing; never recomputed on the device, no kernel assumes
 * equal spacing):
 *   q_logits[b, a, j] = out[b, a N + j];  q_values[b, a] = sum_j softmax_j z_j.
 * Loss (rlax 0.1.2 categorical_q_learning), per sample: P = softmax of the
 * target logits at s_t, a* = argmax_a sum_j P[a, j] z_j (first maximum),
 * p = P[a*], y_i = clip(r + d z_i, z_0, z_{N-1}), m = categorical_l2_project
 * of (y, p) onto z, loss_b = -sum_k m_k log_softmax(l)_k with l the online
 * logits of the taken action; the step's loss is the batch mean, and
 * d loss / d l_k = (softmax(l)_k - m_k) / B.  No clip_gradient, no TD error,
 * no importance weights.
 * The parameter layout is dqz_param_layout's with leaves 8 and 9 widened:
 *   8 linear_1/w [512, A N]   9 linear_1/b [A N]
 * 2 <= N <= 64 and A N <= 1024 (18 actions x 51 atoms = 918 fit). */
int dqz_c51_param_layout(int num_actions, int num_atoms, int64_t offsets[DQZ_NUM_LEAVES],
                         int64_t sizes[DQZ_NUM_LEAVES], int64_t* total);

/* dqz_optimizer_create for that layout (cfg->num_actions = A, shared_bias 0). */
int dqz_c51_optimizer_create(const dqz_optimizer_config* cfg, int num_atoms, dqz_optimizer** out);

typedef struct dqz_c51 dqz_c51;

/* A learner on the categorical layout plus the head's buffers.  cfg: batch
 * 2..256, num_actions, algo DQZ_ALGO_DQN; its optimizer fields and
 * grad_error_bound are unused.  support: device f32 [num_atoms], copied (and
 * checked on the host: this call synchronises). */
int dqz_c51_create(const dqz_learner_config* cfg, int num_atoms, const float* support, dqz_c51** out);
int dqz_c51_destroy(dqz_c51* c51);

/* The dqz_learner inside (owned by the handle): dqz_learner_sync_status and
 * dqz_learner_debug_activations apply to it; its q stays unused. */
int dqz_c51_learner(dqz_c51* c51, dqz_learner** out);

/* One jitted `update` (c51/agent.py:109-117): the learner step's forward with
 * the categorical head in place of the scalar one, its backward in gradient
 * mode into the optimizer's scratch, the fc2 gradient, then
 * dqz_optimizer_apply on params->online / mu / nu and `count`.  slots: device
 * int32 [B].  Same stream, no allocation, no host synchronisation, capturable
 * in a graph.  The learner's health word keeps its meaning (bit 1: a
 * non-finite batch loss). */
int dqz_c51_step(dqz_c51* c51, const dqz_params* params, const dqz_store* store, const int32_t* slots,
                 dqz_optimizer* opt, int32_t* count, void* stream);

/* Gradient only (jax.grad(loss_fn)) into grad_out, dqz_c51_param_layout
 * order, padding untouched; mu / nu may be NULL. */
int dqz_c51_grad(dqz_c51* c51, const dqz_params* params, const dqz_store* store, const int32_t* slots,
                 float* grad_out, void* stream);

/* Device-to-device copies of the last step's outputs (any may be NULL):
 * logits_a [B][N] online logits of the taken action, q_values [2][B][A]
 * (online at s_tm1, target at s_t), loss_b [B] per-sample loss, loss [1] their
 * mean, a_star int32 [B] the target's greedy action. */
int dqz_c51_outputs(dqz_c51* c51, float* logits_a, float* q_values, float* loss_b, float* loss,
                    int32_t* a_star, void* stream);

/* Diagnostic (tests): the last step's full logits [2][B][A N] and
 * dlogits [B][N] (either may be NULL). */
int dqz_c51_debug(dqz_c51* c51, float* logits, float* dlogits, void* stream);

/* dqz_learner_profile of the categorical step (gradient mode into grad_out):
 * phases 0, 3, 5, 6, 9 as there (9 without the fc2 leaves), 4 the logits
 * launch, 8 the per-sample loss head, 7 the fc2 gradient. */
int dqz_c51_profile(dqz_c51* c51, const dqz_params* params, const dqz_store* store, const int32_t* slots,
                    float* grad_out, int iters, float* phase_ms, void* stream);

/* q_values [n][A] of uint8 states / replay slots, and select_action
 * (c51/agent.py:121-129): dqz_forward, dqz_forward_slots and dqz_act on the
 * categorical network; out[i].value = max_a q_values. */
int dqz_c51_forward(dqz_c51* c51, const float* params, const uint8_t* states, int n, float* q_out,
                    void* stream);
int dqz_c51_forward_slots(dqz_c51* c51, const float* params, const dqz_store* store, const int32_t* slots,
                          int n, int which, float* q_out, void* stream);
int dqz_c51_act(dqz_c51* c51, const float* params, const uint8_t* states, int n, double epsilon,
                uint64_t seed, uint64_t counter, dqz_action* out, void* stream);

/* Diagnostic (tests): what the learner step checks of a categorical request,
 * on host structures only (no device call): a request on `slots` in gradient
 * mode at batch `batch`, plus the modes named by `request`; returns the
 * step's own status and message. */
#define DQZ_C51_REQ_WEIGHTS 1u        /* PER importance weights */
#define DQZ_C51_REQ_PER_DRAW 2u       /* the fused prioritized draw */
#define DQZ_C51_REQ_UNIFORM_DRAW 4u   /* in-launch draws */
#define DQZ_C51_REQ_LOGIT_DRAW 8u
#define DQZ_C51_REQ_EXACT_DRAW 16u
#define DQZ_C51_REQ_META_P 32u        /* MGSC meta modes */
#define DQZ_C51_REQ_META_EPI 64u
#define DQZ_C51_REQ_META_SOFTMAX 128u
#define DQZ_C51_REQ_UNIT 256u         /* the HVP's unit cotangent */
#define DQZ_C51_REQ_WRITE_BACK 512u   /* the fused PER write-back */
#define DQZ_C51_REQ_FUSED_RMSPROP 1024u /* no gradient output: the fused centered RMSProp */
int dqz_c51_debug_check(int batch, unsigned request);

/* ---- double-Q selection and importance weights on the wide heads ----------
 * Rainbow's learning rule (rainbow/agent.py:85-150,198:
 * rlax.categorical_double_q_learning, the loss weighted by the replay's
 * importance weights, the clipped loss as the new priority) on the C51 and the
 * QR-DQN networks, switched on when the head is created.
 *   double_q  the forward runs a third copy, online parameters at s_t, and
 *             a* = argmax_a q_values of that copy (first maximum).  The
 *             categorical head then uses p = softmax(target logits)[a*], the
 *             quantile head t_j = r + d x_target[j, a*]; nothing else in either
 *             loss changes and no gradient flows through the third copy.
 *             q_values is then [3][B][A]: dqz_*_outputs keeps returning the
 *             first two blocks and a_star is the selector's choice;
 *             dqz_*_debug returns the outputs of all three copies.
 *   weighted  every step takes is_weights w [B] (the _w entries; the plain
 *             step, grad and profile entries are refused, as a head without it
 *             refuses the _w ones): loss = mean_b(w_b loss_b), d loss / d (taken
 *             outputs) is the plain cotangent times w_b (a weight of exactly 0
 *             gives +0.0 in every element), loss_b stays unweighted.  The head
 *             also writes clip(|loss_b|, 0, 100) into the inner learner's TD
 *             buffer, so dqz_per_write_back on the handle from dqz_c51_learner /
 *             dqz_qr_learner writes the new priorities and the running maximum
 *             into the device sum tree.  The reference has no prioritized
 *             QR-DQN: the quantile priority is this library's definition,
 *             Rainbow's rule applied to the quantile loss.
 * A head with options still refuses, in the plain heads' words: the fused
 * prioritized draw, every in-launch draw, the fused write-back, the MGSC
 * modes, the unit cotangent, fused centered RMSProp and batch 1.  cfg->algo
 * stays DQZ_ALGO_DQN: double_q makes the inner learner the three-copy one. */
typedef struct dqz_wide_options {
  int double_q; /* 0 or 1 */
  int weighted; /* 0 or 1 */
} dqz_wide_options;

/* dqz_c51_create with options (non-null); {0, 0} is dqz_c51_create. */
int dqz_c51_create_opt(const dqz_learner_config* cfg, int num_atoms, const float* support,
                       const dqz_wide_options* options, dqz_c51** out);
/* dqz_c51_step / _grad / _profile of a weighted head: is_weights device f32
 * [B], refused before any device call when null. */
int dqz_c51_step_w(dqz_c51* c51, const dqz_params* params, const dqz_store* store, const int32_t* slots,
                   const float* is_weights, dqz_optimizer* opt, int32_t* count, void* stream);
int dqz_c51_grad_w(dqz_c51* c51, const dqz_params* params, const dqz_store* store, const int32_t* slots,
                   const float* is_weights, float* grad_out, void* stream);
int dqz_c51_profile_w(dqz_c51* c51, const dqz_params* params, const dqz_store* store, const int32_t* slots,
                      const float* is_weights, float* grad_out, int iters, float* phase_ms, void* stream);
/* What the options add to dqz_c51_outputs (either may be NULL): q_selector
 * [B][A], the third copy's q_values (double_q heads only); priorities [B],
 * clip(|loss_b|, 0, 100) (weighted heads only). */
int dqz_c51_outputs_opt(dqz_c51* c51, float* q_selector, float* priorities, void* stream);
/* dqz_c51_debug_check for a head created with `options`. */
int dqz_c51_debug_check_opt(int batch, unsigned request, const dqz_wide_options* options);

/* ---- the Rainbow agent (rainbow/agent.py; networks.py rainbow_atari_network) --
 * The categorical head with double_q and weighted both set, behind a noisy
 * dueling network.  x = flatten(conv3) [B, 3136] (post-ReLU), then
 *   noisy(x) = x Wmu + bmu + ((e_in * x) Wsig + bsig) * e_out
 *   h_adv = relu(noisy_A1(x))   adv = noisy_A2(h_adv)  [A N], mu without a bias
 *   h_val = relu(noisy_V1(x))   val = noisy_V2(h_val)  [N],   mu without a bias
 *   q_logits[b, a, n] = val[b, n] + adv[b, a, n] - mean_a' adv[b, a', n].
 * The noise comes from the caller: one application of the network reads one
 * vector of dqz_rainbow_noise_len(A, N) = 8320 + A N + N floats, in the order
 *   A1_in 3136 | A1_out 512 | A2_in 512 | A2_out A N | V1_in 3136 | V1_out 512 |
 *   V2_in 512 | V2_out N,
 * and a learner step three of them, [3][noise_len]: online(s_tm1) (the only
 * differentiated application), target(s_t), online(s_t) (the selector).  No
 * entry but dqz_rainbow_noise draws noise, so equal noise gives equal bits.
 * Parameter layout, DQZ_RAINBOW_NUM_LEAVES leaves, each padded to 64 floats:
 *   0-5 the conv leaves   6 A1 mu/w [3136,512]  7 A1 mu/b [512]
 *   8 A1 sigma/w  9 A1 sigma/b  10 A2 mu/w [512, A N]  11 A2 sigma/w  12 A2 sigma/b [A N]
 *   13 V1 mu/w  14 V1 mu/b  15 V1 sigma/w  16 V1 sigma/b  17 V2 mu/w [512, N]
 *   18 V2 sigma/w  19 V2 sigma/b [N].
 * Limits are the categorical head's: batch 2..256, A 1..32, N 2..64, A N <=
 * 1024.  The step is always double-Q and weighted and runs in gradient mode
 * followed by the optimizer; it refuses, in the wide heads' words, every
 * in-launch draw, the fused prioritized draw, the fused write-back, the MGSC
 * modes, the unit cotangent and fused centered RMSProp. */
#define DQZ_RAINBOW_NUM_LEAVES 20
typedef struct dqz_rainbow dqz_rainbow;
int dqz_rainbow_param_layout(int num_actions, int num_atoms, int64_t offsets[DQZ_RAINBOW_NUM_LEAVES],
                             int64_t sizes[DQZ_RAINBOW_NUM_LEAVES], int64_t* total);
int dqz_rainbow_noise_len(int num_actions, int num_atoms, int* out);
/* out[i] = sign(t) sqrt|t|, t = sqrt(2) erfinv(lo + u_i (hi - lo)), lo / hi =
 * erf(-/+ sqrt(2)) (a standard normal truncated to [-2, 2]) and u_i the i-th
 * uniform dqz_uniform_philox(seed, counter) gives; *counter_dev += n on device.
 * 1 <= n <= 65536; out device f32 [n]. */
int dqz_rainbow_noise(uint64_t seed, uint64_t* counter_dev, int n, float* out, void* stream);
int dqz_rainbow_optimizer_create(const dqz_optimizer_config* cfg, int num_atoms, dqz_optimizer** out);
/* options: NULL or {1, 1}; anything else is refused (there is no plain Rainbow). */
int dqz_rainbow_create(const dqz_learner_config* cfg, int num_atoms, const float* support,
                       const dqz_wide_options* options, dqz_rainbow** out);
int dqz_rainbow_destroy(dqz_rainbow* rb);
int dqz_rainbow_learner(dqz_rainbow* rb, dqz_learner** out);
/* is_weights: device f32 [B]; noise: device f32 [3][noise_len]; both refused
 * before any device call when null. */
int dqz_rainbow_step(dqz_rainbow* rb, const dqz_params* params, const dqz_store* store, const int32_t* slots,
                     const float* is_weights, const float* noise, dqz_optimizer* opt, int32_t* count, void* stream);
int dqz_rainbow_grad(dqz_rainbow* rb, const dqz_params* params, const dqz_store* store, const int32_t* slots,
                     const float* is_weights, const float* noise, float* grad_out, void* stream);
int dqz_rainbow_profile(dqz_rainbow* rb, const dqz_params* params, const dqz_store* store, const int32_t* slots,
                        const float* is_weights, const float* noise, float* grad_out, int iters, float* phase_ms,
                        void* stream);
/* dqz_c51_outputs / dqz_c51_outputs_opt / dqz_c51_debug of the step's head. */
int dqz_rainbow_outputs(dqz_rainbow* rb, float* logits_a, float* q_values, float* loss_b, float* loss,
                        int32_t* a_star, void* stream);
int dqz_rainbow_outputs_opt(dqz_rainbow* rb, float* q_selector, float* priorities, void* stream);
int dqz_rainbow_debug_head(dqz_rainbow* rb, float* q_logits, float* dlogits, void* stream);
/* Diagnostic: application 0's h_adv, h_val [B][512], adv [B][A N], val [B][N]
 * and dz_adv, dz_val [B][512] of the last step (any may be NULL). */
int dqz_rainbow_debug(dqz_rainbow* rb, float* h_adv, float* h_val, float* adv, float* val, float* dz_adv,
                      float* dz_val, void* stream);
/* q_values [n][A] of one application (noise [noise_len]); act: the argmax and
 * v_t = max_a q per state, no epsilon (states and out may be pinned host memory). */
int dqz_rainbow_forward(dqz_rainbow* rb, const float* params, const uint8_t* states, int n, const float* noise,
                        float* q_out, void* stream);
int dqz_rainbow_forward_slots(dqz_rainbow* rb, const float* params, const dqz_store* store, const int32_t* slots,
                              int n, int which, const float* noise, float* q_out, void* stream);
int dqz_rainbow_act(dqz_rainbow* rb, const float* params, const uint8_t* states, int n, const float* noise,
                    dqz_action* out, void* stream);
/* dqz_c51_debug_check for a Rainbow request (DQZ_C51_REQ_* bits).  No device call. */
int dqz_rainbow_debug_check(int batch, unsigned request);

/* ---- the quantile (QR-DQN) agent (qrdqn/agent.py:36-39,88-134) ------------
 * networks.qr_atari_network (networks.py:295-313): the NatureQNetwork torso
 * with a last layer N * A wide, N quantile values per action, quantile-major:
 *   q_dist[b, i, a] = out[b, i A + a];  q_values[b, a] = mean_i q_dist[b, i, a].
 * Loss (rlax 0.1.2 quantile_q_learning with dist_q_t_selector = dist_q_t: no
 * double-Q), per sample, x_o = online(s_tm1), x_t = target(s_t):
 *   a* = argmax_a mean_j x_t[j, a] (first maximum), theta_i = x_o[i, a_b],
 *   t_j = r + d x_t[j, a*], delta_ij = t_j - theta_i,
 *   w_ij = |tau_i - 1[delta_ij < 0]|,
 *   H_k(x) = 0.5 min(|x|, k)^2 + k (|x| - min(|x|, k)),
 *   loss_b = sum_i (1/N) sum_j w_ij H_k(delta_ij);
 * the step's loss is the batch mean, and
 *   d loss / d x_o[b, i, a_b] = -(1 / (N B)) sum_j w_ij clip(delta_ij, -k, k).
 * k = huber_param > 0 only: huber_param = 0 (rlax's plain |delta| branch) is
 * refused.  No clip_gradient, no importance weights.
 * The parameter layout is dqz_param_layout's with leaves 8 and 9 widened:
 *   8 linear_1/w [512, N A]   9 linear_1/b [N A]
 * 1 <= N <= 256 and A N <= 4096 (18 actions x 201 quantiles = 3618 fit). */
int dqz_qr_param_layout(int num_actions, int num_quantiles, int64_t offsets[DQZ_NUM_LEAVES],
                        int64_t sizes[DQZ_NUM_LEAVES], int64_t* total);

/* dqz_optimizer_create for that layout (cfg->num_actions = A, shared_bias 0). */
int dqz_qr_optimizer_create(const dqz_optimizer_config* cfg, int num_quantiles, dqz_optimizer** out);

typedef struct dqz_qr dqz_qr;

/* A learner on the quantile layout plus the head's buffers (one implementation
 * stands behind this handle type and dqz_c51; the two types keep a handle of
 * one kind out of the other's entries).  cfg: batch
 * 2..256, num_actions, algo DQZ_ALGO_DQN; its optimizer fields and
 * grad_error_bound are unused.  quantiles: device f32 [num_quantiles], copied
 * and checked on the host (this call synchronises): each finite and strictly
 * inside (0, 1), huber_param finite and > 0; a refusal names the index. */
int dqz_qr_create(const dqz_learner_config* cfg, int num_quantiles, const float* quantiles, float huber_param,
                  dqz_qr** out);
int dqz_qr_destroy(dqz_qr* qr);

/* The dqz_learner inside (owned by the handle): dqz_learner_sync_status and
 * dqz_learner_debug_activations apply to it; its q stays unused. */
int dqz_qr_learner(dqz_qr* qr, dqz_learner** out);

/* One jitted `update` (qrdqn/agent.py:112-120): the learner step's forward
 * with the quantile head in place of the scalar one, its backward in gradient
 * mode into the optimizer's scratch, the fc2 gradient, then
 * dqz_optimizer_apply on params->online / mu / nu and `count`.  slots: device
 * int32 [B].  Same stream, no allocation, no host synchronisation, capturable
 * in a graph.  The learner's health word keeps its meaning. */
int dqz_qr_step(dqz_qr* qr, const dqz_params* params, const dqz_store* store, const int32_t* slots,
                dqz_optimizer* opt, int32_t* count, void* stream);

/* Gradient only (jax.grad(loss_fn)) into grad_out, dqz_qr_param_layout order,
 * padding untouched; mu / nu may be NULL. */
int dqz_qr_grad(dqz_qr* qr, const dqz_params* params, const dqz_store* store, const int32_t* slots,
                float* grad_out, void* stream);

/* Device-to-device copies of the last step's outputs (any may be NULL):
 * theta [B][N] online outputs of the taken action, q_values [2][B][A] (online
 * at s_tm1, target at s_t), loss_b [B] per-sample loss, loss [1] their mean,
 * a_star int32 [B] the target's greedy action. */
int dqz_qr_outputs(dqz_qr* qr, float* theta, float* q_values, float* loss_b, float* loss, int32_t* a_star,
                   void* stream);

/* Diagnostic (tests): the last step's full outputs [2][B][N][A] and
 * dtheta [B][N] (either may be NULL). */
int dqz_qr_debug(dqz_qr* qr, float* outputs, float* dtheta, void* stream);

/* dqz_learner_profile of the quantile step (gradient mode into grad_out):
 * phases 0, 3, 5, 6, 9 as there (9 without the fc2 leaves), 4 the outputs
 * launch, 8 the per-sample loss head, 2 the batched dz1 product, 7 the fc2
 * gradient. */
int dqz_qr_profile(dqz_qr* qr, const dqz_params* params, const dqz_store* store, const int32_t* slots,
                   float* grad_out, int iters, float* phase_ms, void* stream);

/* q_values [n][A] of uint8 states / replay slots, and select_action
 * (qrdqn/agent.py:122-134): dqz_forward, dqz_forward_slots and dqz_act on the
 * quantile network; out[i].value = max_a q_values. */
int dqz_qr_forward(dqz_qr* qr, const float* params, const uint8_t* states, int n, float* q_out, void* stream);
int dqz_qr_forward_slots(dqz_qr* qr, const float* params, const dqz_store* store, const int32_t* slots, int n,
                         int which, float* q_out, void* stream);
int dqz_qr_act(dqz_qr* qr, const float* params, const uint8_t* states, int n, double epsilon, uint64_t seed,
               uint64_t counter, dqz_action* out, void* stream);

/* Diagnostic (tests): dqz_c51_debug_check for a quantile request; `request`
 * takes the DQZ_C51_REQ_* bits.  No device call. */
int dqz_qr_debug_check(int batch, unsigned request);

/* The quantile head with dqz_wide_options (above, at the categorical head's):
 * the same entries, the same refusals. */
int dqz_qr_create_opt(const dqz_learner_config* cfg, int num_quantiles, const float* quantiles, float huber_param,
                      const dqz_wide_options* options, dqz_qr** out);
int dqz_qr_step_w(dqz_qr* qr, const dqz_params* params, const dqz_store* store, const int32_t* slots,
                  const float* is_weights, dqz_optimizer* opt, int32_t* count, void* stream);
int dqz_qr_grad_w(dqz_qr* qr, const dqz_params* params, const dqz_store* store, const int32_t* slots,
                  const float* is_weights, float* grad_out, void* stream);
int dqz_qr_profile_w(dqz_qr* qr, const dqz_params* params, const dqz_store* store, const int32_t* slots,
                     const float* is_weights, float* grad_out, int iters, float* phase_ms, void* stream);
int dqz_qr_outputs_opt(dqz_qr* qr, float* q_selector, float* priorities, void* stream);
int dqz_qr_debug_check_opt(int batch, unsigned request, const dqz_wide_options* options);

/* PrioritizedTransitionReplay.add on device (replay.py:1068-1096 ->
 * PrioritizedDistribution.remove_priorities / add_priorities, :642-678): the
 * evicted tree index remove_index (-1: none) is set to 0, add_index to
 * _power(priority, alpha) -- priority < 0 reads the agent's running
 * max_seen_priority from max_seen_dev (prioritized/agent.py:155) -- and
 * index_to_slot[add_index] = slot.  One launch, no host synchronisation. */
int dqz_per_add(double* tree, int64_t cap, int32_t remove_index, int32_t add_index, double priority,
                const double* max_seen_dev, double alpha, int32_t* index_to_slot, int32_t slot, void* stream);

/* Target sync: target <- online (dqn/agent.py:155-156; hard copy, not Polyak). */
int dqz_target_copy(float* target, const float* online, int64_t total, void* stream);

/* ---- MGSC meta-update (dqn_mgsc_batched/agent.py:104-220) -------------- */

typedef struct dqz_meta_config {
  int meta_batch;          /* M (meta_batch_size, run_atari.py:101), any size: batches past 256 run in chunks */
  int num_actions;         /* A; the network is dqn_atari_network (per-action bias) */
  float learning_rate;     /* inner optax.rmsprop(centered) lr, run_atari.py:218-223 */
  float decay;             /* 0.95 */
  float eps;               /* optimizer_epsilon */
  float grad_error_bound;  /* rlax.clip_gradient bound */
  float meta_learning_rate; /* optax.adam lr, run_atari.py:241-243 */
  float b1, b2, meta_eps;  /* optax.adam defaults 0.9, 0.999, 1e-8 */
  int second_order;        /* 0: theta'' = stop_gradient(...) (dqn_mgsc_batched/agent.py:191);
                              1: no stop_gradient (dqn_mgsc_batched_reservoir/agent.py):
                              d theta''/d theta' through the online transition's Hessian */
} dqz_meta_config;

typedef struct dqz_meta dqz_meta;

int dqz_meta_create(const dqz_meta_config* cfg, dqz_meta** out);
int dqz_meta_destroy(dqz_meta* meta);

/* One jitted `meta_update` + `replay.update_priorities` (agent.py:211-220,
 * 302-334); written for the stop-gradient variant, cfg.second_order adds the
 * reservoir variant's d theta''/d theta' term (Hessian-vector product):
 *   p = softmax(logits[pos]) (replay_circular.py:79-86); G = sum_i p_i g_i
 *   (per-transition grads of loss_fn, agent.py:152-172); theta' = theta +
 *   RMSProp(G; mu, nu); g' = grad loss_fn(theta', target=theta, online
 *   transition); theta'' = stop_grad(theta' + RMSProp(g'; mu', nu'));
 *   L = sum |theta' - theta''|^2; Adam on the M logits, written back to
 *   logits[pos[i]].
 * params: online / target / mu / nu are read only (the agent's opt_state is
 * not advanced by meta_update).  slots: device int32 [M] meta-batch replay
 * slots in `store`.  online_store/online_slot: the newest transition (device
 * int32 [1]).  logits: the replay's device logit buffer; pos: device int32
 * [M] absolute positions (distinct).  adam_mu/adam_nu: device f32 [M];
 * adam_count: device int32 [1] (ScaleByAdamState).  logit_buf (may be
 * NULL): the dqz_logit_buffer owning `logits`; its running log-sum-exp is
 * then updated for the M writes (positions distinct), so the buffer's next
 * add / sample needs no re-scan; with NULL the caller must call
 * dqz_logits_invalidate. */
int dqz_meta_update(dqz_meta* meta, const dqz_params* params, const dqz_store* store,
                    const int32_t* slots, const dqz_store* online_store, const int32_t* online_slot,
                    float* logits, const int32_t* pos, float* adam_mu, float* adam_nu,
                    int32_t* adam_count, dqz_logit_buffer* logit_buf, void* stream);

/* Device copies of the last meta-update's intermediates (any may be NULL):
 * probs [M], dlogits [M] (d L / d logits), td [M] meta-batch TD errors,
 * loss [1] = sum |theta' - theta''|^2. */
int dqz_meta_outputs(dqz_meta* meta, float* probs, float* dlogits, float* td, float* loss,
                     void* stream);

/* Health word of the meta-update since the previous check (the meta-level
 * counterpart of dqz_learner_sync_status): the OR of the batch learner's
 * and the one-transition learner's words (bit 0: an in-launch hand-off wait
 * gave up, among them the HVP's ddot1 wait; bit 1: a non-finite loss) and of
 * the meta-update's own word (bit 0: the fused Adam leader's wait for the
 * other chunk blocks gave up).  Synchronises the device.  A non-zero status
 * clears every hand-off word of the meta handle (both learners' and its own
 * arrival counters) and the status; callers treat the meta-updates since
 * their previous check as invalid. */
int dqz_meta_sync_status(dqz_meta* meta, int* status);

/* Diagnostic (tests): from the next meta-update on, every bounded wait of the
 * meta handle gives up after `spin_max` polls (0 restores 2^24); poison != 0
 * sets the HVP's ddot1 arrival counter far below its arrivals (second order)
 * and the Adam entry counter far below M, so the next update's waits on them
 * run out — the timeout path of dqz_meta_sync_status, exercised.
 * Synchronises the device. */
int dqz_meta_debug_stall(dqz_meta* meta, int poison, unsigned spin_max);

/* Diagnostic (tests): a borrowed handle of one of the meta handle's two
 * learners (owned by `meta`, never destroyed by the caller), after the
 * precedent of dqz_c51_learner.  which = 0: the batch learner (B = min(M,
 * 256)), which holds the last chunk's forward, its p-weighted backward
 * signals (dz1 .. dy1 already carry p_i) and td.  which = 1: the
 * one-transition learner (B = 1) at theta' (copy 0 = theta'(s_tm1), copy 1 =
 * theta(s_t)): y1 .. h1, td' and, after a second-order update, the
 * unit-cotangent backward signals d4 .. d1 of q[a] (first order: those of the
 * loss).  dqz_learner_debug_activations and dqz_learner_outputs apply. */
int dqz_meta_debug_learner(dqz_meta* meta, int which, dqz_learner** out);

/* The stage buffers dqz_meta_debug_stages copies out (device pointers, any
 * may be NULL).  T = the parameter count of dqz_param_layout (padded total),
 * C = min(M, 256) the chunk size, K = ceil(M / C) the chunk count.  What each
 * holds after an update:
 *   first order   G: v = dL/dG = -2 u' J (G itself is not kept); thp, mu1,
 *                 nu1: theta', mu', nu'; J: du/dG.
 *   second order  G: G = sum_i p_i g_i; thp: theta'; J; mu1: v_dir; nu1: w
 *                 (the HVP's tangent); GQ: grad q[a] at theta'; HQ: v =
 *                 v_dir + J (alpha s1 grad q - clip(td') H_q w).
 *   K > 1         the batch learner and zv1 .. zvp hold the last chunk only.
 * GQ .. s1 exist only in a second-order handle and zv1 .. zvp are written
 * only when K > 1: asking for one the configuration does not have is refused
 * (DQZ_ERR_INVALID). */
#define DQZ_META_ZVP_PARTS 7  /* fc1 split-K partials of the tangent forward */
#define DQZ_META_HPART_CHUNKS 196  /* K-chunks of the HVP's fc1 tangent */
typedef struct dqz_meta_stages {
  float *G, *thp, *mu1, *nu1, *J; /* [T] each, parameter layout */
  float *GQ, *HQ;                 /* [T] each (second order) */
  /* the HVP's tangents of the one transition (second order), ReLU masks
   * applied: forward ty1 [400][32], ty2 [81][64], ty3 [3136]; hpart
   * [DQZ_META_HPART_CHUNKS][512], whose sum over the chunks is the fc1
   * tangent pre-activation without its bias; backward td4 [512], td3 [3136],
   * td2 [81][64], td1 [400][32] */
  float *ty1, *ty2, *ty3, *hpart, *td4, *td3, *td2, *td1;
  float *s1;                      /* [1] grad q . w (second order) */
  float *p, *s;                   /* [K C]: p = softmax(logits[pos]), 0 past M; s_i = p_i v . g_i (K > 1: 0 past M) */
  /* K > 1, last chunk: the tangent forward V y + vb of the batch learner's
   * activations, zv1 [C][400][32], zv2 [C][81][64], zv3 [C][3136], and the
   * fc1 partials zvp [DQZ_META_ZVP_PARTS][C][512] (no bias) */
  float *zv1, *zv2, *zv3, *zvp;
} dqz_meta_stages;

/* Diagnostic (tests): device-to-device copies of the last meta-update's stage
 * buffers, ordered on `stream`; no kernel is launched and nothing the next
 * update reads is written. */
int dqz_meta_debug_stages(dqz_meta* meta, const dqz_meta_stages* out, void* stream);

/* ---- Atari observation preprocessing (processors.py:421-505) -----------
 * The observation branch of processors.atari on device: element-wise max of
 * the last n RGB frames (np.max over the pooled frames), rgb2y
 * (processors.py:367-371, numpy's float64 evaluation, truncated to uint8)
 * and PIL's BILINEAR resize (processors.py:374-387; Pillow's 8-bit
 * fixed-point two-pass resampler), in one launch.  A dqz_frame_plan holds
 * the resize coefficient tables of one (in_h, in_w) -> (out_h, out_w). */
typedef struct dqz_frame_plan dqz_frame_plan;
int dqz_frame_plan_create(int in_h, int in_w, int out_h, int out_w, dqz_frame_plan** out);
int dqz_frame_plan_destroy(dqz_frame_plan* plan);
/* rgb: n frames uint8 [n][in_h][in_w][3], contiguous; out: uint8
 * [out_h][out_w].  Either may be device memory or pinned host memory. */
int dqz_atari_frame(const dqz_frame_plan* plan, const uint8_t* rgb, int n, uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* DQZ_H_ */
