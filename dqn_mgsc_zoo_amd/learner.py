"""Device learner: owns params / optimizer state and drives libdqz.

`Learner.step(store, slots)` is the jitted `update` of the reference
(dqn/agent.py:109-119, double_q/agent.py, prioritized/agent.py:115-127):
forward of online(s_tm1) and target(s_t) [and online(s_t)], TD loss with
clip_gradient, backward and the optimizer, in place: centered RMSProp fused
into the step (the default), or Adam / plain RMSProp, optionally behind
clip_by_global_norm, applied to the step's finished gradient.  Everything runs in
libdqz.so on the current HIP stream; there is no host fallback.
"""

import ctypes

import numpy as np
import torch

from dqn_mgsc_zoo_amd import _native
from dqn_mgsc_zoo_amd import networks as networks_lib
from dqn_mgsc_zoo_amd import optim_state

ALGOS = {'dqn': _native.ALGO_DQN, 'double': _native.ALGO_DOUBLE,
         'per': _native.ALGO_PER}


class RMSPropConfig:
  """optax.rmsprop(learning_rate, decay, eps, centered) stand-in.

  centered=True (dqn/run_atari.py:208-213) is fused into the learner step's
  kernels; centered=False (scale_by_rms: nu only, eps inside the root) is
  applied to the finished gradient by dqz_optimizer_apply."""

  def __init__(self, learning_rate, decay=0.9, eps=1e-8, centered=False):
    self.learning_rate = float(learning_rate)
    self.decay = float(decay)
    self.eps = float(eps)
    self.centered = bool(centered)


def rmsprop(learning_rate, decay=0.9, eps=1e-8, centered=False):
  return RMSPropConfig(learning_rate, decay, eps, centered)


class AdamConfig:
  """optax.adam(learning_rate, b1, b2, eps) stand-in (eps_root = 0)."""

  def __init__(self, learning_rate, b1=0.9, b2=0.999, eps=1e-8, eps_root=0.0):
    if eps_root != 0.0:
      raise NotImplementedError('eps_root is not used by the reference')
    self.learning_rate = float(learning_rate)
    self.b1 = float(b1)
    self.b2 = float(b2)
    self.eps = float(eps)


def adam(learning_rate, b1=0.9, b2=0.999, eps=1e-8, eps_root=0.0):
  return AdamConfig(learning_rate, b1, b2, eps, eps_root)


class ClipByGlobalNorm:
  """optax.clip_by_global_norm(max_norm) stand-in: the first stage of a chain."""

  def __init__(self, max_norm):
    self.max_norm = float(max_norm)
    if not self.max_norm > 0.0:
      raise ValueError('max_norm must be positive')


def clip_by_global_norm(max_norm):
  return ClipByGlobalNorm(max_norm)


class Chain:
  """optax.chain(clip_by_global_norm(c), optimizer) stand-in
  (c51/run_atari.py:210-216): the only chain the device applies."""

  def __init__(self, clip, optimizer):
    self.clip = clip
    self.optimizer = optimizer
    self.learning_rate = optimizer.learning_rate


def chain(*transforms):
  if (len(transforms) != 2 or not isinstance(transforms[0], ClipByGlobalNorm)
      or not isinstance(transforms[1], (AdamConfig, RMSPropConfig))):
    raise NotImplementedError(
        'only chain(clip_by_global_norm(c), adam(...) | rmsprop(...)) is '
        'supported')
  if getattr(transforms[1], 'centered', False):
    raise NotImplementedError(
        'centered RMSProp is fused into the learner step and cannot follow a '
        'gradient clip; use adam or rmsprop(centered=False)')
  return Chain(*transforms)


def split_optimizer(optimizer):
  """(max_norm or None, AdamConfig | RMSPropConfig) of an accepted optimizer."""
  if isinstance(optimizer, Chain):
    return optimizer.clip.max_norm, optimizer.optimizer
  if isinstance(optimizer, (AdamConfig, RMSPropConfig)):
    return None, optimizer
  raise NotImplementedError(
      'optimizer must be rmsprop(...), adam(...) or chain(clip_by_global_norm'
      '(c), one of them); got %r' % (optimizer,))


def is_centered_rmsprop(optimizer):
  """True for the fused default (what the MGSC meta-gradient differentiates)."""
  return isinstance(optimizer, RMSPropConfig) and optimizer.centered


class Learner:
  """Online/target params + optimizer moments in HBM and a libdqz handle."""

  _h = None  # dqz_learner handle
  _opt_h = None  # dqz_optimizer handle; None: centered RMSProp, fused into the step
  _act_in = None  # act()'s pinned input buffer, set up with the output's on its first call
  # The handle that owns the native state (an attribute's name) and the entries
  # that take it: what a subclass with another head names anew.
  _OWNER = '_h'
  _ENTRIES = dict(destroy='dqz_learner_destroy', forward='dqz_forward',
                  forward_slots='dqz_forward_slots', act='dqz_act')

  def __init__(self, network: networks_lib.NetworkSpec, batch_size, algo='dqn',
               optimizer=None, grad_error_bound=1.0 / 32, device='cuda'):
    if algo not in ALGOS:
      raise ValueError('algo must be one of %s' % sorted(ALGOS))
    if (algo == 'dqn') == network.shared_bias:
      raise ValueError(
          "algo 'dqn' uses dqn_atari_network; 'double'/'per' use "
          'double_dqn_atari_network (shared bias)')
    self.algo = algo
    self.grad_error_bound = float(grad_error_bound)
    self._alloc_state(network, batch_size,
                      optimizer or rmsprop(2.5e-4, 0.95, 0.01 / 32**2, True), device)
    self.q_tm1 = torch.zeros((self.batch_size, network.num_actions),
                             dtype=torch.float32, device=self.device)
    self.td = torch.zeros((self.batch_size,), dtype=torch.float32, device=self.device)
    self.loss = torch.zeros((1,), dtype=torch.float32, device=self.device)
    handle = ctypes.c_void_p()
    _native.check(_native.lib().dqz_learner_create(
        ctypes.byref(self._learner_config(ALGOS[algo])), ctypes.byref(handle)))
    self._h = handle
    # Adam / plain RMSProp / a clipped chain: the step runs in gradient mode
    # and dqz_optimizer_apply follows it (centered RMSProp stays fused).
    if not is_centered_rmsprop(self.optimizer):
      self._opt_h = self._create_optimizer(_native.lib().dqz_optimizer_create)

  def _alloc_state(self, network, batch_size, optimizer, device):
    """The flat state every head shares: parameters, moments, the step count
    and their dqz_params, with the optimizer split into clip and base."""
    self.network = network
    self.batch_size = int(batch_size)
    self.optimizer = optimizer
    self.clip_norm, self.base_optimizer = split_optimizer(optimizer)
    self.device = torch.device(device)
    self.offsets, self.sizes, self.total = network.layout()
    self.online = torch.zeros((self.total,), dtype=torch.float32, device=self.device)
    self.target = torch.zeros_like(self.online)
    self.mu = torch.zeros_like(self.online)
    self.nu = torch.zeros_like(self.online)
    self.count = torch.zeros((1,), dtype=torch.int32, device=self.device)
    self._gnorm = torch.zeros((1,), dtype=torch.float32, device=self.device)
    self._params_c = _native.DqzParams(
        self.online.data_ptr(), self.target.data_ptr(), self.mu.data_ptr(),
        self.nu.data_ptr())

  def _learner_config(self, algo_id):
    base = self.base_optimizer
    return _native.DqzLearnerConfig(
        self.batch_size, self.network.num_actions, algo_id, base.learning_rate,
        getattr(base, 'decay', 0.0), base.eps, self.grad_error_bound)

  def _create_optimizer(self, create, *layout_args):
    """A dqz_optimizer for (base optimizer, clip norm, network) from the
    head's create function: create(config, *layout_args, out)."""
    base = self.base_optimizer
    ocfg = _native.DqzOptimizerConfig(
        _native.OPT_ADAM if isinstance(base, AdamConfig) else _native.OPT_RMSPROP,
        base.learning_rate, getattr(base, 'b1', 0.0), getattr(base, 'b2', 0.0),
        getattr(base, 'decay', 0.0), base.eps,
        self.clip_norm if self.clip_norm is not None else 0.0,
        self.network.num_actions, int(bool(self.network.shared_bias)))
    oh = ctypes.c_void_p()
    _native.check(create(ctypes.byref(ocfg), *layout_args, ctypes.byref(oh)))
    return oh

  def _entry(self, entry):
    """The head's own `entry` (_ENTRIES) of the library."""
    return getattr(_native.lib(), self._ENTRIES[entry])

  def _call(self, entry, *args):
    """That entry on the handle that owns the state."""
    return self._entry(entry)(getattr(self, self._OWNER), *args)

  def __del__(self):
    if _native is None or _native._lib is None:  # pylint: disable=protected-access
      return
    h = getattr(self, self._OWNER)
    if h is not None and h.value:
      self._call('destroy')
      setattr(self, self._OWNER, None)
      self._h = None
    if self._opt_h is not None and self._opt_h.value:
      _native.lib().dqz_optimizer_destroy(self._opt_h)
      self._opt_h = None

  # -- state -------------------------------------------------------------

  def set_params(self, tree, target_tree=None):
    flat = torch.from_numpy(self.network.flatten(tree))
    self.online.copy_(flat)
    if target_tree is None:
      self.target.copy_(flat)
    else:
      self.target.copy_(torch.from_numpy(self.network.flatten(target_tree)))

  def set_opt_state(self, mu_tree, nu_tree):
    self.mu.copy_(torch.from_numpy(self.network.flatten(mu_tree)))
    self.nu.copy_(torch.from_numpy(self.network.flatten(nu_tree)))

  def opt_state(self):
    """The optimizer's state in optax's shape (optim_state), host arrays."""
    base = self.base_optimizer
    if isinstance(base, AdamConfig):
      inner = optim_state.adam_state(int(self.count.item()),
                                     self.params_tree('mu'),
                                     self.params_tree('nu'))
    elif base.centered:
      inner = optim_state.rmsprop_state(self.params_tree('mu'),
                                        self.params_tree('nu'))
    else:
      inner = optim_state.rms_state(self.params_tree('nu'))
    return inner if self.clip_norm is None else optim_state.chained_state(inner)

  def load_opt_state(self, state):
    """Restores what opt_state() returned (centered RMSProp also takes the
    older forms optim_state.rmsprop_moments accepts)."""
    base = self.base_optimizer
    if self.clip_norm is not None:
      state = optim_state.chained_inner(state)
    if isinstance(base, AdamConfig):
      count, mu, nu = optim_state.adam_moments(state)
      self.set_opt_state(mu, nu)
      self.count.fill_(int(count))
    elif base.centered:
      if 'count' in getattr(state[0], '_fields', ()):
        raise ValueError('an Adam state cannot restore a centered-RMSProp learner')
      self.set_opt_state(*optim_state.rmsprop_moments(state))
    else:
      self.nu.copy_(torch.from_numpy(
          self.network.flatten(optim_state.rms_moments(state))))

  def params_tree(self, which='online'):
    t = {'online': self.online, 'target': self.target, 'mu': self.mu,
         'nu': self.nu}[which]
    return self.network.unflatten(t.detach().cpu().numpy())

  def sync_target(self, stream=None):
    """target <- online (dqn/agent.py:155-156)."""
    _native.check(_native.lib().dqz_target_copy(
        _native.ptr(self.target), _native.ptr(self.online), self.total,
        _native.stream_handle(stream)))

  # -- hot path ------------------------------------------------------------

  def _check_slots(self, slots, name='slots'):
    if slots.dtype != torch.int32 or slots.numel() != self.batch_size:
      raise ValueError('%s must be a device int32 tensor of batch size' % name)

  def step(self, store, slots, weights=None, stream=None, write_back=None):
    """One learner step on replay `slots` (device int32 [B]).

    write_back (PER only): (tree, cap, indices, alpha, max_seen_dev) — the
    priority write-back of this step's |td| (dqz_per_write_back's arguments)
    folded into the backward launch (dqz_learner_step_per)."""
    self._check_slots(slots)
    if self.algo == 'per' and weights is None:
      raise ValueError('PER step needs importance weights')
    if self._opt_h is not None:
      _native.check(_native.lib().dqz_learner_step_opt(
          self._h, ctypes.byref(self._params_c), store.c_ref(),
          _native.ptr(slots), _native.ptr(weights), self._opt_h,
          _native.ptr(self.count), _native.stream_handle(stream)))
      if write_back is not None:  # its own launch: it reads the step's td
        tree, cap, indices, alpha, max_seen = write_back
        _native.check(_native.lib().dqz_per_write_back(
            self._h, _native.ptr(tree), int(cap), _native.ptr(indices),
            float(alpha), _native.ptr(max_seen), _native.stream_handle(stream)))
      return
    if write_back is not None:
      tree, cap, indices, alpha, max_seen = write_back
      _native.check(_native.lib().dqz_learner_step_per(
          self._h, ctypes.byref(self._params_c), store.c_ref(),
          _native.ptr(slots), _native.ptr(weights), _native.ptr(tree), int(cap),
          _native.ptr(indices), float(alpha), _native.ptr(max_seen),
          _native.stream_handle(stream)))
      return
    _native.check(_native.lib().dqz_learner_step(
        self._h, ctypes.byref(self._params_c), store.c_ref(),
        _native.ptr(slots), _native.ptr(weights), _native.stream_handle(stream)))

  def step_uniform(self, store, base, size, capacity, seed, counter, slots_out,
                   stream=None):
    """Uniform sample + learner step in one pass (sampler fused into conv1).

    Draws exactly what `sample_uniform(base, size, capacity, B, seed,
    counter, ...)` would, writes them to `slots_out` and advances `counter`.
    """
    self._check_slots(slots_out, 'slots_out')
    if self._opt_h is not None:
      _native.check(_native.lib().dqz_learner_step_opt_uniform(
          self._h, ctypes.byref(self._params_c), store.c_ref(), int(base),
          int(size), int(capacity), int(seed) & (2**64 - 1),
          _native.ptr(counter), _native.ptr(slots_out), self._opt_h,
          _native.ptr(self.count), _native.stream_handle(stream)))
      return
    _native.check(_native.lib().dqz_learner_step_uniform(
        self._h, ctypes.byref(self._params_c), store.c_ref(), int(base),
        int(size), int(capacity), int(seed) & (2**64 - 1), _native.ptr(counter),
        _native.ptr(slots_out), _native.stream_handle(stream)))

  def step_logits(self, store, logit_buffer, slots_out, seed=0, counter=None,
                  uniforms=None, stream=None, exact=False):
    """Learned-logit sample + learner step, the draw inside the forward
    launch (dqz_learner_step_logits): draws what
    logit_buffer.sample_slots_philox(seed, counter, slots_out) — or, given
    device f64 `uniforms` [B] (a Generator's draws), sample_abs(uniforms) —
    would, writes them to `slots_out` and (Philox) advances `counter`.

    exact=True (dqz_learner_step_logits_exact): the reference's own float32
    probabilities and its choice, bit for bit — what
    logit_buffer.sample_exact(uniforms) draws — after three preparation
    launches over the buffer."""
    self._check_slots(slots_out, 'slots_out')
    if (counter is None) == (uniforms is None):
      raise ValueError('pass exactly one of counter (Philox) and uniforms')
    self._need_fused_rmsprop('step_logits')
    lib = _native.lib()
    fn = lib.dqz_learner_step_logits_exact if exact else lib.dqz_learner_step_logits
    _native.check(fn(
        self._h, ctypes.byref(self._params_c), store.c_ref(),
        logit_buffer.handle, _native.ptr(logit_buffer.logits),
        int(seed) & (2**64 - 1), _native.ptr(counter), _native.ptr(uniforms),
        _native.ptr(slots_out), _native.stream_handle(stream)))

  def step_per_draw(self, store, draw, stream=None):
    """A whole prioritized learn in one learner step
    (dqz_learner_step_per_draw): the PER draw inside the forward launch, the
    IS weights in the head, the write-back inside the backward launch.
    `draw` is a _native.DqzPerDraw (see
    replay.PrioritizedTransitionReplay.per_draw)."""
    if self.algo != 'per':
      raise ValueError('step_per_draw needs a PER learner')
    if self._opt_h is not None:
      _native.check(_native.lib().dqz_learner_step_opt_per_draw(
          self._h, ctypes.byref(self._params_c), store.c_ref(),
          ctypes.byref(draw), self._opt_h, _native.ptr(self.count),
          _native.stream_handle(stream)))
      return
    _native.check(_native.lib().dqz_learner_step_per_draw(
        self._h, ctypes.byref(self._params_c), store.c_ref(), ctypes.byref(draw),
        _native.stream_handle(stream)))

  def grad(self, store, slots, weights=None, out=None, stream=None):
    """jax.grad(loss_fn) of the same step into a flat tensor (no update).
    Every element of every leaf is written; the padding floats between the
    leaves and behind the last keep what `out` held (zeros in the tensor
    allocated here)."""
    self._check_slots(slots)
    out = torch.zeros_like(self.online) if out is None else out
    _native.check(_native.lib().dqz_learner_grad(
        self._h, ctypes.byref(self._params_c), store.c_ref(),
        _native.ptr(slots), _native.ptr(weights), _native.ptr(out),
        _native.stream_handle(stream)))
    return out

  def profile(self, store, slots, weights=None, iters=20, stream=None):
    """Average ms per phase (HIP events on the launch stream), dict."""
    self._need_fused_rmsprop('profile')
    out = (ctypes.c_float * _native.NUM_PHASES)()
    _native.check(_native.lib().dqz_learner_profile(
        self._h, ctypes.byref(self._params_c), store.c_ref(),
        _native.ptr(slots), _native.ptr(weights), int(iters), out,
        _native.stream_handle(stream)))
    ms = [float(x) for x in out]
    names = list(_native.PHASE_NAMES)
    # phases merged into another launch report 0 and are left out
    return {n: t for n, t in zip(names, ms) if t > 0.0}

  def _need_fused_rmsprop(self, what):
    if self._opt_h is not None:
      raise NotImplementedError(
          '%s runs the fused centered-RMSProp step only; this learner applies '
          '%s after the step (dqz_learner_step_opt*)' % (
              what, type(self.base_optimizer).__name__))

  def grad_norm(self, stream=None):
    """Global norm of the last step's gradient, before clipping: a device
    f32 [1] tensor (dqz_optimizer_outputs).  Adam / plain RMSProp / clipped
    chains only; the fused centered-RMSProp step keeps no gradient."""
    if self._opt_h is None:
      raise NotImplementedError(
          'the fused centered-RMSProp step does not keep its gradient; use '
          'Learner.grad()')
    _native.check(_native.lib().dqz_optimizer_outputs(
        self._opt_h, _native.ptr(self._gnorm), _native.stream_handle(stream)))
    return self._gnorm

  def fetch_outputs(self, stream=None):
    """Copies (q_tm1, td, loss) of the last step into self tensors."""
    _native.check(_native.lib().dqz_learner_outputs(
        self._h, _native.ptr(self.q_tm1), _native.ptr(self.td),
        _native.ptr(self.loss), _native.stream_handle(stream)))
    return self.q_tm1, self.td, self.loss

  def sync_status(self):
    """0 if every in-launch backward hand-off completed (synchronises)."""
    st = ctypes.c_int(0)
    _native.check(_native.lib().dqz_learner_sync_status(self._h, ctypes.byref(st)))
    return st.value

  def debug_stall(self, sample, spin_max=0):
    """Test hook (dqz_learner_debug_stall): poison `sample`'s dy2 hand-off
    counter (sample >= 0) and cap the bounded spin at `spin_max` polls."""
    _native.check(_native.lib().dqz_learner_debug_stall(self._h, int(sample), int(spin_max)))

  def debug_backward(self, chain=-1):
    """Test hook (dqz_learner_debug_backward): the backward launch's grid from
    the next step on: 1 the chain grid where it is legal (batch <= 64), 0
    the separate block ranges, -1 the default (the chain for 2 <= batch <=
    64).  Returns what the next step
    will use (1 or 0); both compute the same bits."""
    active = ctypes.c_int(-1)
    _native.check(_native.lib().dqz_learner_debug_backward(
        self._h, int(chain), ctypes.byref(active)))
    return active.value

  def debug_sync_words(self):
    """Test hook (dqz_learner_debug_sync_words): the learner's in-launch
    hand-off words and error word as a numpy int32 array (synchronises).
    All zero between launches."""
    total = ctypes.c_int64(0)
    fn = _native.lib().dqz_learner_debug_sync_words
    _native.check(fn(self._h, None, 0, ctypes.byref(total)))
    out = np.zeros((total.value,), np.int32)
    _native.check(fn(self._h, out.ctypes.data, total.value, None))
    return out

  def fetch_activations(self, z=0, backward=False, stream=None):
    """Diagnostic (dqz_learner_debug_activations): the intermediates of the
    most recent step / gradient call as a dict of fresh device tensors.
    Network copy z (0 online(s_tm1), 1 target(s_t), 2 online(s_t)): y1
    [B,20,20,32], y2 [B,9,9,64], y3 [B,7,7,64], h1 [B,512] (post-ReLU) and q
    [B,A]; with `backward`, also dz1 [B,512], dy3 [B,7,7,64], dy2 [B,9,9,64]
    and dy1 [B,20,20,32] of copy 0: d loss / d pre-activation, each already
    multiplied by its own ReLU mask."""
    b, a = self.batch_size, self.network.num_actions
    shapes = dict(y1=(b, 20, 20, 32), y2=(b, 9, 9, 64), y3=(b, 7, 7, 64),
                  h1=(b, 512), q=(b, a))
    if backward:
      shapes.update(dz1=(b, 512), dy3=(b, 7, 7, 64), dy2=(b, 9, 9, 64),
                    dy1=(b, 20, 20, 32))
    out = {k: torch.empty(s, dtype=torch.float32, device=self.device)
           for k, s in shapes.items()}
    _native.check(_native.lib().dqz_learner_debug_activations(
        self._h, int(z),
        *(_native.ptr(out.get(k)) for k in ('y1', 'y2', 'y3', 'h1', 'q', 'dz1',
                                             'dy3', 'dy2', 'dy1')),
        _native.stream_handle(stream)))
    return out

  def q_values(self, states, params=None, stream=None):
    """network.apply(params, s).q_values for uint8 [n,84,84,4] device states."""
    return self._forward(states, params, stream)

  # The workers of q_values, q_values_slots and act: `extra` is what the
  # head's entry takes between the inputs and the outputs.

  def _forward(self, states, params, stream, *extra):
    params = self.online if params is None else params
    states = states.contiguous()
    n = int(states.shape[0])
    out = torch.empty((n, self.network.num_actions), dtype=torch.float32,
                      device=self.device)
    for i in range(0, n, self.batch_size):
      j = min(n, i + self.batch_size)
      _native.check(self._call(
          'forward', _native.ptr(params), _native.ptr(states[i:j]), j - i,
          *extra, _native.ptr(out[i:j]), _native.stream_handle(stream)))
    return out

  def _forward_slots(self, store, slots, which, params, stream, *extra):
    params = self.online if params is None else params
    n = int(slots.numel())
    out = torch.empty((n, self.network.num_actions), dtype=torch.float32,
                      device=self.device)
    _native.check(self._call(
        'forward_slots', _native.ptr(params), store.c_ref(), _native.ptr(slots),
        n, int(which), *extra, _native.ptr(out), _native.stream_handle(stream)))
    return out

  def _forward_act(self, observation, params, *extra):
    if self._act_in is None:
      self._act_in = torch.empty((1, 84, 84, 4), dtype=torch.uint8,
                                 pin_memory=True)
      self._act_in_np = self._act_in.numpy()
      self._act_out = torch.zeros((2,), dtype=torch.int32, pin_memory=True)
      self._act_out_np = self._act_out.numpy()
    self._act_in_np[0] = observation
    _native.check(self._call(
        'act', _native.ptr(self._params_tensor(params)),
        ctypes.c_void_p(self._act_in.data_ptr()), 1, *extra,
        ctypes.c_void_p(self._act_out.data_ptr()), _native.stream_handle()))
    torch.cuda.current_stream(self.device).synchronize()
    return int(self._act_out_np[0]), float(self._act_out_np.view(np.float32)[1])

  def _params_tensor(self, params):
    """Flat device parameters from None (online), a flat tensor, a device
    tree of views (agent.online_params: no copy) or a host tree."""
    if params is None:
      return self.online
    if isinstance(params, torch.Tensor):
      return params
    leaf = next(iter(next(iter(params.values())).values()))
    if isinstance(leaf, torch.Tensor):
      flat = self.network.flat_of_device_tree(params)
      if flat is not None:
        return flat
      params = {m: {n: v.detach().cpu().numpy() for n, v in d.items()}
                for m, d in params.items()}
    return torch.from_numpy(self.network.flatten(params)).to(self.device)

  def q_values_host(self, observation, params=None):
    """Q-values of one host uint8 [84,84,4] state (the actor's select_action)."""
    obs = np.ascontiguousarray(observation, dtype=np.uint8)
    if obs.ndim == 3:
      obs = obs[None]
    if getattr(self, '_obs_buf', None) is None or self._obs_buf.shape[0] < obs.shape[0]:
      self._obs_buf = torch.empty((max(obs.shape[0], 1), 84, 84, 4),
                                  dtype=torch.uint8, device=self.device)
    buf = self._obs_buf[:obs.shape[0]]
    buf.copy_(torch.from_numpy(obs))
    q = self.q_values(buf, self._params_tensor(params))
    out = q.cpu().numpy()
    return out[0] if observation.ndim == 3 else out

  def act(self, observation, epsilon, seed, counter, params=None):
    """select_action on device (dqn/agent.py:121-131, c51/agent.py:121-129):
    (action, max_a q) for one host uint8 [84,84,4] observation, the
    eps-greedy draw being number `counter` of the Philox stream `seed`
    (dqz_act, dqz_c51_act).  The observation is read and the result written
    in place in pinned host buffers: one launch chain and one stream
    synchronisation per call, no staging copies."""
    return self._forward_act(observation, params, float(epsilon),
                             int(seed) & (2**64 - 1), int(counter) & (2**64 - 1))

  def q_values_slots(self, store, slots, which, params=None, stream=None):
    return self._forward_slots(store, slots, which, params, stream)


def sample_uniform(base, size, capacity, n, seed, counter, out, stream=None):
  """Device Philox uniform sampler (replay.py:119-125 distribution)."""
  _native.check(_native.lib().dqz_sample_uniform(
      int(base), int(size), int(capacity), int(n), int(seed) & (2**64 - 1),
      _native.ptr(counter), _native.ptr(out), _native.stream_handle(stream)))
  return out


def _wide_entries(prefix):
  """_ENTRIES of a wide head: every entry is `prefix` + its own name."""
  return {e: prefix + e for e in (
      'create', 'learner', 'optimizer_create', 'destroy', 'step', 'grad',
      'outputs', 'debug', 'profile', 'forward', 'forward_slots', 'act',
      'create_opt', 'step_w', 'grad_w', 'profile_w', 'outputs_opt')}


class _WideLearner(Learner):
  """What the categorical and the quantile learners share: everything but the
  names a subclass states below.

  Same state surface as `Learner` (params, moments, opt_state, sync_target,
  sync_status, grad_norm); the step is the learner step with the wide head, in
  gradient mode, followed by the optimizer, so the optimizer is Adam or plain
  RMSProp, alone or behind clip_by_global_norm (the reference's chain is the
  default).

  double_q / prioritized (dqz_wide_options): Rainbow's learning rule on the
  same network.  double_q selects a* with the online network at s_t, a third
  copy whose q_values are `q[2]`.  prioritized makes every step take the
  replay's importance `weights` [B]: the loss is mean(w loss_b), loss_b stays
  unweighted, and `priorities` [B] = clip(|loss_b|, 0, 100) are also what
  dqz_per_write_back on this learner's inner handle writes to the sum tree.
  With both off the old create entry is called and nothing differs."""

  _wide = None  # the head's handle (dqz_c51 / dqz_qr); it owns the dqz_learner behind _h
  _OWNER = '_wide'
  # what a subclass states
  _CLASS = _NETWORK = None  # its own name and its network factory's, for messages
  _SPEC = None  # the network spec's class ...
  _COUNT = _GRID = None  # ... and its attributes: N and the [N] grid (also the learner's tensor of it)
  _TAKEN = None  # the learner's [B,N] output tensor of the taken action
  _LEARNING_RATE = None  # of the default optimizer
  _ALGO = _TITLE = _HEAD = None  # `algo`, and the head's names in messages
  _PROFILE_SLOTS = None  # profile(): phase slot -> the head's launch there

  def __init__(self, network, batch_size, optimizer, device, *head_args,
               double_q=False, prioritized=False):
    if not isinstance(network, self._SPEC):
      raise ValueError('%s needs networks.%s' % (self._CLASS, self._NETWORK))
    head_args = self._check_head_args(*head_args)
    optimizer = optimizer or chain(clip_by_global_norm(10.0),
                                   adam(self._LEARNING_RATE, eps=0.01 / 32))
    if is_centered_rmsprop(optimizer):
      raise NotImplementedError(
          '%s applies its optimizer to the finished gradient: centered '
          'RMSProp exists only fused into the DQN step; use adam(...), '
          'rmsprop(..., centered=False) or chain(clip_by_global_norm(c), one '
          'of them)' % self._CLASS)
    self.algo = self._ALGO
    self.grad_error_bound = 0.0
    self._alloc_state(network, batch_size, optimizer, device)
    b, a, n = self.batch_size, network.num_actions, getattr(network, self._COUNT)
    f32 = dict(dtype=torch.float32, device=self.device)
    grid = torch.from_numpy(getattr(network, self._GRID)).to(self.device)
    setattr(self, self._GRID, grid)
    setattr(self, self._TAKEN, torch.zeros((b, n), **f32))
    self.double_q, self.prioritized = bool(double_q), bool(prioritized)
    self.copies = 3 if self.double_q else 2
    self.q = torch.zeros((self.copies, b, a), **f32)
    self.priorities = torch.zeros((b,), **f32) if self.prioritized else None
    self.loss_b = torch.zeros((b,), **f32)
    self.loss = torch.zeros((1,), **f32)
    self.a_star = torch.zeros((b,), dtype=torch.int32, device=self.device)
    handle = ctypes.c_void_p()
    if self.double_q or self.prioritized:
      options = _native.DqzWideOptions(int(self.double_q), int(self.prioritized))
      _native.check(self._entry('create_opt')(
          ctypes.byref(self._learner_config(_native.ALGO_DQN)), n,
          _native.ptr(grid), *head_args, ctypes.byref(options),
          ctypes.byref(handle)))
    else:
      _native.check(self._entry('create')(
          ctypes.byref(self._learner_config(_native.ALGO_DQN)), n,
          _native.ptr(grid), *head_args, ctypes.byref(handle)))
    self._wide = handle
    inner = ctypes.c_void_p()
    _native.check(self._call('learner', ctypes.byref(inner)))
    self._h = inner  # owned by the head's handle: sync_status, fetch_activations
    self._opt_h = self._create_optimizer(self._entry('optimizer_create'), n)

  def _check_head_args(self):
    """The head's own constructor arguments, checked: what its create entry
    takes between the grid and the handle."""
    return ()

  def _out_shape(self, b, a, n):
    """fetch_head's view of one copy's [B][A N] outputs."""
    raise NotImplementedError

  def load_opt_state(self, state):
    """Restores what opt_state() returned; a centered-RMSProp state (a DQN
    agent's checkpoint) is refused by name."""
    if optim_state.is_rmsprop_state(state):
      raise ValueError(
          'a centered-RMSProp state cannot restore a %s learner (its '
          'optimizer is %s)' % (self._TITLE, type(self.base_optimizer).__name__))
    super().load_opt_state(state)

  def _weighted_args(self, slots, weights):
    """(entry suffix, arguments behind the store) of a step on `slots`: a
    prioritized learner takes `weights` (device f32 [B]), another none."""
    self._check_slots(slots)
    if not self.prioritized:
      if weights is not None:
        raise ValueError(
            'this %s takes no importance weights: create it with '
            'prioritized=True' % self._CLASS)
      return '', (_native.ptr(slots),)
    if weights is None:
      raise ValueError('a prioritized %s step needs importance weights'
                       % self._CLASS)
    if (weights.dtype != torch.float32 or weights.numel() != self.batch_size or
        not weights.is_contiguous() or not weights.is_cuda):
      raise ValueError('weights must be a device float32 tensor of batch size')
    return '_w', (_native.ptr(slots), _native.ptr(weights))

  def _run(self, entry, store, slots, weights, extra, tail, stream):
    """The worker of step, grad and profile: the head's `entry` (its _w twin
    in a prioritized learner) on the batch, what the head takes behind the
    weights (`extra`, checked by _extra_args behind slots and weights) and the
    entry's own last arguments (`tail`)."""
    suffix, args = self._weighted_args(slots, weights)
    _native.check(self._call(
        entry + suffix, ctypes.byref(self._params_c), store.c_ref(), *args,
        *self._extra_args(*extra), *tail, _native.stream_handle(stream)))

  def _extra_args(self):
    """The head's own step inputs, checked, as the entry's arguments."""
    return ()

  def _profile(self, store, slots, weights, extra, iters, stream):
    """profile's body: the gradient goes to a scratch tensor, the average ms
    per launch come back under the head's own names."""
    scratch = torch.zeros_like(self.online)
    ms = (ctypes.c_float * _native.NUM_PHASES)()
    self._run('profile', store, slots, weights, extra,
              (_native.ptr(scratch), int(iters), ms), stream)
    names = list(_native.PHASE_NAMES)
    for slot, name in self._PROFILE_SLOTS.items():
      names[slot] = name
    return {n: float(t) for n, t in zip(names, ms) if t > 0.0}

  def step(self, store, slots, weights=None, stream=None):  # pylint: disable=arguments-differ
    """One learner step on replay `slots` (device int32 [B]); a prioritized
    learner's also takes the importance `weights` (device f32 [B])."""
    self._run('step', store, slots, weights, (),
              (self._opt_h, _native.ptr(self.count)), stream)

  def grad(self, store, slots, weights=None, out=None, stream=None):  # pylint: disable=arguments-differ
    """jax.grad(loss_fn) of the same step into a flat tensor (no update).
    Every element of every leaf is written; the padding floats between the
    leaves and behind the last keep what `out` held (zeros in the tensor
    allocated here)."""
    out = torch.zeros_like(self.online) if out is None else out
    self._run('grad', store, slots, weights, (), (_native.ptr(out),), stream)
    return out

  def apply(self, grad, stream=None):
    """The optimizer on a finished gradient (what step does behind grad)."""
    _native.check(_native.lib().dqz_optimizer_apply(
        self._opt_h, _native.ptr(self.online), _native.ptr(grad),
        _native.ptr(self.mu), _native.ptr(self.nu), _native.ptr(self.count),
        _native.stream_handle(stream)))

  def fetch_outputs(self, stream=None):
    """(outputs of the taken action [B,N], q_values [2,B,A] of online(s_tm1)
    and target(s_t), per-sample loss [B], mean loss [1], the target's greedy
    action [B]) of the last step, copied into self tensors.  With double_q,
    q_values is [3,B,A] (the third block: online(s_t), the selector) and the
    action is the selector's; a prioritized learner's tuple ends in the
    priorities [B].  The per-sample loss is unweighted, the mean weighted."""
    taken = getattr(self, self._TAKEN)
    _native.check(self._call(
        'outputs', _native.ptr(taken), _native.ptr(self.q),
        _native.ptr(self.loss_b), _native.ptr(self.loss),
        _native.ptr(self.a_star), _native.stream_handle(stream)))
    out = (taken, self.q, self.loss_b, self.loss, self.a_star)
    if self.double_q or self.prioritized:
      _native.check(self._call(
          'outputs_opt', _native.ptr(self.q[2]) if self.double_q else None,
          _native.ptr(self.priorities), _native.stream_handle(stream)))
    return out + (self.priorities,) if self.prioritized else out

  def fetch_head(self, stream=None):
    """Diagnostic: the last step's outputs of every copy (_out_shape; three
    with double_q) and the cotangent [B,N] of the taken action's."""
    b, a = self.batch_size, self.network.num_actions
    n = getattr(self.network, self._COUNT)
    shape = (self.copies,) + tuple(self._out_shape(b, a, n))[1:]
    out = torch.empty(shape, dtype=torch.float32,
                      device=self.device)
    dtaken = torch.empty((b, n), dtype=torch.float32, device=self.device)
    _native.check(self._call('debug', _native.ptr(out), _native.ptr(dtaken),
                             _native.stream_handle(stream)))
    return out, dtaken

  def profile(self, store, slots, weights=None, iters=20, stream=None):  # pylint: disable=arguments-differ
    """Average ms per launch (the head's profile entry), dict; the gradient
    goes to a scratch tensor and no parameter changes."""
    return self._profile(store, slots, weights, (), iters, stream)

  def _no_fused_draw(self, *unused_args, **unused_kwargs):
    raise NotImplementedError(
        'the %s step takes its batch as slots: sample them first '
        '(replay.sample_slots) and call step' % self._HEAD)

  step_uniform = step_logits = step_per_draw = _no_fused_draw


class C51Learner(_WideLearner):
  """The categorical (C51) learner: `update` of c51/agent.py:109-117 and
  `select_action` of :121-129 on device (dqz_c51_*); the default optimizer is
  the chain of c51/run_atari.py:210-216.  Its tensors of the head: `support`
  [N] and `logits_a` [B,N]."""

  _ENTRIES = _wide_entries('dqz_c51_')
  _CLASS, _NETWORK = 'C51Learner', 'c51_atari_network'
  _SPEC = networks_lib.C51NetworkSpec
  _COUNT, _GRID, _TAKEN = 'num_atoms', 'support', 'logits_a'
  _LEARNING_RATE = 2.5e-4
  _ALGO, _TITLE, _HEAD = 'c51', 'C51', 'categorical'
  _PROFILE_SLOTS = {4: 'c51_logits', 8: 'c51_head', 7: 'c51_fc2_grad'}
  _c51 = property(lambda self: self._wide)

  def __init__(self, network: networks_lib.C51NetworkSpec, batch_size,
               optimizer=None, device='cuda', double_q=False,
               prioritized=False):
    super().__init__(network, batch_size, optimizer, device,
                     double_q=double_q, prioritized=prioritized)

  def _out_shape(self, b, a, n):
    return (2, b, a, n)  # q_logits


class RainbowLearner(_WideLearner):
  """The Rainbow learner (rainbow/agent.py): the categorical head, always
  double-Q and prioritized, behind the noisy dueling network
  (networks.rainbow_atari_network) on device (dqz_rainbow_*).

  Noise is an argument everywhere: a step reads `noise` [3, noise_len]
  (online(s_tm1), target(s_t), online(s_t)), a forward or an actor call
  [noise_len]; `make_noise(seed, counter)` draws it on device and advances
  the device counter, so equal (seed, counter) give equal bits.  Its tensors
  of the head: `support` [N] and `logits_a` [B,N]."""

  # always prioritized: its one step, grad and profile are the weighted ones
  _ENTRIES = dict(
      {e: 'dqz_rainbow_' + e for e in (
          'learner', 'optimizer_create', 'destroy', 'outputs', 'forward',
          'forward_slots', 'act', 'outputs_opt')},
      create_opt='dqz_rainbow_create', debug='dqz_rainbow_debug_head',
      step_w='dqz_rainbow_step', grad_w='dqz_rainbow_grad',
      profile_w='dqz_rainbow_profile')
  _CLASS, _NETWORK = 'RainbowLearner', 'rainbow_atari_network'
  _SPEC = networks_lib.RainbowNetworkSpec
  _COUNT, _GRID, _TAKEN = 'num_atoms', 'support', 'logits_a'
  _LEARNING_RATE = 6.25e-5
  _ALGO, _TITLE, _HEAD = 'rainbow', 'Rainbow', 'rainbow'
  _PROFILE_SLOTS = {4: 'rb_noisy_forward', 8: 'c51_head', 2: 'rb_dhidden',
                    5: 'rb_fc1_dx', 7: 'rb_fc_grad'}

  def __init__(self, network: networks_lib.RainbowNetworkSpec, batch_size,
               optimizer=None, device='cuda'):
    optimizer = optimizer or chain(clip_by_global_norm(10.0),
                                   adam(self._LEARNING_RATE, eps=0.005 / 32))
    super().__init__(network, batch_size, optimizer, device,
                     double_q=True, prioritized=True)
    self.noise_len = _native.rainbow_noise_len(network.num_actions,
                                               network.num_atoms)

  def _out_shape(self, b, a, n):
    return (3, b, a, n)  # q_logits

  def make_noise(self, seed, counter, applications=3, out=None, stream=None):
    """[applications, noise_len] of sign(t) sqrt|t|, t ~ N(0, 1) truncated to
    [-2, 2], from Philox stream `seed` at the device uint64 `counter` [1],
    which advances by the number of floats drawn."""
    n = int(applications) * self.noise_len
    if out is None:
      out = torch.empty((int(applications), self.noise_len),
                        dtype=torch.float32, device=self.device)
    _native.check(_native.lib().dqz_rainbow_noise(
        int(seed) & (2**64 - 1), _native.ptr(counter), n, _native.ptr(out),
        _native.stream_handle(stream)))
    return out

  def _check_noise(self, noise, applications):
    if (noise is None or noise.dtype != torch.float32 or not noise.is_cuda or
        not noise.is_contiguous() or
        noise.numel() != applications * self.noise_len):
      raise ValueError('noise must be a contiguous device float32 tensor of '
                       '%d x noise_len (%d) floats'
                       % (applications, self.noise_len))

  def _extra_args(self, noise):  # pylint: disable=arguments-differ
    """A step's noise [3, noise_len], checked behind slots and weights."""
    self._check_noise(noise, 3)
    return (_native.ptr(noise),)

  def step(self, store, slots, weights=None, noise=None, stream=None):  # pylint: disable=arguments-differ
    """One learner step on `slots` with importance `weights` [B] under
    `noise` [3, noise_len]."""
    self._run('step', store, slots, weights, (noise,),
              (self._opt_h, _native.ptr(self.count)), stream)

  def grad(self, store, slots, weights=None, noise=None, out=None, stream=None):  # pylint: disable=arguments-differ
    """The step's gradient into a flat tensor (no update); padding floats keep
    what `out` held."""
    out = torch.zeros_like(self.online) if out is None else out
    self._run('grad', store, slots, weights, (noise,), (_native.ptr(out),),
              stream)
    return out

  def profile(self, store, slots, weights=None, noise=None, iters=20, stream=None):  # pylint: disable=arguments-differ
    return self._profile(store, slots, weights, (noise,), iters, stream)

  def fetch_noisy(self, stream=None):
    """Diagnostic: application 0's (h_adv, h_val [B,512], adv [B,A,N], val
    [B,N], dz_adv, dz_val [B,512]) of the last step."""
    b, a, n = self.batch_size, self.network.num_actions, self.network.num_atoms
    f32 = dict(dtype=torch.float32, device=self.device)
    outs = [torch.empty(s, **f32) for s in
            ((b, 512), (b, 512), (b, a, n), (b, n), (b, 512), (b, 512))]
    _native.check(_native.lib().dqz_rainbow_debug(
        self._wide, *[_native.ptr(t) for t in outs],
        _native.stream_handle(stream)))
    return tuple(outs)

  def q_values(self, states, noise=None, params=None, stream=None):  # pylint: disable=arguments-differ
    """q_values [n,A] of uint8 [n,84,84,4] device states under one
    application's `noise` [noise_len].  n may exceed the batch size: the
    states then go through in batch-size chunks, every chunk under the same
    noise vector, which is the reference's single application over a whole
    batch."""
    self._check_noise(noise, 1)
    return self._forward(states, params, stream, _native.ptr(noise))

  def q_values_slots(self, store, slots, which, noise=None, params=None, stream=None):  # pylint: disable=arguments-differ
    self._check_noise(noise, 1)
    return self._forward_slots(store, slots, which, params, stream,
                               _native.ptr(noise))

  def act(self, observation, noise, params=None):  # pylint: disable=arguments-differ
    """(argmax_a q, max_a q) of one host uint8 [84,84,4] observation under
    `noise` [noise_len]: no epsilon (rainbow/agent.py: the noise explores)."""
    self._check_noise(noise, 1)
    return self._forward_act(observation, params, _native.ptr(noise))


def check_huber_param(huber_param):
  """The quantile head's huber_param as a float; 0 is refused by name."""
  huber_param = float(huber_param)
  if huber_param == 0.0:
    raise NotImplementedError(
        'huber_param = 0 (rlax\'s plain |delta| branch, whose gradient jumps '
        'at every delta = 0) is not built: the quantile head takes '
        'huber_param > 0')
  if not (np.isfinite(huber_param) and huber_param > 0.0):
    raise ValueError('huber_param must be finite and > 0')
  return huber_param


class QrLearner(_WideLearner):
  """The quantile (QR-DQN) learner: `update` of qrdqn/agent.py:112-120 and
  `select_action` of :122-134 on device (dqz_qr_*); the default optimizer is
  the chain of qrdqn/run_atari.py:213-219.  Its tensors of the head:
  `quantiles` [N] and `theta` [B,N]."""

  _ENTRIES = _wide_entries('dqz_qr_')
  _CLASS, _NETWORK = 'QrLearner', 'qr_atari_network'
  _SPEC = networks_lib.QRNetworkSpec
  _COUNT, _GRID, _TAKEN = 'num_quantiles', 'quantiles', 'theta'
  _LEARNING_RATE = 5e-5
  _ALGO, _TITLE, _HEAD = 'qrdqn', 'QR-DQN', 'quantile'
  _PROFILE_SLOTS = {4: 'qr_outputs', 8: 'qr_head', 2: 'qr_dz1',
                    7: 'qr_fc2_grad'}
  _qr = property(lambda self: self._wide)

  def __init__(self, network: networks_lib.QRNetworkSpec, batch_size,
               huber_param=1.0, optimizer=None, device='cuda', double_q=False,
               prioritized=False):
    super().__init__(network, batch_size, optimizer, device, huber_param,
                     double_q=double_q, prioritized=prioritized)

  def _check_head_args(self, huber_param):  # pylint: disable=arguments-differ
    self.huber_param = check_huber_param(huber_param)
    return (self.huber_param,)

  def _out_shape(self, b, a, n):
    return (2, b, n, a)  # q_dist: quantile-major


class _BorrowedLearner:
  """A dqz_learner the meta handle owns (MetaLearner.debug_learners): what
  Learner.fetch_activations and Learner.fetch_outputs need, nothing else.
  Keeps its MetaLearner alive; never destroys the handle."""

  def __init__(self, meta, handle, batch_size):
    self._owner = meta
    self._h = handle
    self.batch_size = batch_size
    self.network = meta.learner.network
    self.device = meta.learner.device
    f32 = dict(dtype=torch.float32, device=self.device)
    self.q_tm1 = torch.zeros((batch_size, self.network.num_actions), **f32)
    self.td = torch.zeros((batch_size,), **f32)
    self.loss = torch.zeros((1,), **f32)

  fetch_activations = Learner.fetch_activations
  fetch_outputs = Learner.fetch_outputs


class MetaLearner:
  """MGSC meta-update on device (dqn_mgsc_batched/agent.py:104-220, 302-334).

  second_order=True is the reservoir agent's meta_loss_fn (no stop_gradient
  on theta'', dqn_mgsc_batched_reservoir/agent.py): the gradient also flows
  through the online transition's gradient at theta' (a Hessian-vector
  product, hvp.hpp).

  Holds the meta optimizer state (optax ScaleByAdamState(count, mu, nu) over
  the M meta-batch logits, shared across calls exactly as the reference's
  `self._meta_opt_state`) and a one-slot frame store for the newest
  transition.  `update` reads the learner's online/target params and RMSProp
  state, never modifies them, and writes the Adam-updated logits back into
  the replay's device logit buffer at the meta batch's positions
  (replay.update_priorities(indices, new_meta_params)).
  """

  def __init__(self, learner: Learner, meta_batch_size, meta_optimizer=None,
               second_order=False):
    from dqn_mgsc_zoo_amd import store as store_lib  # pylint: disable=g-import-not-at-top
    if learner.algo != 'dqn':
      raise ValueError('the MGSC agents use q_learning on dqn_atari_network')
    if not is_centered_rmsprop(learner.optimizer):
      raise ValueError(
          'the MGSC meta-gradient differentiates through the centered-RMSProp '
          'update of the learner (theta\' = theta + u(G; mu, nu)); the agent '
          'optimizer must be rmsprop(..., centered=True)')
    meta_optimizer = meta_optimizer or adam(2.5e-4)
    self.learner = learner
    self.meta_batch_size = int(meta_batch_size)
    self.meta_optimizer = meta_optimizer
    self.second_order = bool(second_order)
    dev = learner.device
    m = self.meta_batch_size
    self.adam_mu = torch.zeros((m,), dtype=torch.float32, device=dev)
    self.adam_nu = torch.zeros((m,), dtype=torch.float32, device=dev)
    self.adam_count = torch.zeros((1,), dtype=torch.int32, device=dev)
    self.probs = torch.zeros((m,), dtype=torch.float32, device=dev)
    self.dlogits = torch.zeros((m,), dtype=torch.float32, device=dev)
    self.td = torch.zeros((m,), dtype=torch.float32, device=dev)
    self.loss = torch.zeros((1,), dtype=torch.float32, device=dev)
    self.online_store = store_lib.FrameStore(1, 8, device=dev)
    self.online_store.fidx[0].copy_(torch.arange(8, dtype=torch.int32))
    self.online_slot = torch.zeros((1,), dtype=torch.int32, device=dev)
    opt = learner.optimizer
    cfg = _native.DqzMetaConfig(
        m, learner.network.num_actions, opt.learning_rate, opt.decay, opt.eps,
        learner.grad_error_bound, meta_optimizer.learning_rate,
        meta_optimizer.b1, meta_optimizer.b2, meta_optimizer.eps,
        int(bool(second_order)))
    handle = ctypes.c_void_p()
    _native.check(_native.lib().dqz_meta_create(ctypes.byref(cfg),
                                                ctypes.byref(handle)))
    self._h = handle

  def __del__(self):
    h = getattr(self, '_h', None)
    if h is not None and h.value and _native is not None and _native._lib is not None:  # pylint: disable=protected-access
      _native.lib().dqz_meta_destroy(h)
      self._h = None

  def set_online_transition(self, transition):
    """Uploads the newest host transition (uint8 [84,84,4] stacks): its eight
    channel frames (s_tm1 0..3, s_t 4..7) as pool rows 0..7 of the one-slot
    store plus its {a, r, d} record, in one launch that reads pinned staging
    in place (FrameStore.put / dqz_store_put): no host wait on queued work."""
    s_tm1 = np.asarray(transition.s_tm1, np.uint8)
    s_t = np.asarray(transition.s_t, np.uint8)
    frames = [(c, s_tm1[..., c]) for c in range(4)] + [(4 + c, s_t[..., c]) for c in range(4)]
    self.online_store.put(0, range(8), int(transition.a_tm1), float(transition.r_t),
                          float(transition.discount_t), frames)

  def update(self, store, slots, logits, positions, stream=None,
             logit_buffer=None):
    """One meta_update on replay `slots` (device int32 [M]); logits updated
    in place at `positions` (device int32 [M], distinct).  `logit_buffer`
    (the replay's device logit buffer, replay_circular._DeviceLogits) keeps
    its running log-sum-exp and chunk sums current through the write; when
    it is omitted and `logits` is a live buffer's tensor, that buffer is
    used (a raw tensor kept from `replay.logits` must not bypass the state
    its samplers read)."""
    m = self.meta_batch_size
    if slots.dtype != torch.int32 or slots.numel() != m:
      raise ValueError('slots must be a device int32 tensor of meta batch size')
    if positions.dtype != torch.int32 or positions.numel() != m:
      raise ValueError('positions must be a device int32 tensor [M]')
    if logits.dtype != torch.float32:
      raise ValueError('logits must be float32')
    if logit_buffer is not None and logits.data_ptr() != logit_buffer.logits.data_ptr():
      raise ValueError('logit_buffer does not own these logits')
    if logit_buffer is None:
      from dqn_mgsc_zoo_amd import replay_circular  # pylint: disable=g-import-not-at-top
      logit_buffer = replay_circular.logit_buffer_of(logits)
    lrn = self.learner
    _native.check(_native.lib().dqz_meta_update(
        self._h, ctypes.byref(lrn._params_c), store.c_ref(),  # pylint: disable=protected-access
        _native.ptr(slots), self.online_store.c_ref(),
        _native.ptr(self.online_slot), _native.ptr(logits),
        _native.ptr(positions), _native.ptr(self.adam_mu),
        _native.ptr(self.adam_nu), _native.ptr(self.adam_count),
        None if logit_buffer is None else logit_buffer.handle,
        _native.stream_handle(stream)))

  def fetch_outputs(self, stream=None):
    """(probs [M], dL/dlogits [M], meta-batch td [M], meta loss [1])."""
    _native.check(_native.lib().dqz_meta_outputs(
        self._h, _native.ptr(self.probs), _native.ptr(self.dlogits),
        _native.ptr(self.td), _native.ptr(self.loss),
        _native.stream_handle(stream)))
    return self.probs, self.dlogits, self.td, self.loss

  def sync_status(self):
    """0 if every bounded wait of the meta-update completed and every loss
    was finite since the previous check (dqz_meta_sync_status: the batch
    and one-transition learners' health words and the meta handle's own;
    synchronises; a non-zero word also clears every hand-off word)."""
    st = ctypes.c_int(0)
    _native.check(_native.lib().dqz_meta_sync_status(self._h, ctypes.byref(st)))
    return st.value

  def debug_stall(self, poison=True, spin_max=0):
    """Test hook (dqz_meta_debug_stall): cap every bounded wait of the
    meta handle at `spin_max` polls (0 restores the default) and, with
    `poison`, make the next update's HVP ddot1 and Adam entry waits run out."""
    _native.check(_native.lib().dqz_meta_debug_stall(self._h, int(bool(poison)), int(spin_max)))

  def debug_learners(self):
    """Diagnostic (dqz_meta_debug_learner): (batch learner, one-transition
    learner) as light wrappers of the meta handle's own learners, on which
    fetch_activations and fetch_outputs work as on a Learner.  The batch
    learner holds the last chunk's forward, p-weighted backward signals and
    td; the one-transition learner the pass at theta' (after a second-order
    update its backward signals are the unit-cotangent ones of q[a])."""
    out = []
    for which, b in ((0, min(self.meta_batch_size, 256)), (1, 1)):
      h = ctypes.c_void_p()
      _native.check(_native.lib().dqz_meta_debug_learner(self._h, which, ctypes.byref(h)))
      out.append(_BorrowedLearner(self, h, b))
    return tuple(out)

  def fetch_stages(self, stream=None):
    """Diagnostic (dqz_meta_debug_stages): the stage buffers of the most
    recent update as a dict of fresh device tensors (include/dqz.h
    dqz_meta_stages says what each holds after which kind of update): G, thp,
    mu1, nu1, J [T]; p, s [K C]; second order also GQ, HQ [T], ty1 [400,32],
    ty2 [81,64], ty3 [3136], hpart [196,512], td4 [512], td3 [3136], td2
    [81,64], td1 [400,32], s1 [1]; more than one chunk also zv1 [C,400,32],
    zv2 [C,81,64], zv3 [C,3136], zvp [7,C,512] of the last chunk."""
    t = int(self.learner.online.numel())
    c = min(self.meta_batch_size, 256)
    k = -(-self.meta_batch_size // c)
    shapes = dict(G=(t,), thp=(t,), mu1=(t,), nu1=(t,), J=(t,), p=(k * c,), s=(k * c,))
    if self.second_order:
      shapes.update(GQ=(t,), HQ=(t,), ty1=(400, 32), ty2=(81, 64), ty3=(3136,),
                    hpart=(_native.META_HPART_CHUNKS, 512), td4=(512,), td3=(3136,),
                    td2=(81, 64), td1=(400, 32), s1=(1,))
    if k > 1:
      shapes.update(zv1=(c, 400, 32), zv2=(c, 81, 64), zv3=(c, 3136),
                    zvp=(_native.META_ZVP_PARTS, c, 512))
    out = {n: torch.empty(s, dtype=torch.float32, device=self.learner.device)
           for n, s in shapes.items()}
    req = _native.DqzMetaStages(**{n: v.data_ptr() for n, v in out.items()})
    _native.check(_native.lib().dqz_meta_debug_stages(
        self._h, ctypes.byref(req), _native.stream_handle(stream)))
    return out

  def get_state(self):
    """optax.adam's state, (ScaleByAdamState(count, mu, nu), EmptyState()),
    with host arrays (dqn_mgsc_batched/agent.py:80,390)."""
    return optim_state.adam_state(int(self.adam_count.item()),
                                  self.adam_mu.cpu().numpy(),
                                  self.adam_nu.cpu().numpy())

  def set_state(self, state):
    count, mu, nu = optim_state.adam_moments(state)
    self.adam_count.fill_(count)
    self.adam_mu.copy_(torch.as_tensor(np.asarray(mu, np.float32)))
    self.adam_nu.copy_(torch.as_tensor(np.asarray(nu, np.float32)))
