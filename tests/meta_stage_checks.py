"""Per-stage checks of the MGSC meta-update (tests/test_meta_stages_gpu.py):
every stage of csrc/meta.hpp, csrc/hvp.hpp and the Rms::meta1/3 epilogues
restated as a plain operation on that stage's own inputs, with the bars a
float32 implementation is held to.  No bar is read off an implementation.

Products (the HVP's tangent chain and parameter blocks, the tangent forward
of a chunked meta batch) go through layer_checks.product_check: a stage that
sums two products is ONE product of concatenated operands, e.g.
  ty2 = mask(y2) ([cols(y1) | cols(ty1)] @ [Wdot2 ; W2] + bdot2),  K = 2 x 512,
so both bars (elementwise (K + 3) 2^-24 |a| @ |w|, RMS <= 4 x sequential f32)
apply unchanged.  STAGES lists them in dependency order; `ops` gives a stage's
operands from a dict of inputs, `evaluate` its value in fp64 or numpy
float32, `check` its product_check row.

Dot products (s1 = grad q . w, s_i = v . p_i g_i): `dot_check`, the same two
bars with K the term count (the sequential float32 sum through np.cumsum,
which accumulates in index order).

Elementwise stages, u = 2^-24, every rounding relative to the magnitude it
rounds:
  v = v_dir + J (alpha s1 gq - clip hq)   (hvp.hpp HqOut; `combine_check`)
        t1 = alpha s1 gq, t2 = clip hq, t1 - t2, J (.), v_dir + (.): four
        roundings relative to at most |J| (|t1| + |t2|), the last relative to
        at most |v_dir| + |J| (|t1| + |t2|); hq itself is a K-term product of
        the device's tangents, (K + 3) u |a| @ |w| =: b(hq).  So
        |dv| <= |J clip| b(hq) + u (|v_dir| + 5 |J| (|t1| + |t2|)).
        The error is put against THIS bound, not against |v|: v_dir dominates
        v, and a bar relative to |v| would pass a wrong H_q w leaf.  The RMS
        bar compares with seq_f32's hq through the same float32 combine.
  dlogits_i = s_i - p_i tot, tot = sum_j s_j   (meta.hpp meta_adam_body)
        tot: (M - 1) u sum |s|; p_i tot and the subtraction one rounding
        each: |d| <= u (p_i (M - 1) sum |s| + |s_i| + 2 p_i |tot|).
  mu' = c g + d mu, nu' = c g^2 + d nu   (Rms::meta1, first order only: the
        second order overwrites them)
        three / four roundings: 3 u (|c g| + |d mu|), 4 u (c g^2 + d |nu|).
  theta', J (Rms::meta1, meta_rms1_kernel) and v_dir, w (Rms::meta3) call
        rsqrtf.  Neither the ROCm headers (hip/amd_detail/math_fwd.h declares
        __ocml_rsqrt_f32 without an accuracy) nor a document shipped with the
        toolchain states its error, so these four get NO a-priori bound: they
        are held to the 4 x bar alone, RMS error against fp64 <= 4 x the RMS
        error of the numpy float32 restatement below (np.sqrt and the division
        are correctly rounded), `restated_check`.  Their rows print nan for
        `max err / bound`.  (With a documented figure the bound would have to
        be taken relative to |nu'| + mu'^2 + eps, not to D = nu' - mu'^2 +
        eps, which cancels.)
The optimizer constants enter every restatement as the float32 values the
device holds (`Consts`), so their own rounding is no one's error.

tests/test_meta_stage_checks_cpu.py ties the chained restatements to
oracle.learner_ref (hvp, meta_update), runs the float32 restatements through
every bar, and shows that damaged stages fail theirs.
"""

import types

import numpy as np

from oracle import learner_ref
from tests import layer_checks as lc

f32, f64 = np.float32, np.float64
U = lc.EPS
C = learner_ref.CONV_NAMES
FC1 = 'sequential/sequential_1/linear'
FC2 = 'sequential/sequential_1/linear_1'
LEAVES = ((C[0], 'w'), (C[0], 'b'), (C[1], 'w'), (C[1], 'b'), (C[2], 'w'), (C[2], 'b'),
          (FC1, 'w'), (FC1, 'b'), (FC2, 'w'), (FC2, 'b'))
LEAF_LABEL = ('conv1 w', 'conv1 b', 'conv2 w', 'conv2 b', 'conv3 w', 'conv3 b', 'fc1 w', 'fc1 b',
              'fc2 w', 'fc2 b')


def tree_of(net, flat):
  """Flat parameter-layout array -> tree of views, dtype kept."""
  offsets, sizes, _ = net.layout()
  flat = np.asarray(flat)
  out = {}
  for (mod, name), shape, off, size in zip(net.leaf_paths(), net.leaf_shapes(), offsets, sizes):
    out.setdefault(mod, {})[name] = flat[off:off + size].reshape(shape)
  return out


def flat_of(net, tree, dtype=f64):
  offsets, sizes, total = net.layout()
  flat = np.zeros(total, dtype)
  for (mod, name), off, size in zip(net.leaf_paths(), offsets, sizes):
    flat[off:off + size] = np.asarray(tree[mod][name], dtype).reshape(-1)
  return flat


def result(err, bound, seq_err):
  """product_check's dict from an error array, its a-priori bound (None: the
  stage has none) and the float32 restatement's error array."""
  err, seq_err = np.asarray(err, f64), np.asarray(seq_err, f64)
  rms = float(np.sqrt(np.mean(err**2)))
  rms_seq = float(np.sqrt(np.mean(seq_err**2)))
  if bound is None:
    over, frac, ok = float('nan'), 0.0, True
  else:
    bound = np.broadcast_to(np.asarray(bound, f64), err.shape)
    with np.errstate(divide='ignore', invalid='ignore'):
      over = float(np.where(err > 0, err / bound, 0.0).max())
    frac, ok = float(np.mean(err > bound)), bool(np.all(err <= bound))
  return dict(max_over_bound=over, frac_over=frac, rms=rms, rms_seq=rms_seq,
              rms_ratio=rms / rms_seq if rms_seq > 0 else (0.0 if rms == 0 else np.inf),
              ok_bound=ok, ok_rms=bool(rms <= lc.RMS_MARGIN * rms_seq))


# ---- the HVP's product stages ----------------------------------------------

STAGES = ('ty1', 'ty2', 'ty3', 'hsum', 'hdot', 'td3', 'td2', 'td1',
          'hq conv1 w', 'hq conv1 b', 'hq conv2 w', 'hq conv2 b', 'hq conv3 w', 'hq conv3 b', 'hq fc1 w')
TANGENTS = STAGES[:8]
SHAPES = dict(ty1=(1, 20, 20, 32), ty2=(1, 9, 9, 64), ty3=(1, 7, 7, 64), hsum=(1, 512), hdot=(1, 512),
              td4=(1, 512), td3=(1, 7, 7, 64), td2=(1, 9, 9, 64), td1=(1, 20, 20, 32))


def _w(tree, i, leaf='w'):
  a = np.asarray(tree[C[i]][leaf], f64)
  return a.reshape(-1, a.shape[-1]) if leaf == 'w' else a


def _rows(x):
  x = np.asarray(x, f64)
  return x.reshape(-1, x.shape[-1])


def ops(name, I):
  """Operands of product stage `name`: SimpleNamespace(a, w, b, mask, k,
  shape) with value = mask * (a @ w + b).  I: dict with x0 [1,84,84,4]
  (pixels / 255), the primal y1, y2, y3 (NHWC, one sample), h [1,512], the
  unit-cotangent backward signals d1 .. d4 in the same shapes, th (theta')
  and tw (the tangent w) as trees, and the tangents of the stages before
  (ty1 .., hpart [196,512] or hsum, td4 ..).  Dropping a term (the damaged
  stages of the CPU test) is I['drop'] = the stage's name: its `ydot (x) d`
  or `W ydot` half is zeroed."""
  th, tw = I['th'], I['tw']
  drop = I.get('drop') == name
  b = mask = k = None
  if name == 'ty1':
    a, w, b, mask = lc.conv_cols(I['x0'], 0), _w(tw, 0), _w(tw, 0, 'b'), I['y1']
  elif name in ('ty2', 'ty3'):
    i = int(name[2]) - 1
    y, ty = I['y%d' % i], I['ty%d' % i]
    a = np.concatenate([lc.conv_cols(y, i), lc.conv_cols(ty, i) * (0.0 if drop else 1.0)], axis=1)
    w, b, mask = np.concatenate([_w(tw, i), _w(th, i)]), _w(tw, i, 'b'), I['y%d' % (i + 1)]
  elif name == 'hsum':  # the fc1 tangent pre-activation without its bias: sum of the K-chunk partials
    a = np.concatenate([_rows(I['y3']).reshape(1, -1), _rows(I['ty3']).reshape(1, -1)], axis=1)
    w = np.concatenate([np.asarray(tw[FC1]['w'], f64), np.asarray(th[FC1]['w'], f64)])
  elif name == 'hdot':  # hvp_g_hidden: mask(h) (bdot1 + sum of the 196 chunk partials)
    part = np.asarray(I['hpart'], f64) if 'hpart' in I else np.asarray(I['hsum'], f64).reshape(1, -1)
    a = np.ones((1, part.shape[0] + 1))
    w, mask = np.concatenate([part, np.asarray(tw[FC1]['b'], f64)[None]]), I['h']
  elif name == 'td3':
    a = np.concatenate([_rows(I['d4']), _rows(I['td4'])], axis=1)
    w = np.concatenate([np.asarray(tw[FC1]['w'], f64).T, np.asarray(th[FC1]['w'], f64).T])
    mask = I['y3']
  elif name in ('td2', 'td1'):
    i = int(name[2])  # the conv layer above: td_i comes through conv i + 1's weights (index i)
    d, dd = np.asarray(I['d%d' % (i + 1)], f64), np.asarray(I['td%d' % (i + 1)], f64).reshape(I['d%d' % (i + 1)].shape)
    a0, w0, k0 = lc.conv_dx_operands(d, np.asarray(tw[C[i]]['w'], f64), i)
    a1, w1, _ = lc.conv_dx_operands(dd, np.asarray(th[C[i]]['w'], f64), i)
    a, w, k, mask = np.concatenate([a0, a1], axis=1), np.concatenate([w0, w1]), 2 * k0, I['y%d' % i]
  elif name == 'hq conv1 w':
    a, w = lc.conv_cols(I['x0'], 0).T, _rows(I['td1'])
  elif name in ('hq conv2 w', 'hq conv3 w'):
    i = int(name[7]) - 1
    a = np.concatenate([lc.conv_cols(I['ty%d' % i], i).T * (0.0 if drop else 1.0), lc.conv_cols(I['y%d' % i], i).T],
                       axis=1)
    w = np.concatenate([_rows(I['d%d' % (i + 1)]), _rows(I['td%d' % (i + 1)])])
  elif name in ('hq conv1 b', 'hq conv2 b', 'hq conv3 b'):
    w = _rows(I['td%s' % name[7]])
    a = np.ones((1, w.shape[0]))
  elif name == 'hq fc1 w':
    a = np.stack([_rows(I['ty3']).reshape(-1) * (0.0 if drop else 1.0), _rows(I['y3']).reshape(-1)], axis=1)
    w = np.concatenate([_rows(I['d4']), _rows(I['td4'])])
  else:
    raise KeyError(name)
  if mask is not None:
    mask = _rows(mask).reshape(a.shape[0], -1) > 0
    if I.get('no_mask') == name:
      mask = None
  return types.SimpleNamespace(a=a, w=w, b=b, mask=mask, k=k)


def td4(I, dtype=f64):
  """ddot4 = (h > 0) Wdot2[:, a]: a gather and a mask, exact in any format."""
  col = np.asarray(I['tw'][FC2]['w'], dtype)[:, I['act']]
  return np.where(np.asarray(I['h']).reshape(-1) > 0, col, dtype(0.0))[None]  # (not col * mask: that leaves -0.0)


def evaluate(name, I, dtype=f64):
  """The stage's value in `dtype` arithmetic (numpy's own product order)."""
  o = ops(name, I)
  r = np.asarray(o.a, dtype) @ np.asarray(o.w, dtype)
  if o.b is not None:
    r = r + np.asarray(o.b, dtype)
  if o.mask is not None:
    r = r * o.mask
  assert r.dtype == dtype
  return r.reshape(SHAPES.get(name, r.shape))


def chain(I, dtype=f64, stages=STAGES):
  """Every product stage in order, each from the values of the ones before
  (and td4); returns I extended with them."""
  I = dict(I)
  I['td4'] = td4(I, dtype)
  for name in stages:
    I[name] = evaluate(name, I, dtype)
  return I


def check(name, got, I):
  o = ops(name, I)
  return lc.product_check(got, o.a, o.w, o.b, k_terms=o.k, mask=o.mask)


def hq_tree(I):
  """H_q w as a tree, from a chain's values (fc2 w: column a = hdot; fc1 b =
  ddot4; fc2 b = 0)."""
  a = I['act']
  f2 = np.zeros(np.shape(I['tw'][FC2]['w']), np.asarray(I['hdot']).dtype)
  f2[:, a] = np.asarray(I['hdot']).reshape(-1)
  out = {FC1: {'w': I['hq fc1 w'], 'b': np.asarray(I['td4']).reshape(-1)},
         FC2: {'w': f2, 'b': np.zeros(f2.shape[1], f2.dtype)}}
  for i in range(3):
    out[C[i]] = {'w': np.asarray(I['hq conv%d w' % (i + 1)]).reshape(np.shape(I['tw'][C[i]]['w'])),
                 'b': np.asarray(I['hq conv%d b' % (i + 1)]).reshape(-1)}
  return out


# ---- v = v_dir + J (alpha s1 gq - clip hq) ------------------------------------

def combine_f(vd, j, gq, a_s1, clip, hq, dtype):
  vd, j, gq, hq = (np.asarray(x, dtype).reshape(-1) for x in (vd, j, gq, hq))
  r = vd + j * (dtype(a_s1) * gq - dtype(clip) * hq)
  assert r.dtype == dtype
  return r


def alpha_clip(td, bound, s1, alpha_one=False):
  """(alpha s1, clip(td')) as HqOut forms them; alpha_one: the damaged form
  that keeps alpha = 1 outside the clip bound."""
  td, bound = float(td), float(f32(bound))
  return (float(s1) if (abs(td) < bound or alpha_one) else 0.0), float(np.clip(td, -bound, bound))


def combine_check(got, vd, j, gq, a_s1, clip, o=None, hq=None):
  """One leaf (or part of one) of v.  o: the product operands of its H_q w
  (ops(...)), or hq: an H_q w that involves no arithmetic (zeros, ddot4)."""
  if o is not None:
    a64, w64 = np.asarray(o.a, f64), np.asarray(o.w, f64)
    hq64 = (a64 @ w64).reshape(-1)
    k = a64.shape[1] if o.k is None else o.k
    hq_bound = ((k + 3) * U * (np.abs(a64) @ np.abs(w64))).reshape(-1)
    hq_seq = lc.seq_f32(o.a, o.w).reshape(-1)
    if o.mask is not None:
      m = o.mask.reshape(-1)
      hq64, hq_seq = hq64 * m, hq_seq * m
  else:
    hq64 = np.asarray(hq, f64).reshape(-1)
    hq_bound, hq_seq = 0.0, hq64.astype(f32)
  ref = combine_f(vd, j, gq, a_s1, clip, hq64, f64)
  vd64, j64, gq64 = (np.abs(np.asarray(x, f64).reshape(-1)) for x in (vd, j, gq))
  t = np.abs(a_s1) * gq64 + np.abs(clip) * np.abs(hq64)
  bound = j64 * np.abs(clip) * hq_bound + U * (vd64 + 5.0 * j64 * t)
  seq = combine_f(vd, j, gq, a_s1, clip, hq_seq, f32).astype(f64)
  return result(np.abs(np.asarray(got, f64).reshape(-1) - ref), bound, seq - ref)


def v_rows(got_v, I, vd, j, gq, a_s1, clip):
  """combine_check of every leaf of the device's v (trees of the device's
  v_dir, J, grad q; I: the device's tangents), fc2 w split into the taken
  action's column (H_q w = hdot) and the others (H_q w = 0)."""
  a = I['act']
  rows = []

  def leaf(t, mod, name):
    return np.asarray(t[mod][name])

  for label, (mod, name) in zip(LEAF_LABEL, LEAVES):
    args = [leaf(t, mod, name) for t in (got_v, vd, j, gq)]
    if label == 'fc2 w':
      col = [x[:, a] for x in args]
      rows.append(('v fc2 w[:, a]', combine_check(*col, a_s1, clip, o=ops('hdot', I))))
      rest = [np.delete(x, a, axis=1) for x in args]
      rows.append(('v fc2 w[:, not a]', combine_check(*rest, a_s1, clip, hq=np.zeros(rest[0].size))))
    elif label == 'fc2 b':
      rows.append(('v fc2 b', combine_check(*args, a_s1, clip, hq=np.zeros(args[0].size))))
    elif label == 'fc1 b':
      rows.append(('v fc1 b', combine_check(*args, a_s1, clip, hq=I['td4'])))
    else:
      rows.append(('v ' + label, combine_check(*args, a_s1, clip, o=ops('hq ' + label, I))))
  return rows


# ---- dot products --------------------------------------------------------------

def dot_check(got, a, b, k_terms=None, b_mag=None):
  """got [n] ~ sum_k a[n, k] b[n or 1, k], both bars.  b_mag: the magnitude
  b's own rounding is relative to, where b is itself computed (>= |b|)."""
  a64, b64 = np.atleast_2d(np.asarray(a, f64)), np.atleast_2d(np.asarray(b, f64))
  k = a64.shape[1] if k_terms is None else k_terms
  ref = (a64 * b64).sum(axis=1)
  bm = np.abs(b64) if b_mag is None else np.atleast_2d(np.asarray(b_mag, f64))
  bound = (k + 3) * U * (np.abs(a64) * bm).sum(axis=1)
  prod = np.atleast_2d(np.asarray(a, f32)) * np.atleast_2d(np.asarray(b, f32))
  seq = np.cumsum(prod, axis=1, dtype=f32)[:, -1].astype(f64)
  return result(np.abs(np.asarray(got, f64).reshape(-1) - ref), bound, seq - ref)


def dlogits_check(got, s, p):
  s64, p64 = np.asarray(s, f64), np.asarray(p, f64)
  tot = s64.sum()
  ref = s64 - p64 * tot
  bound = U * (p64 * (s64.size - 1) * np.abs(s64).sum() + np.abs(s64) + 2 * p64 * abs(tot))
  s32, p32 = np.asarray(s, f32), np.asarray(p, f32)
  seq = (s32 - p32 * np.cumsum(s32, dtype=f32)[-1]).astype(f64)
  return result(np.abs(np.asarray(got, f64) - ref), bound, seq - ref)


# ---- the RMSProp stages ----------------------------------------------------------

class Consts:
  """The optimizer constants as the device holds them (dqz_meta_config's
  floats; c1 = (float)(1.0 - (double)decay))."""

  def __init__(self, lr=2.5e-4, decay=0.95, eps=0.01 / 32**2):
    self.lr, self.decay, self.eps = f32(lr), f32(decay), f32(eps)
    self.c1 = f32(1.0 - float(self.decay))

  def cast(self, dtype):
    return dtype(self.lr), dtype(self.decay), dtype(self.c1), dtype(self.eps)


def meta1(g, th, mu, nu, k, dtype=f64):
  """(theta', mu', nu', J) of Rms::meta1 / meta_rms1_kernel."""
  g, th, mu, nu = (np.asarray(x, dtype) for x in (g, th, mu, nu))
  lr, d, c1, eps = k.cast(dtype)
  m = c1 * g + d * mu
  v = c1 * (g * g) + d * nu
  dd = v - m * m + eps
  rs = dtype(1.0) / np.sqrt(dd)
  thp = th + (-lr) * (g * rs)
  j = -lr * (dd - c1 * g * (g - m)) * (rs * rs * rs)
  assert thp.dtype == dtype and j.dtype == dtype
  return thp, m, v, j


def meta3(gq, big_g, mu, nu, td, bound, k, dtype=f64):
  """(v_dir, w) of Rms::meta3 from grad q, G, the learner's mu, nu (mu', nu'
  are restated: the second order overwrites the device's) and td'."""
  gq, big_g, mu, nu = (np.asarray(x, dtype) for x in (gq, big_g, mu, nu))
  lr, d, c1, eps = k.cast(dtype)
  mu1, nu1 = c1 * big_g + d * mu, c1 * (big_g * big_g) + d * nu
  clip = dtype(np.clip(float(td), -float(f32(bound)), float(f32(bound))))
  g = -clip * gq
  m = c1 * g + d * mu1
  v = c1 * (g * g) + d * nu1
  d2 = v - m * m + eps
  rs = dtype(1.0) / np.sqrt(d2)
  rs3 = rs * rs * rs
  u = (-lr) * (g * rs)
  vdir = dtype(2.0) * u * c1 * d * lr * g * rs3 * (big_g - m)
  w = dtype(2.0) * u * (-lr) * rs3 * (d2 - c1 * g * (g - m))
  assert vdir.dtype == dtype and w.dtype == dtype
  return vdir, w


def meta2(g, mu1, nu1, j, k, dtype=f64):
  """v = -2 u' J of Rms::meta2 (first order)."""
  g, mu1, nu1, j = (np.asarray(x, dtype) for x in (g, mu1, nu1, j))
  lr, d, c1, eps = k.cast(dtype)
  m = c1 * g + d * mu1
  v = c1 * (g * g) + d * nu1
  u = (-lr) * (g * (dtype(1.0) / np.sqrt(v - m * m + eps)))
  return dtype(-2.0) * u * j


def restated_check(got, ref64, ref32):
  """The 4 x bar alone (stages that call rsqrtf, see the module docstring)."""
  ref64 = np.asarray(ref64, f64)
  return result(np.abs(np.asarray(got, f64) - ref64), None, np.asarray(ref32, f64) - ref64)


def moments_check(got_mu, got_nu, g, mu, nu, k):
  """mu', nu' of Rms::meta1 with their a-priori bounds."""
  g, mu, nu = (np.asarray(x, f64) for x in (g, mu, nu))
  _, m64, v64, _ = meta1(g, 0 * g, mu, nu, k)
  _, m32, v32, _ = meta1(g, 0 * g, mu, nu, k, f32)
  c1, d = float(k.c1), float(k.decay)
  bm = 3 * U * (np.abs(c1 * g) + np.abs(d * mu))
  bv = 4 * U * (c1 * g * g + d * np.abs(nu))
  return [('mu1', result(np.abs(np.asarray(got_mu, f64) - m64), bm, m32 - m64)),
          ('nu1', result(np.abs(np.asarray(got_nu, f64) - v64), bv, v32 - v64))]


# ---- the meta batch's side: G, the tangent forward, s_i ---------------------------

def head_cotangent(q0, q1, action, reward, discount, p, bound, dtype=f64):
  """The batch head's cotangent at q_i[a_i], -p_i clip(td_i), from the
  device's q arrays, and the magnitude its rounding is relative to."""
  idx = np.arange(len(action))
  q0, q1 = np.asarray(q0, dtype), np.asarray(q1, dtype)
  r, d, p = np.asarray(reward, dtype), np.asarray(discount, dtype), np.asarray(p, dtype)
  v, qa = q1.max(axis=1), q0[idx, action]
  td = (r + d * v) - qa
  b = dtype(f32(bound))
  g = -p * np.clip(td, -b, b)
  return g, td, np.abs(p) * (np.abs(r) + np.abs(d * v) + np.abs(qa))


def sample_grad(x, act, i, gq_i, a_i, num_actions, gq_mag_i=None):
  """p_i g_i of sample i as a flat list of leaves in LEAVES order (fp64) and
  the same with every factor's magnitude, from the batch learner's arrays
  (dy already carry p_i) and the pixels x [M,84,84,4] / 255.  The fc2 leaves
  use the self-formed cotangent gq_i (gq_mag_i: what its rounding is
  relative to)."""
  out, mag = [], []
  gq_mag_i = abs(gq_i) if gq_mag_i is None else gq_mag_i
  prev = np.asarray(x[i:i + 1], f64)
  for l in range(3):
    cols = lc.conv_cols(prev, l)
    dy = _rows(act['dy%d' % (l + 1)][i])
    out += [cols.T @ dy, dy.sum(axis=0)]
    mag += [np.abs(cols).T @ np.abs(dy), np.abs(dy).sum(axis=0)]
    prev = np.asarray(act['y%d' % (l + 1)][i:i + 1], f64)
  y3, dz1, h1 = prev.reshape(-1), np.asarray(act['dz1'][i], f64), np.asarray(act['h1'][i], f64)
  out += [np.outer(y3, dz1), dz1]
  mag += [np.outer(np.abs(y3), np.abs(dz1)), np.abs(dz1)]
  w2, b2 = np.zeros((512, num_actions)), np.zeros(num_actions)
  w2[:, a_i], b2[a_i] = h1 * gq_i, gq_i
  w2m, b2m = np.zeros_like(w2), np.zeros_like(b2)
  w2m[:, a_i], b2m[a_i] = np.abs(h1) * gq_mag_i, gq_mag_i
  out += [w2, b2]
  mag += [w2m, b2m]
  return [o.reshape(-1) for o in out], [m.reshape(-1) for m in mag]


# ---- one second-order update, stage by stage ------------------------------------

def backward_signals(params, act, dq, dtype=f64):
  """d loss / d pre-activation of every layer for the cotangent dq [B,A] at
  q, each multiplied by its ReLU mask (act: y1, y2, y3 NHWC and h1): dict
  dz1 [B,512], dy3, dy2, dy1."""
  n = dq.shape[0]
  out = {'dz1': (np.asarray(dq, dtype) @ np.asarray(params[FC2]['w'], dtype).T) * (act['h1'] > 0)}
  d = (out['dz1'] @ np.asarray(params[FC1]['w'], dtype).T) * (act['y3'].reshape(n, -1) > 0)
  out['dy3'] = d.reshape(act['y3'].shape)
  for l in (2, 1):
    a, wf, _ = lc.conv_dx_operands(out['dy%d' % (l + 1)], np.asarray(params[C[l]]['w'], dtype), l)
    y = act['y%d' % l]
    out['dy%d' % l] = ((a @ wf).reshape(y.shape) * (y > 0)).astype(dtype)
  return out


def grad_leaves(x, act, sig, dq, dtype=f64):
  """The gradient tree of sum(dq * q) from the signals of backward_signals
  (summed over the batch)."""
  n = dq.shape[0]
  out = {}
  prev = np.asarray(x, dtype)
  for l in range(3):
    dy = _rows(sig['dy%d' % (l + 1)]).astype(dtype)
    cols = lc.conv_cols(prev, l).astype(dtype)
    out[C[l]] = {'w': (cols.T @ dy).reshape(CONV_SHAPES[l]), 'b': dy.sum(axis=0)}
    prev = act['y%d' % (l + 1)]
  out[FC1] = {'w': act['y3'].reshape(n, -1).astype(dtype).T @ sig['dz1'], 'b': sig['dz1'].sum(axis=0)}
  out[FC2] = {'w': act['h1'].astype(dtype).T @ np.asarray(dq, dtype), 'b': np.asarray(dq, dtype).sum(axis=0)}
  return out


CONV_SHAPES = tuple((k, k, ci, co) for k, _, ci, co in learner_ref.CONV_SPECS)


def tmap(f, *trees):
  return {m: {n: f(*(t[m][n] for t in trees)) for n in trees[0][m]} for m in trees[0]}


def tcat(tree, dtype=None):
  """The leaves in LEAVES order as one vector."""
  return np.concatenate([np.asarray(tree[m][n], dtype).reshape(-1) for m, n in LEAVES])


def forward_act(params, s, dtype):
  """The oracle's fp64 forward, its activations cast to dtype (NHWC)."""
  q, cache = learner_ref.forward(params, s)
  act = {'y%d' % (i + 1): cache['y%d' % i].astype(dtype) for i in range(3)}
  act.update(h1=cache['h1'].astype(dtype), q=q.astype(dtype))
  return act


def simulate(case, dtype=f64, consts=None, damage=None, second_order=True):
  """One meta-update (second order, or first) in `dtype` numpy, stage by stage, every
  stage from the stored values of the stages before: the dict of arrays the
  GPU test reads off the device (trees for the [T] buffers).  case: dict of
  host inputs (online, target, mu, nu trees; s_tm1, s_t [M,84,84,4], action,
  reward, discount; logits [M]; ot_tm1, ot_t [84,84,4], oa, o_r, o_d; bound).
  damage: None, ('drop', stage), ('no_mask', stage), 'alpha_one' or 'overlap'
  (ddot1 from theta' with four rows of W2 replaced by the same rows of v)."""
  k = consts or Consts()
  cast = lambda t: tmap(lambda v: np.asarray(v, dtype), t)
  th, mu, nu = cast(case['online']), cast(case['mu']), cast(case['nu'])
  m, a_n = len(case['action']), np.shape(case['online'][FC2]['w'])[1]
  x = np.asarray(case['s_tm1'], dtype) / dtype(255.0)
  lg = np.asarray(case['logits'], dtype)
  p = np.exp(lg - (lg.max() + np.log(np.exp(lg - lg.max()).sum())))
  act = forward_act(case['online'], case['s_tm1'], dtype)
  q1 = forward_act(case['target'], case['s_t'], dtype)['q']
  gq_b, td, _ = head_cotangent(act['q'], q1, case['action'], case['reward'], case['discount'], p, case['bound'], dtype)
  dq = np.zeros((m, a_n), dtype)
  dq[np.arange(m), case['action']] = gq_b
  act.update(backward_signals(th, act, dq, dtype))
  big_g = grad_leaves(x, act, act, dq, dtype)
  m1 = tmap(lambda *v: meta1(*v, k, dtype), big_g, th, mu, nu)
  thp, jac = tmap(lambda v: v[0], m1), tmap(lambda v: v[3], m1)
  # the one transition at theta' (target: theta)
  x1 = np.asarray(case['ot_tm1'][None], dtype) / dtype(255.0)
  act1 = forward_act(thp, case['ot_tm1'][None], dtype)
  qt = forward_act(case['online'], case['ot_t'][None], dtype)['q']
  td1 = (dtype(case['o_r']) + dtype(case['o_d']) * qt.max()) - act1['q'][0, case['oa']]
  e_a = np.zeros((1, a_n), dtype)
  e_a[0, case['oa']] = 1
  if not second_order:  # v = -2 u'(g') J, g' the loss gradient of the one transition (batch of one)
    b = dtype(f32(case['bound']))
    dq1 = -np.clip(td1, -b, b) * e_a
    act1.update(backward_signals(thp, act1, dq1, dtype))
    g_p = grad_leaves(x1, act1, act1, dq1, dtype)
    v = tmap(lambda g, mm, nn, j: meta2(g, mm[1], mm[2], j, k, dtype), g_p, m1, m1, jac)
    return dict(G=v, thp=thp, J=jac, mu1=tmap(lambda t: t[1], m1), nu1=tmap(lambda t: t[2], m1), p=p, act=act,
                q1=q1, act1=act1, tdp=td1, big_g=big_g)
  act1.update(backward_signals(thp, act1, e_a, dtype))
  gq = grad_leaves(x1, act1, act1, e_a, dtype)
  m3 = tmap(lambda g, gg, mm, nn: meta3(g, gg, mm, nn, td1, case['bound'], k, dtype), gq, big_g, mu, nu)
  vdir, w = tmap(lambda v: v[0], m3), tmap(lambda v: v[1], m3)
  s1 = (tcat(gq) * tcat(w)).sum(dtype=dtype)
  I = dict(x0=x1, y1=act1['y1'], y2=act1['y2'], y3=act1['y3'], h=act1['h1'], d1=act1['dy1'], d2=act1['dy2'],
           d3=act1['dy3'], d4=act1['dz1'], th=thp, tw=w, act=case['oa'])
  if isinstance(damage, tuple):
    I[damage[0]] = damage[1]
  a_s1, clip = alpha_clip(td1, case['bound'], s1, alpha_one=damage == 'alpha_one')
  if damage == 'overlap':
    I = chain(I, dtype, STAGES[:STAGES.index('td1')])
    v2 = combine_f(vdir[C[1]]['w'], jac[C[1]]['w'], gq[C[1]]['w'], a_s1, clip, evaluate('hq conv2 w', I, dtype), dtype)
    bad = {mod: dict(d) for mod, d in thp.items()}
    bad[C[1]]['w'] = thp[C[1]]['w'].copy()
    bad[C[1]]['w'].reshape(-1, 64)[200:204] = v2.reshape(-1, 64)[200:204]
    I['td1'] = evaluate('td1', dict(I, th=bad), dtype)
    I = chain(I, dtype, STAGES[STAGES.index('td1') + 1:]) | {'td4': I['td4']}
  else:
    I = chain(I, dtype)
  hq = hq_tree(I)
  v = tmap(lambda vd, j, g, h: combine_f(vd, j, g, a_s1, clip, h, dtype).reshape(np.shape(vd)), vdir, jac, gq, hq)
  vflat = tcat(v)
  s = np.zeros(m, dtype)
  for i in range(m):
    g_i, _ = sample_grad(x, act, i, gq_b[i], case['action'][i], a_n)
    s[i] = (vflat * np.concatenate(g_i).astype(dtype)).sum(dtype=dtype)
  dl = s - p * s.sum(dtype=dtype)
  out = dict(G=big_g, thp=thp, J=jac, mu1=vdir, nu1=w, GQ=gq, HQ=v, s1=s1, p=p, s=s, dlogits=dl, act=act,
             q1=q1, act1=act1, tdp=td1, hq=hq, hpart=np.asarray(I['hsum']).reshape(1, -1))
  out.update({n: I[n] for n in ('ty1', 'ty2', 'ty3', 'td4', 'td3', 'td2', 'td1')})
  return out


def one_transition_inputs(case, D):
  """ops' input dict from a device-like dict D (simulate's, or the GPU's)."""
  a1 = D['act1']
  I = dict(x0=np.asarray(case['ot_tm1'][None], f64) / 255.0, y1=a1['y1'], y2=a1['y2'], y3=a1['y3'], h=a1['h1'],
           d1=a1['dy1'], d2=a1['dy2'], d3=a1['dy3'], d4=a1['dz1'], th=D['thp'], tw=D['nu1'], act=case['oa'],
           hpart=D['hpart'])
  I.update({n: np.asarray(D[n]).reshape(SHAPES[n]) for n in ('ty1', 'ty2', 'ty3', 'td4', 'td3', 'td2', 'td1')})
  return I


def leaf_rows(prefix, f):
  return [('%s %s' % (prefix, lab), f(m, n)) for lab, (m, n) in zip(LEAF_LABEL, LEAVES)]


def second_order_rows(case, D, consts=None, batch_side=True):
  """Every stage of a second-order update from the device-like dict D's own
  values: list of (name, result).  batch_side False (a chunked meta batch):
  without G from the batch learner and s, which the caller checks from the
  last chunk."""
  k = consts or Consts()
  m = len(case['action'])
  a_n = np.shape(case['online'][FC2]['w'])[1]
  rows = []
  act, x = D['act'], None
  if batch_side:
    x = np.asarray(case['s_tm1'], f64) / 255.0
    # G per leaf from the batch learner's p-weighted dy and its y arrays
    prev = x
    for l in range(3):
      dy = _rows(act['dy%d' % (l + 1)])
      rows.append(('G conv%d w' % (l + 1), lc.product_check(D['G'][C[l]]['w'], lc.conv_cols(prev, l).T, dy)))
      rows.append(('G conv%d b' % (l + 1), lc.product_check(D['G'][C[l]]['b'], np.ones((1, dy.shape[0])), dy)))
      prev = act['y%d' % (l + 1)]
    rows.append(('G fc1 w', lc.product_check(D['G'][FC1]['w'], act['y3'].reshape(m, -1).T, act['dz1'])))
    rows.append(('G fc1 b', lc.product_check(D['G'][FC1]['b'], np.ones((1, m)), act['dz1'])))
    hc = [head_cotangent(act['q'], D['q1'], case['action'], case['reward'], case['discount'], D['p'], case['bound'], t)
          for t in (f64, f32)]
    dq, dq32, dq_mag = (np.zeros((m, a_n), t) for t in (f64, f32, f64))
    idx = np.arange(m)
    dq[idx, case['action']], dq32[idx, case['action']], dq_mag[idx, case['action']] = hc[0][0], hc[1][0], hc[0][2]
    kw = dict(k_terms=m + 8, w_mag=dq_mag, w_seq=dq32)
    rows.append(('G fc2 w', lc.product_check(D['G'][FC2]['w'], act['h1'].T, dq, **kw)))
    rows.append(('G fc2 b', lc.product_check(D['G'][FC2]['b'], np.ones((1, m)), dq, **kw)))
  # theta', J from G, theta, mu, nu; v_dir, w from G, grad q, td' (4 x bar alone: rsqrtf)
  on, mu, nu = case['online'], case['mu'], case['nu']
  m1 = {t: tmap(lambda *v: meta1(*v, k, t), D['G'], on, mu, nu) for t in (f64, f32)}
  rows += leaf_rows("theta'", lambda a, b: restated_check(D['thp'][a][b], m1[f64][a][b][0], m1[f32][a][b][0]))
  rows += leaf_rows('J', lambda a, b: restated_check(D['J'][a][b], m1[f64][a][b][3], m1[f32][a][b][3]))
  m3 = {t: tmap(lambda g, gg, mm, nn: meta3(g, gg, mm, nn, D['tdp'], case['bound'], k, t), D['GQ'], D['G'], mu, nu)
        for t in (f64, f32)}
  rows += leaf_rows('v_dir', lambda a, b: restated_check(D['mu1'][a][b], m3[f64][a][b][0], m3[f32][a][b][0]))
  rows += leaf_rows('w', lambda a, b: restated_check(D['nu1'][a][b], m3[f64][a][b][1], m3[f32][a][b][1]))
  rows.append(('s1', dot_check(D['s1'], tcat(D['GQ']), tcat(D['nu1']))))
  # the HVP chain, every stage from the device's own tangents
  I = one_transition_inputs(case, D)
  for name in TANGENTS:
    if name == 'hsum':
      rows.append(('sum hpart', check('hsum', np.asarray(D['hpart'], f64).sum(axis=0), I)))
    elif name != 'hdot':  # hdot is not stored: it is v's fc2 column a (v_rows)
      rows.append((name, check(name, D[name], I)))
  a_s1, clip = alpha_clip(D['tdp'], case['bound'], D['s1'])
  rows += v_rows(D['HQ'], I, D['mu1'], D['J'], D['GQ'], a_s1, clip)
  if batch_side:
    gq_b, _, gq_mag = hc[0]
    vflat = tcat(D['HQ'], f64)
    g, gm = zip(*(sample_grad(x, act, i, gq_b[i], case['action'][i], a_n, gq_mag[i]) for i in range(m)))
    rows.append(('s', dot_check(D['s'], vflat[None], np.stack([np.concatenate(v) for v in g]),
                                k_terms=vflat.size + 400 + 8, b_mag=np.stack([np.concatenate(v) for v in gm]))))
  rows.append(('dlogits', dlogits_check(D['dlogits'], D['s'][:m], D['p'][:m])))
  return rows


def theta_rows(case, D, consts=None):
  """thp against theta' = theta + u(G; mu, nu) restated from the device's G
  (second_order_rows' `theta'` rows alone): after a second-order update thp
  still holds theta' (v goes to HQ)."""
  k = consts or Consts()
  m1 = {t: tmap(lambda *v: meta1(*v, k, t)[0], D['G'], case['online'], case['mu'], case['nu']) for t in (f64, f32)}
  return leaf_rows("theta'", lambda a, b: restated_check(D['thp'][a][b], m1[f64][a][b], m1[f32][a][b]))


def td4_exact(case, D):
  """ddot4 is a gather and a mask: bit equality.  Returns the number of
  elements whose bits differ and, of those, how many differ in value too."""
  want = td4(dict(tw=D['nu1'], act=case['oa'], h=D['act1']['h1']), f32).reshape(-1)
  got = np.asarray(D['td4'], f32).reshape(-1)
  return int(np.count_nonzero(got.view(np.uint32) != want.view(np.uint32))), int(np.count_nonzero(got != want))


def meta_case(bound, meta_batch, a, kink_free=False):
  """The host inputs of tests/test_meta_gpu.py's
  test_second_order_meta_update_matches_oracle (same seeds, same online
  action), as simulate's `case` plus what the device needs (store contents,
  slots, full logit buffer, positions).  kink_free: the slots are drawn by
  helpers.kink_free_slots (seed 56) instead, for comparisons with the
  unpinned fp64 oracle."""
  from dqn_mgsc_zoo_amd import networks  # pylint: disable=g-import-not-at-top
  from tests import helpers  # pylint: disable=g-import-not-at-top
  net = networks.dqn_atari_network(a)
  online = net.init(51)
  target = helpers.perturbed_tree(online, 52)
  rng = np.random.default_rng(53)
  mu = {m: {n: (1e-3 * rng.standard_normal(np.shape(v))).astype(f32) for n, v in d.items()}
        for m, d in online.items()}
  nu = {m: {n: (mu[m][n].astype(f64)**2 + 1e-6 * rng.random(np.shape(v))).astype(f32) for n, v in d.items()}
        for m, d in mu.items()}
  rng = np.random.default_rng(54)
  capacity = max(128, 2 * meta_batch)
  frames, fidx, action, reward, discount = helpers.random_store_contents(capacity, 2 * capacity + 64, a, 55)
  slots = rng.choice(capacity, meta_batch, replace=False).astype(np.int32)
  logits = rng.standard_normal(max(64, 2 * meta_batch)).astype(f32)
  pos = rng.choice(logits.size, meta_batch, replace=False).astype(np.int32)
  ot_tm1 = rng.integers(0, 256, (84, 84, 4), dtype=np.uint8)
  ot_t = rng.integers(0, 256, (84, 84, 4), dtype=np.uint8)
  if kink_free:
    slots = helpers.kink_free_slots(online, dict(frames=frames, fidx=fidx), capacity, meta_batch,
                                    np.random.default_rng(56))
  return dict(net=net, online=online, target=target, mu=mu, nu=nu, bound=bound,
              store=dict(frames=frames, fidx=fidx, action=action, reward=reward, discount=discount),
              capacity=capacity, slots=slots, all_logits=logits, pos=pos, logits=logits[pos],
              s_tm1=helpers.stacks_from(frames, fidx, slots, 0), s_t=helpers.stacks_from(frames, fidx, slots, 1),
              action=action[slots].astype(np.int64), reward=reward[slots], discount=discount[slots],
              ot_tm1=ot_tm1, ot_t=ot_t, oa=2 if a == 6 else 13, o_r=1.0, o_d=0.99)


# ---- first order; a chunked meta batch ---------------------------------------------

def product_parts(a, w, k_terms=None, w_mag=None, w_seq=None):
  """(fp64 product, its a-priori float32 bound, seq_f32's product), the pieces
  of layer_checks.product_check."""
  a64, w64 = np.asarray(a, f64), np.asarray(w, f64)
  k = a64.shape[1] if k_terms is None else k_terms
  mag = np.abs(a64) @ (np.abs(w64) if w_mag is None else np.asarray(w_mag, f64))
  return a64 @ w64, (k + 3) * U * mag, lc.seq_f32(a, w if w_seq is None else w_seq).astype(f64)


def g_from_batch(case, D):
  """G per leaf from the batch learner's p-weighted dy and its y arrays: trees
  of (fp64 value, a-priori bound of a float32 product, seq_f32's value)."""
  m, a_n = len(case['action']), np.shape(case['online'][FC2]['w'])[1]
  act = D['act']
  out = {}
  prev = np.asarray(case['s_tm1'], f64) / 255.0
  for l in range(3):
    dy = _rows(act['dy%d' % (l + 1)])
    out[C[l]] = {'w': product_parts(lc.conv_cols(prev, l).T, dy), 'b': product_parts(np.ones((1, dy.shape[0])), dy)}
    prev = act['y%d' % (l + 1)]
  out[FC1] = {'w': product_parts(act['y3'].reshape(m, -1).T, act['dz1']),
              'b': product_parts(np.ones((1, m)), act['dz1'])}
  hc = [head_cotangent(act['q'], D['q1'], case['action'], case['reward'], case['discount'], D['p'], case['bound'], t)
        for t in (f64, f32)]
  dq, dq32, dq_mag = (np.zeros((m, a_n), t) for t in (f64, f32, f64))
  idx = np.arange(m)
  dq[idx, case['action']], dq32[idx, case['action']], dq_mag[idx, case['action']] = hc[0][0], hc[1][0], hc[0][2]
  kw = dict(k_terms=m + 8, w_mag=dq_mag, w_seq=dq32)
  out[FC2] = {'w': product_parts(act['h1'].T, dq, **kw), 'b': product_parts(np.ones((1, m)), dq, **kw)}
  shape = lambda t, like: tuple(np.asarray(x).reshape(np.shape(like)) for x in t)
  return tmap(shape, out, case['online'])


def g_from_moment(case, D, consts=None):
  """G recovered from the stored mu' = fl(c g + d mu) (a chunked meta batch
  keeps no G in the first order and the batch learner only its last chunk):
  g = (mu' - d mu) / c in fp64, within the three roundings of mu' divided by
  c.  Same triples as g_from_batch (the float32 value: g rounded)."""
  k = consts or Consts()
  c1, d = float(k.c1), float(k.decay)

  def one(m1, mu):
    m1, mu = np.asarray(m1, f64), np.asarray(mu, f64)
    g = (m1 - d * mu) / c1
    return g, 3 * U * (np.abs(m1) + 2 * np.abs(d * mu)) / c1, g.astype(f32).astype(f64)

  return tmap(one, D['mu1'], case['mu'])


def first_order_rows(case, D, g3, consts=None, with_mu=True):
  """theta', mu', nu', J of Rms::meta1 / meta_rms1_kernel from G (g3: trees of
  (value, bound, float32 value), g_from_batch or g_from_moment) and the
  learner's theta, mu, nu.  mu', nu' carry a-priori bounds (G's own bound
  b(g) goes through them: c b(g), c (2 |g| b(g) + b(g)^2)); theta' and J
  (rsqrtf) the 4 x bar alone."""
  k = consts or Consts()
  c1, d = float(k.c1), float(k.decay)
  rows = []
  on, mu, nu = case['online'], case['mu'], case['nu']
  r64 = tmap(lambda g, *v: meta1(g[0], *v, k), g3, on, mu, nu)
  r32 = tmap(lambda g, *v: meta1(g[2], *v, k, f32), g3, on, mu, nu)
  rows += leaf_rows("theta'", lambda a, b: restated_check(D['thp'][a][b], r64[a][b][0], r32[a][b][0]))

  def moment(a, b, which):
    g, bg, _ = g3[a][b]
    if which == 1:
      bound = c1 * bg + 3 * U * (np.abs(c1 * g) + np.abs(d * np.asarray(mu[a][b], f64)))
    else:
      bound = c1 * (2 * np.abs(g) * bg + bg * bg) + 4 * U * (c1 * g * g + d * np.abs(np.asarray(nu[a][b], f64)))
    got = D['mu1' if which == 1 else 'nu1'][a][b]
    return result(np.abs(np.asarray(got, f64) - r64[a][b][which]), bound, r32[a][b][which] - r64[a][b][which])

  if with_mu:
    rows += leaf_rows("mu'", lambda a, b: moment(a, b, 1))
  rows += leaf_rows("nu'", lambda a, b: moment(a, b, 2))
  rows += leaf_rows('J', lambda a, b: restated_check(D['J'][a][b], r64[a][b][3], r32[a][b][3]))
  return rows


def chunk_rows(case, D, first, n, consts=None):
  """The tangent forward and s of the last chunk's n real samples (global
  indices first .. first + n - 1, chunk-local 0 .. n - 1) of a chunked meta
  batch, from the batch learner's arrays, the device's v (D['v'], a tree) and
  its zv arrays: zv_l = cols(y_{l-1}) @ V_l + vb_l (no ReLU), sum zvp = y3 @
  V_fc1, and s_i = <dy1, zv1> + <dy2, zv2> + <dy3, zv3> + <dz1, vb1 + sum_s
  zvp_s> + gq_i (vb2[a_i] + <h1, V2[:, a_i]>) with gq_i = -p_i clip(td_i)
  formed from the device's q."""
  act, v = D['act'], D['v']
  sl = slice(first, first + n)
  rows = []
  prev = np.asarray(case['s_tm1'][sl], f64) / 255.0
  for l in range(3):
    w = np.asarray(v[C[l]]['w'], f64)
    rows.append(('zv%d' % (l + 1), lc.product_check(D['zv%d' % (l + 1)], lc.conv_cols(prev, l),
                                                    w.reshape(-1, w.shape[-1]), v[C[l]]['b'])))
    prev = act['y%d' % (l + 1)]
  rows.append(('sum zvp', lc.product_check(np.asarray(D['zvp'], f64).sum(axis=0), act['y3'].reshape(n, -1),
                                           v[FC1]['w'])))
  gq, _, gq_mag = head_cotangent(act['q'], D['q1'], case['action'][sl], case['reward'][sl], case['discount'][sl],
                                 D['p'][sl], case['bound'])
  zv, dy, dym = [], [], []
  for i in range(n):
    a_i = case['action'][first + i]
    parts = [D['zv1'][i], D['zv2'][i], D['zv3'][i], v[FC1]['b']] + [D['zvp'][s][i] for s in range(D['zvp'].shape[0])]
    zv.append(np.concatenate([np.asarray(t, f64).reshape(-1) for t in parts] +
                             [[float(v[FC2]['b'][a_i])], np.asarray(v[FC2]['w'], f64)[:, a_i]]))
    dz1, h1 = np.asarray(act['dz1'][i], f64), np.asarray(act['h1'][i], f64)
    sig = [np.asarray(act[t][i], f64).reshape(-1) for t in ('dy1', 'dy2', 'dy3')] + \
        [dz1] * (1 + D['zvp'].shape[0])
    dy.append(np.concatenate(sig + [[gq[i]], gq[i] * h1]))
    dym.append(np.concatenate([np.abs(t) for t in sig] + [[gq_mag[i]], gq_mag[i] * np.abs(h1)]))
  rows.append(('s (last chunk)', dot_check(D['s'][sl], np.stack(zv), np.stack(dy), k_terms=zv[0].size + 8,
                                           b_mag=np.stack(dym))))
  return rows
