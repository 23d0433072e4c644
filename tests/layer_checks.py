"""Per-kernel checks of the learner's layers (tests/test_layers_gpu.py): each
layer, dX and dW product of the network written as one matrix product
`a @ w + b` of the kernel's own inputs, and the two bars a float32
implementation of that product is held to.  Both bars come from the
reference alone, never from the implementation under test:

  * elementwise, |got - ref| <= (K + 3) 2^-24 (|a| @ |w| + |b|): the a-priori
    bound of a K-term float32 dot product in any summation order (each of
    the K products and K - 1 additions rounds once, relative error 2^-24
    each; + 3 for the bias add and the operand conversions of the layer,
    such as x / 255);
  * RMS over the array <= 4 x the RMS error of the same product accumulated
    in float32 in plain sequential order (`seq_f32`).  Sequential order is
    the worst common order (its error grows like sqrt(K), a blocked or
    split-K order's more slowly), so a correct kernel should do no worse;
    4 x absorbs the difference in constants between two random-walk
    estimates.  This sees lost precision (conv1's weights cut to two bf16
    pieces, 16 significant bits, give 41 x the sequential RMS, ten times
    the bar, at 0.26 of the elementwise bound), which the
    elementwise bound is too loose to see.

Large batches.  The forward and dX products are independent per sample, so
at a batch whose fp64 operands would not fit a host budget (conv2 dX at B =
256 is a 102,400 x 1,024 matrix) the caller checks them on
`boundary_samples(B)` only, cutting the kernel's input and output with
`take_samples` before it forms the operands.  The dW and db products sum
over every sample and keep them all; `product_check` then takes K in pieces
(`a` and `w` as equal-length sequences of column blocks of a and row blocks
of w, or a generator of (a_k, w_k) pairs), so the whole operand is never held
at once.  The sequential float32 product carries its accumulator from piece
to piece and is the same bits as the unchunked one.

tests/test_layer_checks_cpu.py runs these checks on numpy's own float32
(BLAS order) and on deliberately damaged products.
"""

import numpy as np

from oracle import learner_ref

EPS = 2.0**-24
RMS_MARGIN = 4.0
f32 = np.float32


def conv_cols(x, layer):
  """im2col of layer's input x [B,H,W,C] -> [B*OH*OW, k*k*C] (HWIO order)."""
  k, st, _, _ = learner_ref.CONV_SPECS[layer]
  c = learner_ref._im2col(np.asarray(x), k, st)  # pylint: disable=protected-access
  return c.reshape(-1, c.shape[-1])


def conv_dx_operands(dz, w, layer):
  """The input gradient of conv `layer` (1 or 2) as one product: returns
  (a [B*H*W, k*k*co], wf [k*k*co, ci], K) with a @ wf = conv_transpose(dz, w)
  flattened over (b, h, w).  dz [B,OH,OW,co] is dilated by the stride,
  padded by k - 1 and gathered with stride 1; wf is w flipped in space with
  ci and co exchanged.  K is the largest number of nonzero terms of one
  output, ceil(k / stride)^2 co (the other columns of a are structural
  zeros)."""
  k, st, ci, co = learner_ref.CONV_SPECS[layer]
  dz = np.asarray(dz)
  b, oh, ow, _ = dz.shape
  dil = np.zeros((b, st * (oh - 1) + 1, st * (ow - 1) + 1, co), dz.dtype)
  dil[:, ::st, ::st, :] = dz
  pad = np.pad(dil, ((0, 0), (k - 1, k - 1), (k - 1, k - 1), (0, 0)))
  a = learner_ref._im2col(pad, k, 1)  # pylint: disable=protected-access
  wf = np.asarray(w)[::-1, ::-1].transpose(0, 1, 3, 2).reshape(k * k * co, ci)
  return a.reshape(-1, k * k * co), wf, (-(-k // st))**2 * co


SUBSET_ABOVE = 64  # batches up to here keep every sample (the chain grid's limit, and the old shapes')


def boundary_samples(batch):
  """The samples on which the per-sample products of a large batch are
  checked: 0 and B - 1, the two either side of every multiple of 16 up to 64
  (the 16-row groups of the MFMA tiles, the 32-row groups of fc1, the chain
  grid's last batch), and the two either side of 128 (the second half of
  MAXB; conv2 / conv3's slab sums change form there) where the batch has
  them.  Sorted, without repeats."""
  want = {0, batch - 1}
  for m in (16, 32, 48, 64, 128):
    want.update((m - 1, m))
  return np.array(sorted(s for s in want if 0 <= s < batch), np.int64)


def sample_subset(batch):
  """Every sample up to SUBSET_ABOVE, boundary_samples(batch) above."""
  return np.arange(batch) if batch <= SUBSET_ABOVE else boundary_samples(batch)


def take_samples(arr, batch, samples):
  """Rows of the chosen samples from an array whose leading axis is
  [batch] or [batch * r] (sample-major), in the same layout."""
  arr = np.asarray(arr)
  r = arr.shape[0] // batch
  assert r * batch == arr.shape[0]
  out = arr.reshape((batch, r) + arr.shape[1:])[np.asarray(samples)]
  return out.reshape((-1,) + arr.shape[1:])


def seq_f32(a, w, b=None, acc=None, last=True):
  """a @ w (+ b) in float32, every output accumulated term by term in index
  order: acc = fl(acc + fl(a_k w_k)), the bias added last.  `acc` continues
  an earlier piece of K (which passed last=False, and so added no bias)."""
  at = np.ascontiguousarray(np.asarray(a, f32).T)
  w = np.asarray(w, f32)
  if acc is None:
    acc = np.zeros((at.shape[1], w.shape[1]), f32)
  for k in range(at.shape[0]):
    acc += at[k][:, None] * w[k][None, :]
  if b is not None and last:
    acc += np.asarray(b, f32)
  return acc


def _pieces(a, w, w_mag, w_seq):
  """(a_k, w_k, w_mag_k, w_seq_k) over K: one piece for plain arrays; for
  sequences of blocks, or a generator of (a_k, w_k) pairs, one per block."""
  if isinstance(a, np.ndarray) and isinstance(w, np.ndarray):
    yield a, w, w_mag, w_seq
  elif w is None:
    assert w_mag is None and w_seq is None
    for ak, wk in a:
      yield ak, wk, None, None
  else:
    assert len(a) == len(w)
    for i, (ak, wk) in enumerate(zip(a, w)):
      yield ak, wk, None if w_mag is None else w_mag[i], None if w_seq is None else w_seq[i]


def product_check(got, a, w, b=None, k_terms=None, mask=None, relu=False, w_mag=None,
                  w_seq=None):
  """Both bars for got ~ (a @ w + b) [* mask, or through a ReLU].  a, w, b
  are the kernel's own inputs (float32 values); the reference is their fp64
  product.  ReLU is 1-Lipschitz, so the bound of the pre-activation holds
  for the activation as well, whichever side of 0 either value falls on.
  An operand the kernel does not read from memory but forms itself (the
  cotangent at q, from the TD error) is given as its fp64 value w, with
  w_mag the magnitude its own rounding is relative to (in place of |w|, and
  k_terms counting its operations too) and w_seq its float32 restatement
  for the sequential product.
  K in pieces: a and w (and w_mag, w_seq where given) as sequences of the
  column blocks of a and the row blocks of w, or a alone as a generator of
  (a_k, w_k) pairs with w=None; the reference and the bound add the pieces
  in fp64, the sequential product carries its accumulator through them.
  Returns dict(max_over_bound, frac_over, rms, rms_seq, rms_ratio, ok_bound,
  ok_rms)."""
  ref = mag = seq = None
  k_all = 0
  for ak, wk, mk, sk in _pieces(a, w, w_mag, w_seq):
    a64, w64 = np.asarray(ak, np.float64), np.asarray(wk, np.float64)
    k_all += a64.shape[1]
    r = a64 @ w64
    m = np.abs(a64) @ (np.abs(w64) if mk is None else np.asarray(mk, np.float64))
    ref, mag = (r, m) if ref is None else (ref + r, mag + m)
    seq = seq_f32(ak, wk if sk is None else sk, acc=seq, last=False)
  k = k_all if k_terms is None else k_terms
  if b is not None:
    ref = ref + np.asarray(b, np.float64)
    mag = mag + np.abs(np.asarray(b, np.float64))
    seq += np.asarray(b, f32)  # the bias last, as seq_f32 adds it
  seq = seq.astype(np.float64)
  if mask is not None:
    m = np.asarray(mask, bool).reshape(ref.shape)
    ref, seq = ref * m, seq * m
  if relu:
    ref, seq = np.maximum(ref, 0.0), np.maximum(seq, 0.0)
  got = np.asarray(got, np.float64).reshape(ref.shape)
  err = np.abs(got - ref)
  bound = (k + 3) * EPS * mag
  with np.errstate(divide='ignore', invalid='ignore'):
    over = np.where(err > 0, err / bound, 0.0)
  rms = float(np.sqrt(np.mean(err**2)))
  rms_seq = float(np.sqrt(np.mean((seq - ref)**2)))
  return dict(max_over_bound=float(over.max()), frac_over=float(np.mean(err > bound)), rms=rms,
              rms_seq=rms_seq, rms_ratio=rms / rms_seq if rms_seq > 0 else (0.0 if rms == 0 else np.inf),
              ok_bound=bool(np.all(err <= bound)), ok_rms=bool(rms <= RMS_MARGIN * rms_seq))


def report(rows):
  """Prints every (name, product_check result), then asserts both bars on
  all of them."""
  for name, r in rows:
    print('%-22s max err / bound %.4f   rms %.2e   rms / sequential-f32 rms %.3f%s' % (
        name, r['max_over_bound'], r['rms'], r['rms_ratio'],
        '' if r['ok_bound'] and r['ok_rms'] else '   <-- FAILS'))
  bad = [(n, 'bound' if not r['ok_bound'] else 'rms', r['max_over_bound'], r['rms_ratio'])
         for n, r in rows if not (r['ok_bound'] and r['ok_rms'])]
  assert not bad, bad
