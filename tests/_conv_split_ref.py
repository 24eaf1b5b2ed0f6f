"""The split convolutions (csrc/conv_x2.h, conv_x2d.h, conv_pl.h and the split path of csrc/conv.hip) element by element:
operands on which the kernels' arithmetic is exact with the integer model they must then equal bit for bit (instrument
A), a float64 reference with a derived per-element bound (instrument B), and a numpy model of the arithmetic (not of the
kernels' code) that has to stay inside half of every bound, and that can be broken on purpose, before anything runs on
a GPU (tests/test_conv_split_cases_cpu.py).  Vocabulary and metric are those of tests/_attn_ref.py.

The GEMM view.  Both directions are one contraction out[n, m, y, x] = sum_{k, tap} W[m, k, tap] a[n, k, y + dy, x + dx]
over the taps that fall inside the map: the forward with a = x, W = w (M = Cout rows, Kc = Cin), the data gradient with
a = dy and W[ci, co, tap] = w[co, ci, 8 - tap] (M = Cin rows, Kc = Cout; wprep_kernel's `flip`).  gemm_weights() makes
W from a weight tensor in either layout; a Problem carries a, W and the epilogue of one call.

Instrument A.  A tensor of values h + l, h in {0, +-1, .. +-hmax}, l in {0, +-2^-12}, l = 0 where h = 0, and one
element exactly 2, has the scale s = 2^12 (split.h pow2_scale_of: 2 * 2^12 = 2^13), hi = 4096 h and lo = +-1 exactly.
Every product hi hi, hi lo, lo hi is then a multiple of 2^-12 in unscaled units, and while sum |terms| + |addends| stays
at or under 2^12 (exactness() <= 2^24 granules) every partial sum of every subset is a 24-bit integer of granules: fp32
accumulation is exact in ANY order, and so are the slab sums and an epilogue of dyadic addends, out_div in {1, 2},
alpha / beta in {1, 0.5, 0}.  three_term() is that result in float64; it differs from the full float64 product by
exactly sum lo lo, the term the kernels drop by design.

Instrument B.  |got - ref| <= (1 + 2^-4) (2^-24 Bu + F) + 2^-126 per element (SECOND_ORDER of _attn_ref.py; 2^-126: the
smallest normal number, for results `acc * unscale` leaves subnormal), with u = 2^-24 and
  Bu = (k_c(K_px) + k_ep) S_abs + k_add A,
  S_abs = |gain| sum |W| |a| over the taps inside the map at that pixel, gain = 1 / out_div (forward) or alpha,
  K_px  = Kc times the number of those taps (a tap outside the map adds exact zeros), k_c(n) = 3 n + 12 (_attn_ref.py),
  A     = the epilogue addends in absolute value: (|bias| + |temb| + |res|) / out_div, or |beta dx0|,
  F     = |gain| (f_a sum |W| + f_w sum |a|) over the same taps, f = 2^-25 / s, s = pow2_scale_of of the maximum of
          the extent that shares the scale.
Extents, read from the code: the activation operand's scale is that of the WHOLE tensor -- split_planes_kernel reduces
the whole 256-float record that stk_amax_partial_f32 filled over the whole tensor, and the f32-operand entries launch
amax_partial_kernel over each source and gemm_kernel's block_amax(xpart, nxpart = 512) reduces BOTH records, so two
sources share one scale; the weights' scale is that of the layer's whole weight tensor (wamax_kernel walks M Kc taps,
weight_scale takes the maximum of its WPART partials).
Counts, beside the lines they come from:
  acc *= unscale                          conv_x2.h / conv_x2d.h: a power of two, exact (0 roundings)
  v[u] += t (slab_fwd / slab_dgrad)       the first slab is added to 0 exactly: splits - 1 roundings on partial sums
  v += bv; v += tv; v += rv (EpFwd)       one rounding for each addend present, each on a partial sum <= S_abs + A
  p.inv_div = 1.f / out_div; v *= inv_div  two roundings where out_div != 1, none at 1 (use_div is off)
  old = beta * *q (EpDgrad)               one rounding on |beta dx0| where beta != 0
  old + p.alpha * acc                     two roundings (product, sum) without contraction, one with an fma: counted 2,
                                          on S_abs and on |beta dx0| alike (alpha = 1, beta = 0: still counted)
  => forward  k_ep = (splits - 1) + n_addends + 2 [out_div != 1],  k_add = n_addends + 2 [out_div != 1]
     dgrad    k_ep = (splits - 1) + 2,                             k_add = 2

The model (model()): numpy float32 / float16 with the same precisions -- pow2_scale_of of the stated extent, hi / lo,
the three products (lo hi, hi lo, hi hi: SA / SB of the kernels) accumulated in float32 one contracted index after
another in the kernels' k order (32-channel group, tap, channel), one accumulator per K split, `unscale` formed as
(1 / sw) / sx, the slabs added in order, the epilogue in float32 without fma.  No tiles, waves or LDS; it runs on a
subset of images and pixels (the scales still come from the whole tensors).  MUTANTS lists the ways it can be broken.

Departures from the issue text: three_term() makes two float64 convolutions instead of three (hi (hi + lo) + lo hi,
linear, the same sum); K_px counts the taps inside the map instead of all nine (tighter)."""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from _attn_ref import SECOND_ORDER, U, k_c, pow2_scale_of, ratio, within      # noqa: F401  (re-exported)

HALF_STEP = 2.0 ** -25             # half the fp16 subnormal step
TINY = 2.0 ** -126
GRANULE = 2.0 ** -12               # of the exact operands' products, in unscaled units
KC = 32                            # channels per k chunk (x2::KC)

MUTANTS = ('hi lo dropped', 'lo hi dropped', 'lo at half weight', 'lo at double weight', 'lo lo added', 'tap dropped',
           'taps flipped', 'taps transposed', 'right border not padded', 'slab dropped', 'slab summed twice',
           'short split truncated', 'second source with beta1', 'dead rows written', 'temb of the tile\'s first image',
           'bias before unscale', 'out_div on the accumulator only', 'scale of the first source', 'unscale in one division')

# One call in the GEMM view.  a: float32 [N, Kc, H, W]; W: float32 [M, Kc, taps]; taps 9 or 1; splits: chunk counts of the
# K splits (sum = taps Kc / 32).  Forward: bias [M], temb [N, M], res [N, M, H, W] or None, div.  Dgrad: alpha, C1 (rows of
# the first source), beta = (beta1, beta2), dx0 [N, M, H, W] (rows of a beta == 0 source may hold anything, NaN included).
# S1: channels of a's first source (two-source forward of the f32-operand entry), else Kc.
Problem = namedtuple('Problem', 'dgrad a W taps splits bias temb res div alpha C1 beta dx0 S1')


def problem(dgrad, a, W, taps, splits=None, bias=None, temb=None, res=None, div=1.0, alpha=1.0, C1=None, beta=(0.0, 0.0),
            dx0=None, S1=None):
  M, Kc = W.shape[:2]
  nch = taps * (Kc // KC)
  splits = tuple(splits) if splits else (nch,)
  assert sum(splits) == nch and Kc % KC == 0, (splits, nch)
  return Problem(bool(dgrad), a, W, taps, splits, bias, temb, res, float(np.float32(div)), float(np.float32(alpha)),
                 M if C1 is None else C1, tuple(float(np.float32(b)) for b in beta), dx0, Kc if S1 is None else S1)


def gemm_weights(w, layout, Cin, Cout, K, dgrad):
  """W[m, k, tap] of the GEMM view from a weight tensor: OIHW (layout 0) or NIN [Cin][Cout] (layout 1, 1x1)."""
  w = np.asarray(w)
  w4 = w.T.reshape(Cout, Cin, 1, 1) if layout == 1 else w.reshape(Cout, Cin, K, K)
  if dgrad:
    w4 = w4.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]
  return np.ascontiguousarray(w4.reshape(w4.shape[0], w4.shape[1], K * K))


# ---- the split rule ------------------------------------------------------------------------------------------------------
def split(a, s=None):
  """hi, lo (float32 arrays holding the fp16 values of the SCALED tensor) and s of a float32 array by the rule of
  csrc/split.h; s: the scale of a wider extent than a itself."""
  a = np.asarray(a, np.float32)
  if s is None:
    s = pow2_scale_of(np.abs(a).max() if a.size else 0.0)
  with np.errstate(over='ignore', invalid='ignore'):
    v = (a * np.float32(s)).astype(np.float32)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
  return hi.astype(np.float32), lo.astype(np.float32), float(s)


# ---- instrument A --------------------------------------------------------------------------------------------------------
def exact_tensor(shape, hmax, seed):
  """float32 values h + l, h in {0, +-1 .. +-hmax}, l in {0, +-2^-12} (0 where h = 0; towards zero where |h| = 2, so that
  the maximum is exactly 2), and one element exactly 2 at a seeded position away from index 0."""
  g = np.random.default_rng(seed)
  n = int(np.prod(shape))
  h = g.integers(-hmax, hmax + 1, n).astype(np.float64)
  l = g.integers(-1, 2, n).astype(np.float64) * GRANULE
  l = np.where(h == 0, 0.0, l)
  l = np.where(np.abs(h) == 2, -np.sign(h) * np.abs(l), l)
  t = h + l
  t[int(g.integers(max(1, n // 3), n))] = 2.0
  t = t.astype(np.float32).reshape(shape)
  assert np.abs(t).max() == 2.0
  return t


def _corr(a, W, taps):
  """float64 sum_{k, tap} W[m, k, tap] a[n, k, y + dy, x + dx] with zero padding: torch.conv2d (a correlation)."""
  k = 3 if taps == 9 else 1
  w4 = torch.from_numpy(np.ascontiguousarray(W, dtype=np.float64)).reshape(W.shape[0], W.shape[1], k, k)
  return F.conv2d(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)), w4, padding=k // 2).numpy()


def _decoded(p):
  """the unscaled hi and lo planes of both operands, float64, with the scales of the extents of the module text"""
  sa, sw = pow2_scale_of(np.abs(p.a).max()), pow2_scale_of(np.abs(p.W).max())
  ah, al, _ = split(p.a, sa)
  wh, wl, _ = split(p.W, sw)
  return ah.astype(np.float64) / sa, al.astype(np.float64) / sa, wh.astype(np.float64) / sw, wl.astype(np.float64) / sw


def _addend(p, idx):
  """the epilogue's addend and its absolute-value form, float64 [len(idx), M, H, W]: the result is gain acc + addend"""
  N, _, H, Wd = p.a.shape
  M = p.W.shape[0]
  add, mag = np.zeros((len(idx), M, H, Wd)), np.zeros((len(idx), M, H, Wd))
  if p.dgrad:
    for rows, b in ((slice(0, p.C1), p.beta[0]), (slice(p.C1, M), p.beta[1])):
      if b != 0.0 and p.dx0 is not None:
        add[:, rows] = b * p.dx0[idx][:, rows].astype(np.float64)
    return add, np.abs(add)
  for t in (None if p.bias is None else p.bias.astype(np.float64)[None, :, None, None],
            None if p.temb is None else p.temb[idx].astype(np.float64)[:, :, None, None],
            None if p.res is None else p.res[idx].astype(np.float64)):
    if t is not None:
      add, mag = add + t, mag + np.abs(t)
  return add / p.div, mag / p.div


def gain_of(p):
  return p.alpha if p.dgrad else 1.0 / p.div


def three_term_acc(p, idx=None):
  """(hi hi + hi lo + lo hi, lo lo) before gain and addend, float64: depends on the operands alone"""
  idx = list(range(p.a.shape[0])) if idx is None else idx
  ah, al, wh, wl = _decoded(p)
  return _corr(ah[idx], wh + wl, p.taps) + _corr(al[idx], wh, p.taps), _corr(al[idx], wl, p.taps)


def three_term(p, idx=None, acc=None):
  """{'out': gain (hi hi + hi lo + lo hi) + addend, 'lolo': gain sum lo lo}, float64, images idx (all by default);
  acc: three_term_acc() of the same operands."""
  idx = list(range(p.a.shape[0])) if idx is None else idx
  acc, lolo = three_term_acc(p, idx) if acc is None else acc
  return {'out': gain_of(p) * acc + _addend(p, idx)[0], 'lolo': gain_of(p) * lolo}


def exactness(p, idx=None):
  """(sum |terms| + |addends|) / granule per element, before the gain: <= 2^24 means every partial sum of every subset,
  epilogue included, is a 24-bit integer of granules."""
  idx = list(range(p.a.shape[0])) if idx is None else idx
  ah, al, wh, wl = (np.abs(t) for t in _decoded(p))
  s = _corr(ah[idx], wh + wl, p.taps) + _corr(al[idx], wh, p.taps)
  return (s + _addend(p, idx)[1] / abs(gain_of(p))) / GRANULE


def is_exact_split(t, hmax):
  """the premise of instrument A on one tensor: scale 2^12, hi = 4096 h, lo in {0, +-1}"""
  hi, lo, s = split(t)
  return s == 4096.0 and bool(np.all(hi % 4096.0 == 0)) and bool(np.all(np.abs(hi) <= 4096.0 * max(hmax, 2))) and \
      bool(np.all(np.abs(lo) <= 1.0)) and bool(np.all((hi + lo) / 4096.0 == t))


# ---- instrument B --------------------------------------------------------------------------------------------------------
def parts(p, idx=None):
  """the float64 contractions reference() and bound() are made of (they depend on the operands alone, not on the epilogue
  or the entry): acc = sum W a, S = sum |W| |a|, sum_w, sum_a and K_px, over the taps inside the map."""
  idx = list(range(p.a.shape[0])) if idx is None else idx
  N, Kc, H, Wd = p.a.shape
  aa, aw = np.abs(p.a[idx].astype(np.float64)), np.abs(p.W.astype(np.float64))
  ones = np.ones((1, Kc, H, Wd))
  return {'acc': _corr(p.a[idx], p.W, p.taps), 'S': _corr(aa, aw, p.taps),
          'sum_w': _corr(ones, aw, p.taps),                                    # [1, M, H, W]
          'sum_a': _corr(aa, np.ones((1, Kc, p.taps)), p.taps),                # [n, 1, H, W]
          'kpx': _corr(ones, np.ones((1, Kc, p.taps)), p.taps)}                # [1, 1, H, W]: Kc x taps inside


def reference(p, idx=None, pt=None):
  """float64 result of the call on the fp32 operands, images idx: [len(idx), M, H, W]."""
  idx = list(range(p.a.shape[0])) if idx is None else idx
  pt = parts(p, idx) if pt is None else pt
  return gain_of(p) * pt['acc'] + _addend(p, idx)[0]


def bound(p, idx=None, pt=None):
  """{'Bu', 'F', 'bound'} of the module text, float64 [len(idx), M, H, W]."""
  idx = list(range(p.a.shape[0])) if idx is None else idx
  pt = parts(p, idx) if pt is None else pt
  g = abs(gain_of(p))
  A = _addend(p, idx)[1]
  ns = len(p.splits)
  if p.dgrad:
    k_ep, k_add = (ns - 1) + 2, 2
  else:
    n_add = sum(t is not None for t in (p.bias, p.temb, p.res))
    k_ep = (ns - 1) + n_add + (2 if p.div != 1.0 else 0)
    k_add = n_add + (2 if p.div != 1.0 else 0)
  Bu = (k_c(pt['kpx']) + k_ep) * g * pt['S'] + k_add * A
  fa = HALF_STEP / pow2_scale_of(np.abs(p.a).max())
  fw = HALF_STEP / pow2_scale_of(np.abs(p.W).max())
  Fl = g * (fa * pt['sum_w'] + fw * pt['sum_a'])
  return {'Bu': Bu, 'F': Fl, 'bound': SECOND_ORDER * (U * Bu + Fl) + TINY}


# ---- the numpy model -----------------------------------------------------------------------------------------------------
def pixels_of(H, Wd, limit=192, seed=0):
  """the pixels the model covers: all of a small map, else the corners, the border midpoints and a seeded sample"""
  hw = H * Wd
  if hw <= limit:
    return np.arange(hw)
  fixed = {0, Wd - 1, hw - Wd, hw - 1, Wd // 2, (H // 2) * Wd, (H // 2) * Wd + Wd - 1, hw - Wd // 2, Wd, 2 * Wd - 1}
  g = np.random.default_rng(seed)
  rest = g.choice(hw, limit - len(fixed), replace=False)
  return np.array(sorted(fixed | set(int(i) for i in rest)))


def k_order(Kc, taps):
  """the kernels' order of the contracted index: (32-channel group, tap, channel in group) -> (k, tap) pairs, and the
  chunk (32 of them) each belongs to"""
  ks, ts = [], []
  for cc in range(Kc // KC):
    for t in range(taps):
      ks += list(range(cc * KC, cc * KC + KC))
      ts += [t] * KC
  return np.array(ks), np.array(ts)


def _gather(a, taps, pix, wrap_right=False):
  """cols[n, k, tap, j] = a[n, k, y + dy, x + dx] of pixel pix[j], 0 outside the map (wrap_right: a read past the right
  border returns the next element in memory, the first of the next row)"""
  n, Kc, H, Wd = a.shape
  flat = a.reshape(n, Kc, H * Wd)
  y, x = pix // Wd, pix % Wd
  cols = np.zeros((n, Kc, taps, len(pix)), np.float32)
  for t in range(taps):
    dy, dx = (t // 3 - 1, t % 3 - 1) if taps == 9 else (0, 0)
    iy, ix = y + dy, x + dx
    ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < Wd)
    src = iy * Wd + ix
    if wrap_right:
      ok = ok | ((iy >= 0) & (iy < H) & (ix == Wd) & (src < H * Wd))
    cols[:, :, t, ok] = flat[:, :, src[ok]]
  return cols


def model(p, idx=None, pix=None, mutant=None, order=None):
  """The arithmetic of the split kernels (module text) on images idx and pixels pix -> float32 [len(idx), M, len(pix)].
  order: a seed; the contracted indices of every split are then accumulated in a shuffled order."""
  assert mutant is None or mutant in MUTANTS, mutant
  with np.errstate(over='ignore', invalid='ignore', under='ignore'):
    return _model(p, idx, pix, mutant, order)


def _model(p, idx, pix, mutant, order):
  f32 = np.float32
  N, Kc, H, Wd = p.a.shape
  M = p.W.shape[0]
  idx = list(range(N)) if idx is None else list(idx)
  pix = np.arange(H * Wd) if pix is None else np.asarray(pix)
  P = len(pix)
  extent = p.a[:, :p.S1] if mutant == 'scale of the first source' else p.a
  sa, sw = pow2_scale_of(np.abs(extent).max()), pow2_scale_of(np.abs(p.W).max())
  W = p.W
  if mutant == 'tap dropped':
    W = W.copy()
    W[:, :, p.taps - 1] = 0
  elif mutant == 'taps flipped':
    W = W[:, :, ::-1]
  elif mutant == 'taps transposed' and p.taps == 9:
    W = W.reshape(M, Kc, 3, 3).transpose(0, 1, 3, 2).reshape(M, Kc, 9)
  ah, al, _ = split(p.a[idx], sa)
  wh, wl, _ = split(W, sw)
  if mutant == 'lo at half weight':
    al = al * f32(0.5)
  elif mutant == 'lo at double weight':
    al = al * f32(2.0)
  wrap = mutant == 'right border not padded'
  ch, cl = _gather(ah, p.taps, pix, wrap), _gather(al, p.taps, pix, wrap)        # [n, Kc, taps, P]
  ks, ts = k_order(Kc, p.taps)
  splits = list(p.splits)
  if mutant == 'short split truncated' and splits[-1] % 2:
    splits[-1] -= 1
  if mutant == 'unscale in one division':
    unscale = f32(1.0) / (f32(sw) * f32(sa))                 # the product is inf past 2^127: unscale 0
  else:
    unscale = (f32(1.0) / f32(sw)) / f32(sa)
  n = len(idx)
  slabs = []
  c0 = 0
  for z, nc in enumerate(splits):
    sel = np.arange(c0 * KC, (c0 + nc) * KC)
    c0 += p.splits[z]
    if order is not None:
      sel = np.random.default_rng(order + z).permutation(sel)
    acc = np.zeros((n, M, P), f32)
    for j in sel:
      k, t = ks[j], ts[j]
      a_h, a_l = ch[:, None, k, t, :], cl[:, None, k, t, :]
      w_h, w_l = wh[None, :, k, t, None], wl[None, :, k, t, None]
      if mutant != 'lo hi dropped':
        acc += w_l * a_h
      if mutant != 'hi lo dropped':
        acc += w_h * a_l
      acc += w_h * a_h
      if mutant == 'lo lo added':
        acc += w_l * a_l
    slabs.append(acc)
  # epilogue
  bias = None if p.bias is None else p.bias.astype(f32)[None, :, None]
  if mutant == 'bias before unscale' and bias is not None:
    slabs[0] = slabs[0] + bias
    bias = None
  slabs = [s * unscale for s in slabs]
  if mutant == 'slab dropped' and len(slabs) > 1:
    slabs = slabs[:-1]
  elif mutant == 'slab summed twice' and len(slabs) > 1:
    slabs = slabs + slabs[-1:]
  v = slabs[0]
  for s in slabs[1:]:
    v = v + s
  if p.dgrad:
    out = np.empty((n, M, P), f32)
    for rows, b in ((slice(0, p.C1), p.beta[0]), (slice(p.C1, M), p.beta[1] if mutant != 'second source with beta1' else p.beta[0])):
      old = f32(0.0)
      if b != 0.0:
        old = f32(b) * p.dx0[idx][:, rows].reshape(n, -1, H * Wd)[:, :, pix].astype(f32)
      out[:, rows] = old + f32(p.alpha) * v[:, rows]
    return out
  inv_div = f32(1.0) / f32(p.div)
  if mutant == 'out_div on the accumulator only' and p.div != 1.0:
    v = v * inv_div
  if bias is not None:
    v = v + bias
  if p.temb is not None:
    img = np.asarray(idx)[:, None] * np.ones(P, int)[None, :]                    # image of every element
    if mutant == 'temb of the tile\'s first image':
      img = ((img * (H * Wd) + pix[None, :]) // 128 * 128) // (H * Wd)
    v = v + p.temb.astype(f32)[img].transpose(0, 2, 1)
  if p.res is not None:
    v = v + p.res[idx].reshape(n, M, H * Wd)[:, :, pix].astype(f32)
  if p.div != 1.0 and mutant != 'out_div on the accumulator only':
    v = v * inv_div
  if mutant == 'dead rows written':                # rows M .. pad128(M) - 1 of image b land on rows 0 .. of image b + 1
    dead = (M + 127) // 128 * 128 - M
    for i, b in enumerate(idx):
      if dead and b + 1 in idx:
        v[idx.index(b + 1), :dead] = f32(0.0)          # a zero accumulator through an epilogue without addends
  return v.astype(f32)


def at(t, pix):
  """[n, M, H, W] -> [n, M, len(pix)]"""
  return t.reshape(t.shape[0], t.shape[1], -1)[:, :, pix]
