"""The short-map attention kernels (csrc/attention.hip) on every kernel family and launch form: the case table, the launch
rule of `launch` / `launch_mh` restated, the operands of each input family, the placements as flat buffers (shared by the
numpy model's emulation of a wrong stride and by the GPU run) and the guarded launch sequence
(tests/test_gpu_attention_forms.py on the HIP library, tests/test_attention_cases_cpu.py without a GPU).  The reference,
the bounds and the numpy model are tests/_attn_ref.py.

Families (family(case), the vocabulary of REQUIRED).  The single-head instantiations are 'sh rolled 128' (T <= 128),
'sh rolled 256' and 'sh full' (C = T = 256); the MH ones 'mh rolled 128', 'mh rolled 256' and 'mh full' with the head widths
32 / 64 / 128 / 256 at T = 256.  The MH entry runs the MH instantiations when heads > 1 or a gradient is NULL, else the
single-head ones (stk_mh::short_fwd / short_bwd).  The four full widths share one family for the launch forms: a placement,
a beta or a scale reaches the kernel through Args.xs / ys / as / os, beta[] and scale, which no instantiation treats
differently; every width is reached on its own.  Further marks: 'split-n' (a full head of d <= 128: phase B by (channel
block, half tile)), 'dead waves' (d = 32 or 96 on the rolled TK = 256 kernel: waves whose first channel block lies beyond d),
'one head through mh' and 'C 512'.

Placements.  separate: q, k, v and dq, dk, dv are six tensors of image stride C T.  stacked: the channel slices of one
[B, 3 C, T] tensor each, stride 3 C T.  padded: six tensors of stride C T + 28 (q, k, v) and C T + 12 (gradients): the input
gaps hold +-2 max |tensor| (finite in fp16 at the kernel's scale, so a masked lane still multiplies by an exact zero; a
maximum that read the gap would be twice too large), the output gaps sentinels.  mixed-a: stacked q / k / v, separate
gradients; mixed-b the reverse.  do is always contiguous.  beta: 'zero' runs beta = 0 on NaN-filled gradients, 'triple'
(beta_q, beta_k, beta_v) = (0.5, 1.0, 0.25) on randn-filled ones.  null (MH entry only): the one gradient passed as NULL.

Input families (inputs()):
  randn       q, k scaled so that the scores have a standard deviation of 3 (at 1 the softmax of a small head is almost
              uniform and a head or row mix-up moves little); v, do randn.
  decades     randn, each (image, head) of each of q, k, v, do times its own factor of {1, 1e-1, 1e-2, 1e-3}.
  apart       randn times (3e3, 2e-3, 5e-4, 1e-6).
  negative    q = a u + noise, k = -a u + noise for one sign vector u: every score <= -20 (asserted).  On every T that is
              not a multiple of 32: a pad column let through the mask has score 0 and takes the whole softmax.
  offset      k = +a u + noise: row maxima around +60.
  coherent    q, k = (1 + 0.9 2^-11) 2^j, j in {-1, 0, 1}: every lo part is positive and as large as it gets, so a lost
              hi lo term is a coherent 4.4e-4 of every score instead of a random walk.
  tiny do     randn with do = 2^-100 randn: the ds tiles' scales reach 2^120, and their product with k's or q's scale passes
              2^127, which the epilogue's 1 / (sa sds) turned into a factor 0; it divides by one after the other now.
  floor cases (FLOOR_CASES; the floor may dominate the bound there, and the model has to show an error of a quarter of it):
    floor peaked      one key takes all but ~4e-11 of every row (the others' exp(s - max) ~ 0.4 2^-38, below half a step of
                      the 2^13 split; at 1e-9 of the mass they would round either way and cancel) and carries v = 0; v >= 0.
                      o then IS what the other keys contribute.
    floor unattended  a whole 64-key tile with p ~ 0.33 2^-38 for every query; do >= 0.  dv of those keys is pure floor; their
                      ds is 2^-37 of the other tile's, which only a scale taken over the tile keeps.
    floor ds row      one query's do, and so its row of ds, is 2^-20 of its neighbours' in the same 64-query tile.  At
                      2^-20 the split residual of that row is 2^-18 of its values, under the rounding part of the bound
                      (k u > 2^-17 at d = 32, T = 28), and it is a sum of residuals of either sign (the model reaches 0.06
                      of the worst case at T = 4 and at T = 28).  So the row is no floor case in the sense of the two
                      conditions: it is held to condition 1 like every other case, and what a ds scale from the wrong
                      extent does is shown by 'floor unattended' (the mutant of tests/test_attention_cases_cpu.py).
"""
import collections
import functools

import numpy as np

import _attn_ref as ar

STK_OK, STK_EINVAL, STK_EUNSUPPORTED = 0, -1, -3
TRIPLE = (0.5, 1.0, 0.25)
NPART = 256

Case = collections.namedtuple('Case', 'name entry B C heads T place beta scale null fam')


def _c(entry, B, C, heads, T, place, beta='zero', scale='d', null=None, fam='randn'):
  name = f'{entry}_B{B}C{C}h{heads}T{T}_{place}_{beta}_s{scale}' + ('' if null is None else f'_null{null}') + '_' + fam.replace(' ', '-')
  return Case(name, entry, B, C, heads, T, place, beta, scale, null, fam)


CASES = [
  # ---- single-head entries ------------------------------------------------------------------------------------------------
  _c('sh', 1, 32, 1, 4, 'separate'),                                            # grid 1
  _c('sh', 3, 64, 1, 28, 'stacked', 'triple', 0.37, fam='negative'),            # grid 3
  _c('sh', 2, 96, 1, 32, 'padded', fam='decades'),
  _c('sh', 7, 160, 1, 36, 'mixed-a', 'triple', fam='negative'),                 # grid 7
  _c('sh', 2, 224, 1, 64, 'mixed-b', fam='apart'),
  _c('sh', 2, 256, 1, 68, 'padded', 'triple', fam='negative'),
  _c('sh', 3, 64, 1, 100, 'separate', scale=0.37, fam='offset'),
  _c('sh', 2, 256, 1, 128, 'stacked'),
  _c('sh', 1, 32, 1, 132, 'padded', 'triple', fam='negative'),                  # grid 3, the first T on TK = 256
  _c('sh', 3, 96, 1, 196, 'stacked', scale=0.37, fam='negative'),
  _c('sh', 2, 160, 1, 252, 'mixed-a', fam='negative'),                          # grid 8
  _c('sh', 2, 224, 1, 256, 'separate', 'triple'),
  _c('sh', 3, 64, 1, 256, 'mixed-b', fam='decades'),
  _c('sh', 1, 256, 1, 256, 'separate'),                                         # the straight-line kernel
  _c('sh', 2, 256, 1, 256, 'stacked', 'triple', 0.37),
  _c('sh', 3, 256, 1, 256, 'padded', fam='decades'),
  _c('sh', 2, 256, 1, 256, 'mixed-a', 'triple', fam='offset'),
  _c('sh', 2, 256, 1, 256, 'mixed-b', fam='apart'),
  # ---- MH: the straight-line widths at T = 256 -----------------------------------------------------------------------------
  _c('mh', 1, 64, 2, 256, 'separate'),                                          # d = 32, grid 8
  _c('mh', 2, 128, 4, 256, 'padded', 'triple', 0.37, fam='decades'),            # d = 32, grid 32
  _c('mh', 1, 128, 2, 256, 'stacked', null=0, fam='decades'),                   # d = 64
  _c('mh', 2, 192, 3, 256, 'mixed-a', 'triple'),                                # d = 64, odd head count
  _c('mh', 1, 256, 2, 256, 'mixed-b', scale=0.37, null=1),                      # d = 128
  _c('mh', 2, 256, 2, 256, 'padded', null=2, fam='apart'),                      # d = 128
  _c('mh', 2, 512, 2, 256, 'stacked', 'triple', fam='decades'),                 # d = 256, C = 512: the largest tensor
  _c('mh', 1, 512, 2, 256, 'separate', fam='offset'),                           # d = 256
  # ---- MH: the rolled TK = 128 kernel ---------------------------------------------------------------------------------------
  _c('mh', 1, 64, 2, 4, 'separate', fam='negative'),
  _c('mh', 3, 96, 3, 28, 'stacked', 'triple', fam='negative'),                  # grid 9
  _c('mh', 9, 64, 2, 32, 'padded', scale=0.37, fam='decades'),                  # grid 18
  _c('mh', 2, 192, 2, 36, 'mixed-a', null=0, fam='negative'),                   # d = 96
  _c('mh', 1, 320, 2, 64, 'mixed-b', 'triple', null=1),                         # d = 160
  _c('mh', 1, 448, 2, 68, 'separate', null=2, fam='negative'),                  # d = 224
  _c('mh', 1, 512, 2, 100, 'stacked', fam='negative'),                          # d = 256
  _c('mh', 1, 128, 1, 128, 'padded', 'triple'),                                 # one head, every gradient: the single-head kernels
  _c('mh', 1, 128, 1, 64, 'separate', null=0),                                  # one head on the MH kernels
  # ---- MH: the rolled TK = 256 kernel ---------------------------------------------------------------------------------------
  _c('mh', 1, 64, 2, 132, 'separate', 'triple', fam='negative'),                # d = 32: waves 1 .. 7 have no phase-B tile
  _c('mh', 1, 192, 2, 256, 'stacked'),                                          # d = 96 at T = 256: rolled, waves 3 .. 7 idle
  _c('mh', 1, 192, 2, 196, 'padded', scale=0.37, null=1, fam='negative'),
  _c('mh', 2, 320, 2, 252, 'mixed-a', 'triple', null=2, fam='negative'),        # d = 160
  _c('mh', 1, 448, 2, 132, 'mixed-b', null=0, fam='offset'),                    # d = 224
  # ---- the floor cases and the coherent split -------------------------------------------------------------------------------
  _c('mh', 2, 64, 2, 28, 'separate', fam='floor peaked'),
  _c('mh', 1, 64, 2, 128, 'separate', fam='floor unattended'),
  _c('sh', 2, 32, 1, 28, 'separate', fam='floor ds row'),
  _c('mh', 2, 64, 2, 64, 'separate', fam='coherent'),
  _c('sh', 2, 64, 1, 128, 'separate', fam='tiny do'),                           # last: a case's seed is its position
]
IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
FLOOR_CASES = {'floor peaked': ('o',), 'floor unattended': ('dv',)}          # family -> outputs held to a quarter of the floor
DS_ROW = 5                                                                    # the small query of 'floor ds row'
PLACES = ('separate', 'stacked', 'padded', 'mixed-a', 'mixed-b')
T_VALUES = (4, 28, 32, 36, 64, 68, 100, 128, 132, 196, 252, 256)
D_VALUES = (32, 64, 96, 160, 224, 256)
GRIDS = (1, 3, 7, 8, 9)


# ---- the launch rule, restated ---------------------------------------------------------------------------------------------
def scale_of(c):
  """The float32 score scale the entries receive."""
  return float(np.float32((c.C // c.heads) ** -0.5 if c.scale == 'd' else c.scale))


def uses_mh_kernels(c):
  """stk_mh::short_fwd / short_bwd -> (forward, backward): the MH instantiations or the single-head ones."""
  if c.entry == 'sh':
    return False, False
  return c.heads > 1, c.heads > 1 or c.null is not None


def kernel(mh, d, T):
  """`launch` (mh False; d = C) / `launch_mh`: (family, TK, full)."""
  if T == 256 and (d in (32, 64, 128, 256) if mh else d == 256):
    return ('mh full' if mh else 'sh full'), 256, True
  if T <= 128:
    return ('mh rolled 128' if mh else 'sh rolled 128'), 128, False
  return ('mh rolled 256' if mh else 'sh rolled 256'), 256, False


def family(c):
  """The kernel family of the case's backward (its forward is the same unless one head runs with a NULL gradient)."""
  return kernel(uses_mh_kernels(c)[1], c.C // c.heads, c.T)[0]


def grid(c):
  return c.B * c.heads * ((c.T + 63) // 64)


def forms(c):
  """Everything case c reaches (strings, the vocabulary of REQUIRED)."""
  d = c.C // c.heads
  fam, TK, full = kernel(uses_mh_kernels(c)[1], d, c.T)
  f = {fam, f'{fam} {c.place}', f'{fam} beta {c.beta}', f'{fam} scale {c.scale}', f'T {c.T}', f'd {d}', f'grid {grid(c)}',
       f'{fam} fam {c.fam}', f'fam {c.fam}'}
  if grid(c) > 16:
    f.add('grid above 16')
  if c.null is not None:
    f.add(f'{fam} null {c.null}')
  if fam == 'mh full':
    f.add(f'mh full d {d}')
    if d <= 128:
      f.add('split-n')
  if fam == 'mh rolled 256' and d in (32, 96):
    f.add(f'dead waves d {d}')
  if c.entry == 'mh' and c.heads == 1:
    f.add('one head through mh, ' + ('MH kernels' if c.null is not None else 'single-head kernels'))
  if c.C == 512 and c.heads == 2:
    f.add('C 512')
  if c.fam == 'negative':
    f.add(f'negative T {c.T}')
  return f


FAMILIES = ('sh rolled 128', 'sh rolled 256', 'sh full', 'mh rolled 128', 'mh rolled 256', 'mh full')


def _required():
  R = set(FAMILIES)
  for fam in FAMILIES:
    R |= {f'{fam} {p}' for p in PLACES} | {f'{fam} beta zero', f'{fam} beta triple', f'{fam} scale d', f'{fam} scale 0.37'}
    if fam.startswith('mh'):
      R |= {f'{fam} null {i}' for i in range(3)}
  R |= {f'T {T}' for T in T_VALUES} | {f'd {d}' for d in D_VALUES} | {f'grid {g}' for g in GRIDS} | {'grid above 16'}
  R |= {f'mh full d {d}' for d in (32, 64, 128, 256)} | {'split-n', 'dead waves d 32', 'dead waves d 96', 'C 512'}
  R |= {'one head through mh, MH kernels', 'one head through mh, single-head kernels'}
  R |= {f'negative T {T}' for T in T_VALUES if T % 32}
  R |= {f'fam {f}' for f in ('randn', 'decades', 'apart', 'negative', 'offset', 'coherent', 'tiny do') + tuple(FLOOR_CASES)}
  return R


REQUIRED = _required()


# ---- operands ----------------------------------------------------------------------------------------------------------------
def _inputs(c, seed=None):
  """seed: for a case of another table (tests/_attn_long_cases.py); this table's cases take theirs from their position."""
  B, C, T, H = c.B, c.C, c.T, c.heads
  d = C // H
  scale = scale_of(c)
  rng = np.random.default_rng(4100 + IDS.index(c.name) if seed is None else seed)
  rn = lambda *s: rng.standard_normal(s)
  per_head = lambda u: np.tile(u, H)[None, :, None]                             # a [d] vector on every head: [1, C, 1]
  u0 = per_head(rng.choice([-1.0, 1.0], d))
  q, k, v, do = rn(B, C, T), rn(B, C, T), rn(B, C, T), rn(B, C, T)
  fam = c.fam
  if fam in ('randn', 'decades', 'apart', 'floor ds row', 'tiny do'):
    a = (3.0 / (scale * d ** 0.5)) ** 0.5
    q, k = q * a, k * a
    if fam == 'decades':
      F = np.array([1.0, 1e-1, 1e-2, 1e-3])
      fac = F[rng.integers(0, 4, (4, B, H))]
      fac[:, 0, 0] = 1.0                                                        # one head keeps its sharp scores
      q, k, v, do = (t * np.repeat(fac[i], d, 1)[:, :, None] for i, t in enumerate((q, k, v, do)))
    elif fam == 'apart':
      q, k, v, do = q / a * 3e3, k / a * 2e-3, v * 5e-4, do * 1e-6
    elif fam == 'floor ds row':
      do[:, :, DS_ROW] *= 2.0 ** -20
    elif fam == 'tiny do':
      do = do * 2.0 ** -100
  elif fam in ('negative', 'offset'):
    a = ((34.0 if fam == 'negative' else 55.0) / (scale * d)) ** 0.5
    sg = 2.0 / (scale * a * (2 * d) ** 0.5)
    q, k = a * u0 + sg * q, (-a if fam == 'negative' else a) * u0 + sg * k
  elif fam == 'coherent':
    m = 1.0 + 0.9 * 2.0 ** -11
    q, k = m * 2.0 ** rng.integers(-1, 2, (B, C, T)), m * 2.0 ** rng.integers(-1, 2, (B, C, T))
  elif fam == 'floor peaked':
    a = ((38 * np.log(2.0) - np.log(0.4)) / (scale * d)) ** 0.5                 # exp(-scale a^2 d) = 0.4 2^-38
    sg = 0.1 / (scale * a * d ** 0.5)
    j0 = 3
    q, k = a * u0 + sg * q, sg * k
    k[:, :, j0] += a * u0[0, :, 0]
    v = np.abs(v)
    v[:, :, j0] = 0.0
  elif fam == 'floor unattended':
    a = ((38 * np.log(2.0) - np.log(0.33) - np.log(64.0)) / (scale * d)) ** 0.5  # p = exp(-scale a^2 d) / 64 = 0.33 2^-38
    sg = 0.1 / (scale * a * d ** 0.5)
    q, k = a * u0 + sg * q, sg * k
    k[:, :, 64:] -= a * u0
    do = np.abs(do)
  else:
    raise ValueError(fam)
  t = {n: np.ascontiguousarray(x, dtype=np.float32) for n, x in (('q', q), ('k', k), ('v', v), ('do', do))}
  g0 = [rn(B, C, T).astype(np.float32) * np.float32(np.abs(t[n]).mean() * s) for n, s in (('q', 1.0), ('k', 1.0), ('v', 1.0))]
  t['g0'] = g0 if c.beta == 'triple' else [np.full((B, C, T), np.nan, np.float32)] * 3
  return t


@functools.lru_cache(maxsize=4)
def inputs(name):
  """The float32 operands of a case (cached, never modified): q, k, v, do of [B, C, T] and g0, the three initial gradients
  (NaN under beta = 0)."""
  return _inputs(BY_NAME[name])


def betas(c):
  return TRIPLE if c.beta == 'triple' else (0.0, 0.0, 0.0)


@functools.lru_cache(maxsize=2)
def reference(name):
  """(want, bnd, ref): the float64 outputs of a case as the launch leaves them (beta g0 added), the bounds of
  tests/_attn_ref.py and the bare reference with its 'aux' quantities, computed once and shared."""
  c, t = BY_NAME[name], inputs(name)
  ref = ar.reference(t['q'], t['k'], t['v'], t['do'], c.heads, scale_of(c))
  bnd = ar.bounds(ref, t['q'], t['k'], t['v'], t['do'], c.heads, scale_of(c), betas(c), t['g0'])
  want = {n: ref[n] for n in ar.OUTPUTS}
  for i, n in enumerate(('dq', 'dk', 'dv')):
    if betas(c)[i] != 0.0:
      want[n] = betas(c)[i] * t['g0'][i].astype(np.float64) + ref[n]
  return want, bnd, ref


def checked(c):
  """The outputs a case is held to: a NULL gradient is compared with its initial bits instead."""
  return tuple(n for i, n in enumerate(ar.OUTPUTS) if c.null is None or n != ('dq', 'dk', 'dv')[c.null])


# ---- placements: flat buffers ------------------------------------------------------------------------------------------------
GAP_SENTINEL = np.float32(-1.5 * 2.0 ** 79)


def strides(c):
  """(qkv_bstride, grad_bstride, q / k / v stacked, gradients stacked)."""
  ct = c.C * c.T
  return {'separate': (ct, ct, False, False), 'stacked': (3 * ct, 3 * ct, True, True), 'padded': (ct + 28, ct + 12, False, False),
          'mixed-a': (3 * ct, ct, True, False), 'mixed-b': (ct, 3 * ct, False, True)}[c.place]


def _flat(ts, B, ct, bs, stacked, gap):
  """The flat buffers of three [B, C, T] tensors and their offsets: [(buffer index, first element)] * 3.  gap(i): the
  filler of tensor i's gaps."""
  if stacked:
    return [np.ascontiguousarray(np.concatenate([t.reshape(B, ct) for t in ts], 1)).reshape(-1)], [(0, i * ct) for i in range(3)]
  bufs = []
  for i, t in enumerate(ts):
    f = np.full((B - 1) * bs + ct, gap(i), np.float32)
    for b in range(B):
      f[b * bs:b * bs + ct] = t[b].reshape(-1)
    bufs.append(f)
  return bufs, [(i, 0) for i in range(3)]


def layout(c):
  """The buffers a launch of case c sees: 'in' / 'grad': (flat float32 buffers, [(buffer, offset)] of q, k, v / dq, dk, dv),
  'written': per gradient buffer the mask of the elements the launch may write."""
  t = inputs(c.name)
  ct = c.C * c.T
  bs, gs, qst, gst = strides(c)
  sign = lambda i: np.float32((2.0 if i % 2 == 0 else -2.0) * np.abs(t['qkv'[i]]).max())
  ins = _flat([t['q'], t['k'], t['v']], c.B, ct, bs, qst, sign)
  grads = _flat(t['g0'], c.B, ct, gs, gst, lambda i: GAP_SENTINEL)
  written = [np.zeros(f.shape, bool) for f in grads[0]]
  for i, (bi, off) in enumerate(grads[1]):
    if c.null != i:
      for b in range(c.B):
        written[bi][off + b * gs:off + b * gs + ct] = True
  return {'in': ins, 'grad': grads, 'written': written, 'bs': bs, 'gs': gs}


def gather(flat, off, B, ct, stride, shape):
  """[B, C, T] read from a flat buffer at an image stride; elements past the buffer read as zero."""
  out = np.zeros((B, ct), flat.dtype)
  for b in range(B):
    seg = flat[off + b * stride:off + b * stride + ct]
    out[b, :seg.size] = seg
  return out.reshape(shape)


def run_model(c, mutant=None):
  """The numpy model on the buffers of case c, read and written at the strides the host code passes on.  mutant: one of
  _attn_ref.model's, 'scale of C', 'gradients at the qkv stride', 'do at the gradient stride'."""
  t, L = inputs(c.name), layout(c)
  B, C, T = c.B, c.C, c.T
  ct, shape = C * T, (B, C, T)
  q, k, v = (gather(L['in'][0][bi], off, B, ct, L['bs'], shape) for bi, off in L['in'][1])
  do = gather(t['do'].reshape(-1), 0, B, ct, L['gs'] if mutant == 'do at the gradient stride' else ct, shape)
  scale = float(np.float32(C ** -0.5)) if mutant == 'scale of C' else scale_of(c)
  inner = mutant if mutant not in ('scale of C', 'gradients at the qkv stride', 'do at the gradient stride') else None
  out = ar.model(q, k, v, do, c.heads, scale, betas(c), t['g0'], inner)
  ws = L['bs'] if mutant == 'gradients at the qkv stride' else L['gs']
  bufs = [f.copy() for f in L['grad'][0]]
  for i, n in enumerate(('dq', 'dk', 'dv')):
    bi, off = L['grad'][1][i]
    if c.null == i:
      continue
    for b in range(B):
      seg = bufs[bi][off + b * ws:off + b * ws + ct]
      seg[:] = out[n][b].reshape(-1)[:seg.size]
  for i, n in enumerate(('dq', 'dk', 'dv')):
    bi, off = L['grad'][1][i]
    out[n] = gather(bufs[bi], off, B, ct, L['gs'], shape)
  return out


# ---- the launch sequence -------------------------------------------------------------------------------------------------------
def run(lib, c, dev='cuda'):
  """One forward and one backward of case c through the C ABI on fresh guarded buffers -> the outputs and 'rec' as numpy
  arrays.  Asserted here: the guards, every element of the gradient buffers outside the images (gaps, a NULL gradient's
  slice), the operands' bits."""
  import torch
  from _stream_util import Guarded
  t, L = inputs(c.name), layout(c)
  B, C, T, H = c.B, c.C, c.T, c.heads
  nan = lambda *s: np.full(s, np.nan, np.float32)
  gin = [Guarded(f, dev) for f in L['in'][0]]
  ggr = [Guarded(f, dev) for f in L['grad'][0]]
  gdo = Guarded(t['do'], dev)
  G = {'o': Guarded(nan(B, C, T), dev), 'lse': Guarded(nan(B, H, T), dev), 'delta': Guarded(nan(B, H, T), dev),
       'rec': Guarded(nan(4 * NPART), dev)}
  ptr = lambda g, off: g.view.data_ptr() + 4 * off
  ins = [ptr(gin[bi], off) for bi, off in L['in'][1]]
  outs = [None if c.null == i else ptr(ggr[bi], off) for i, (bi, off) in enumerate(L['grad'][1])]
  bq, bk, bv = betas(c)
  scale = scale_of(c)
  stream = torch.cuda.current_stream().cuda_stream
  o, lse, delta, rec = (G[n].view.data_ptr() for n in ('o', 'lse', 'delta', 'rec'))
  if c.entry == 'sh':
    assert lib.attention_ok(B, C, T) == 1, c.name
    lib.attention_fwd_f32(ins[0], ins[1], ins[2], L['bs'], o, lse, rec, B, C, T, scale, stream)
    lib.attention_bwd_f32(ins[0], ins[1], ins[2], L['bs'], gdo.view.data_ptr(), lse, rec, delta, outs[0], bq, outs[1], bk,
                          outs[2], bv, L['gs'], B, C, T, scale, stream)
  else:
    assert lib.attention_mh_ok(B, C, T, H) == 1 and int(lib.attention_mh_ws_bytes(B, C, T, H)) == 0, c.name
    ws = torch.zeros(4, device=dev)
    lib.attention_mh_fwd_f32(ins[0], ins[1], ins[2], L['bs'], o, lse, rec, B, C, T, H, scale, ws.data_ptr(), 0, stream)
    lib.attention_mh_bwd_f32(ins[0], ins[1], ins[2], L['bs'], o, gdo.view.data_ptr(), lse, rec, delta, outs[0], bq, outs[1], bk,
                             outs[2], bv, L['gs'], B, C, T, H, scale, ws.data_ptr(), 0, stream)
  torch.cuda.synchronize()
  for n, g in list(G.items()) + [(f'in{i}', g) for i, g in enumerate(gin)] + [(f'grad{i}', g) for i, g in enumerate(ggr)] + [('do', gdo)]:
    g.check(f'{c.name} {n}')
  bits = lambda a: np.ascontiguousarray(a).view(np.int32)
  for i, g in enumerate(gin):
    assert np.array_equal(bits(g.view.cpu().numpy()), bits(L['in'][0][i])), f'{c.name}: operand buffer {i} was written'
  assert np.array_equal(bits(gdo.view.cpu().numpy()), bits(t['do'])), f'{c.name}: do was written'
  got = {n: G[n].view.cpu().numpy() for n in G}
  flat = [g.view.cpu().numpy() for g in ggr]
  for i, f in enumerate(flat):
    keep = ~L['written'][i]
    assert np.array_equal(bits(f)[keep], bits(L['grad'][0][i])[keep]), \
        f'{c.name}: gradient buffer {i} was written outside its images (a gap, or the slice of a NULL gradient)'
  for i, n in enumerate(('dq', 'dk', 'dv')):
    bi, off = L['grad'][1][i]
    got[n] = gather(flat[bi], off, B, C * T, L['gs'], (B, C, T))
  return got
