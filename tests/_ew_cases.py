"""The case tables of the element-wise family (csrc/elementwise.hip) and one runner per entry.

A runner calls a library through the C ABI on whatever device that library lives on (the product on the GPU, the plain-C
checker on the host): tests/test_gpu_elementwise.py and tests/test_ew_cases_cpu.py walk the same tables.  Every operand sits
in a Guarded buffer (tests/_stream_util.py): 8 sentinels before and after it, checked after the call; every pure output is
NaN-prefilled, and so is an accumulated one at beta = 0.  The references and bounds are tests/_ew_ref.py's.

Launch forms.  The entries launched through launch_ew take the 16-byte form when the length (the row length `inner` for the
row-indexed ones) is a multiple of 4 and every streamed pointer is 16-byte aligned, the scalar form otherwise; `form` and
`strided` of a case say what it reaches (stk_ew_grid caps the grid at CAP = 2048 * 256 items and strides the rest).  Only those
entries are handed entered-one-in operands; the naive resamplers move float2s and get entered-two-in ones; the plain scalar
kernels run aligned.
"""
import collections
import functools
import itertools
import math

import numpy as np
import torch

import _ew_ref as R
from _stream_util import Guarded, U, within
from _util import call, dev_of

CAP = 2048 * 256
FLAT_N = (1, 3, 4, 5, 255, 256, 257, 1028, 4099, CAP + 5, 4 * CAP + 4)
ROWS = ((1, 1), (3, 4), (5, 7), (3, 260), (6, 768), (3, 174763), (3, 699052))
STD = (0.01, 0.3, 1.0, 50.0, 348.0)
BETAS = (0.0, 0.5, 1.0)
EDGE = [s * v for v in (0.0, 1e-40, 1e-30, 1.278, 20.0, 87.0, 89.0, 104.0, 1e4, 3e38) for s in (1.0, -1.0)]
FLAGS = tuple(itertools.product((0, 1), (0, 1), (0, 1)))                   # (vp, mode, reduce_mean)

Case = collections.namedtuple('Case', 'entry group p where form strided')
Entry = collections.namedtuple('Entry', 'base kind accum null')
ENTRIES, CASES = collections.OrderedDict(), []
STRIDED_PLAIN = ('concat', 'concat_bwd', 'fixed_fourier_fwd', 'fixed_fourier_bwd', 'resample_naive', 'fill_strided',
                 'samples_to_uint8')


def params(c):
  return dict(c.p)


def case_name(c):
  return f'{c.entry} {c.group} ' + ' '.join(f'{k}={v}' for k, v in c.p if k not in ('n', 'N', 'inner', 'argmax')) + f' {c.where}'


def _add(entry, group, p, where='aligned', form='plain', items=0):
  CASES.append(Case(entry, str(group), tuple(sorted(p.items())), where, form, items > CAP))


def _forms(entry, group, p, length, total, several):
  """The placements of one launch_ew case: aligned; entered-one-in where the length is a multiple of 4 (the scalar form by
  misalignment); and, once per entry with several pointers (total = 1028), the output alone and one input alone."""
  vec = length % 4 == 0
  _add(entry, group, p, 'aligned', 'vec' if vec else 'scalar', total // 4 if vec else total)
  if vec:
    _add(entry, group, p, 'entered-one-in', 'scalar', total)
    if several and total in (1028, 3 * 260):
      _add(entry, group, p, 'out-one-in', 'scalar', total)
      _add(entry, group, p, 'in-one-in', 'scalar', total)


def _table():
  E = ENTRIES
  # ---- flat, through launch_ew
  E['silu_fwd'] = Entry('silu_fwd', 'flat', False, False)
  E['silu_bwd'] = Entry('silu_bwd', 'flat', True, False)
  for act in range(5):
    E[f'act_fwd[{act}]'] = Entry('act_fwd', 'flat', False, False)
    E[f'act_bwd[{act}]'] = Entry('act_bwd', 'flat', True, False)
  for n in FLAT_N:
    _forms('silu_fwd', n, dict(n=n), n, n, True)
    for beta in BETAS:
      _forms('silu_bwd', n, dict(n=n, beta=beta), n, n, True)
    for act in range(5):
      _forms(f'act_fwd[{act}]', n, dict(n=n, act=act), n, n, True)
      for beta in BETAS:
        _forms(f'act_bwd[{act}]', n, dict(n=n, act=act, beta=beta), n, n, True)
  E['axpby'] = Entry('axpby', 'flat', True, True)
  E['add_div'] = Entry('add_div', 'flat', False, False)
  E['affine'] = Entry('affine', 'flat', False, False)
  E['fill'] = Entry('fill', 'flat', False, False)
  E['dropout_mask'] = Entry('dropout_mask', 'flat', False, False)
  for n in FLAT_N:
    _forms('axpby', n, dict(n=n, alpha=1.5, beta=0.5, variant='separate'), n, n, True)
    _forms('axpby', n, dict(n=n, alpha=R.f32(0.7), beta=1.0, variant='alias'), n, n, True)       # out is b
    _forms('axpby', n, dict(n=n, alpha=R.f32(0.7), beta=0.0, variant='alias'), n, n, True)       # out is b, NaN there
    _forms('axpby', n, dict(n=n, alpha=R.f32(0.7), beta=0.0, variant='null'), n, n, True)        # b = NULL
    _forms('add_div', n, dict(n=n, div=R.f32(math.sqrt(2.0))), n, n, True)
    _forms('add_div', n, dict(n=n, div=1.0), n, n, True)
    _forms('affine', n, dict(n=n, a=2.0, b=-1.0), n, n, True)
    _forms('fill', n, dict(n=n, v=1.25), n, n, False)
    for drop in (0.0, R.f32(0.1), 0.5):
      _forms('dropout_mask', n, dict(n=n, p=drop, seed=12345), n, n, False)
  E['fused_bias_act_f32'] = Entry('fused_bias_act', 'flat', False, True)
  for n in FLAT_N + (60,):                         # 60 = (4, 3, 5): a multiple of 4 whose step_b = 5 is not
    combos = itertools.product((1, 3), (0, 1, 2), (True, False), (True, False))
    if n > CAP:
      combos = [(3, 0, True, False), (3, 1, True, True)]
    for act, grad, bias, ref in combos:
      _forms('fused_bias_act_f32', n, dict(n=n, act=act, grad=grad, bias=bias, ref=ref, step_b=5, size_b=3, alpha=R.f32(0.2),
                                           scale=R.f32(math.sqrt(2.0)), dtype='f32'), n, n, True)
  for dt in ('f16', 'f64'):                        # plain grid-stride kernels: one small, one ragged shape
    E[f'fused_bias_act_{dt}'] = Entry('fused_bias_act', 'plain', False, True)
    for n, step_b, size_b in ((60, 5, 3), (4 * 6 * 77 + 1, 77, 6)):
      for act, grad, bias, ref in ((3, 0, True, False), (3, 1, True, True), (1, 0, False, False), (3, 2, True, True)):
        _add(f'fused_bias_act_{dt}', n, dict(n=n, act=act, grad=grad, bias=bias, ref=ref, step_b=step_b, size_b=size_b,
                                            alpha=R.f32(0.2), scale=R.f32(math.sqrt(2.0)), dtype=dt))
  # ---- row-indexed, through launch_ew
  E['rowscale'] = Entry('rowscale', 'row', False, False)
  E['perturb'] = Entry('perturb', 'row', False, True)
  for vp, mode, rm in FLAGS:
    E[f'sm_loss_bwd[{vp}{mode}{rm}]'] = Entry('sm_loss_bwd', 'row', False, False)
  for N, inner in ROWS:
    g = f'{N}x{inner}'
    for mode in (0, 1):
      _forms('rowscale', g, dict(N=N, inner=inner, mode=mode), inner, N * inner, True)
    for null in (False, True):
      _forms('perturb', g, dict(N=N, inner=inner, null=null), inner, N * inner, True)
    for vp, mode, rm in FLAGS:
      _forms(f'sm_loss_bwd[{vp}{mode}{rm}]', g, dict(N=N, inner=inner, vp=vp, mode=mode, rm=rm), inner, N * inner, True)
  # ---- plain scalar kernels
  E['sm_loss_fwd'] = Entry('sm_loss_fwd', 'plain', False, False)
  for inner in (1, 5, 255, 256, 257, 768, 12288):
    for N in (1, 6):
      for vp, mode, rm in FLAGS:
        _add('sm_loss_fwd', inner, dict(N=N, inner=inner, vp=vp, mode=mode, rm=rm))
  E['timestep_embedding'] = Entry('timestep_embedding', 'plain', False, False)
  for dim in (2, 3, 128, 129, 512):
    for B in (1, 6):
      _add('timestep_embedding', dim, dict(B=B, dim=dim, argmax=999.0))
  E['fourier_embedding'] = Entry('fourier_embedding', 'plain', False, False)
  E['fourier_embedding_bwd'] = Entry('fourier_embedding_bwd', 'plain', True, False)
  for nf in (1, 32, 128, 256, 257, 300):
    for B in (1, 6):
      _add('fourier_embedding', nf, dict(B=B, nf=nf, argmax=2400.0))
      for beta in BETAS:
        _add('fourier_embedding_bwd', nf, dict(B=B, nf=nf, beta=beta))
  E['fixed_fourier_fwd'] = Entry('fixed_fourier_fwd', 'plain', False, False)
  E['fixed_fourier_bwd'] = Entry('fixed_fourier_bwd', 'plain', True, False)
  for N, C, HW in ((1, 1, 1), (2, 3, 16), (1, 5, 77), (1, 3, 174763)):
    g = f'{N}x{C}x{HW}'
    _add('fixed_fourier_fwd', g, dict(N=N, C=C, HW=HW, argmax=805.0), items=N * C * HW)
    for beta in BETAS:
      _add('fixed_fourier_bwd', g, dict(N=N, C=C, HW=HW, beta=beta, argmax=805.0), items=N * C * HW)
  E['concat'] = Entry('concat', 'plain', False, False)
  E['concat_bwd'] = Entry('concat_bwd', 'plain', True, True)
  for N, Ca, Cb, HW in ((1, 1, 1, 1), (2, 3, 5, 16), (1, 7, 2, 9), (2, 3, 5, 32769)):
    g, total = f'{N}x{Ca}x{Cb}x{HW}', N * (Ca + Cb) * HW
    _add('concat', g, dict(N=N, Ca=Ca, Cb=Cb, HW=HW), items=total)
    for beta in (0.0, 0.5):
      for null in ('', 'da', 'db'):
        _add('concat_bwd', g, dict(N=N, Ca=Ca, Cb=Cb, HW=HW, beta=beta, null=null), items=total)
  E['resample_naive'] = Entry('resample_naive', 'pair', True, False)
  shapes = [(0, s) for s in ((1, 1, 1), (2, 3, 5), (6, 16, 16), (9, 244, 244))] + \
           [(1, s) for s in ((1, 2, 2), (2, 6, 10), (6, 16, 16), (9, 488, 488))]
  for mode, (P, H, W) in shapes:
    for alpha, beta in ((1.0, 0.0), (0.25, 1.0)):
      for where in ('aligned', 'entered-two-in'):
        _add('resample_naive', f'{"up" if mode == 0 else "down"}{P}x{H}x{W}',
             dict(planes=P, H=H, W=W, mode=mode, alpha=alpha, beta=beta), where, 'pair', P * H * W if mode == 0 else P * H * W // 4)
  E['fill_strided'] = Entry('fill_strided', 'plain', False, False)
  for count, ln, stride in ((1, 1, 1), (3, 4, 4), (5, 3, 7), (4, 512, 4096), (3, 3584, 4096), (129, 4096, 4100)):
    _add('fill_strided', f'{count}x{ln}x{stride}', dict(count=count, len=ln, stride=stride, v=1.25), items=count * ln)
  E['samples_to_uint8'] = Entry('samples_to_uint8', 'plain', False, False)
  for N, C, HW in [(2, C, HW) for C in (1, 3) for HW in (1, 25, 4096)] + [(1, 1, CAP + 3)]:
    _add('samples_to_uint8', f'{N}x{C}x{HW}', dict(N=N, C=C, HW=HW), items=N * HW)
  E['preprocess_u8'] = Entry('preprocess_u8', 'plain', False, False)
  for C, flip, centered, dequant in itertools.product((1, 3), (0, 1), (0, 1), (0, 1)):
    _add('preprocess_u8', f'C{C}', dict(N=4, C=C, H=5, W=7, flip=flip, centered=centered, dequant=dequant, seed=1234))


_table()
GROUPS = list(collections.OrderedDict(((c.entry, c.group), None) for c in CASES))
GROUP_IDS = [f'{e}-{g}' for e, g in GROUPS]


def group_cases(entry, group):
  return [c for c in CASES if c.entry == entry and c.group == group]


# ---- operands ---------------------------------------------------------------------------------------------------------
def _rn(seed, *shape, scale=1.0):
  return (np.random.RandomState(seed).standard_normal(shape) * scale).astype(np.float32)


def _nan(*shape, dtype=np.float32):
  return np.full(shape, np.nan, dtype=dtype)


def _act_x(n):
  """A random body with the edge values appended (as many of them as fit; only edge values where n < 21)."""
  x = _rn(n, n, scale=2.0)
  m = min(n, len(EDGE))
  x[n - m:] = np.array((EDGE + EDGE)[n % len(EDGE):][:m], dtype=np.float32) if n <= len(EDGE) else np.array(EDGE, dtype=np.float32)
  return x


def _std(N):
  return np.array([STD[i % len(STD)] for i in range(N)], dtype=np.float32)


def _inputs(base, p):
  n = p.get('n', 0)
  if base in ('silu_fwd', 'act_fwd'):
    return dict(x=_act_x(n))
  if base in ('silu_bwd', 'act_bwd'):
    return dict(x=_act_x(n), dy=_rn(n + 1, n), dx0=_rn(n + 2, n))
  if base in ('axpby', 'add_div'):
    return dict(a=_rn(n, n), b=None if p.get('variant') == 'null' else _rn(n + 1, n))
  if base == 'affine':
    return dict(x=_rn(n, n))
  if base == 'fused_bias_act':
    dt = {'f32': np.float32, 'f16': np.float16, 'f64': np.float64}[p['dtype']]
    return dict(x=_rn(n, n).astype(dt), b=_rn(7, p['size_b']).astype(dt) if p['bias'] else None,
                ref=_rn(n + 1, n).astype(dt) if p['ref'] else None)
  if base in ('rowscale', 'perturb', 'sm_loss_bwd', 'sm_loss_fwd'):
    N, inner = p['N'], p['inner']
    rs = np.random.RandomState(N)
    return dict(x=_rn(inner, N * inner), net=_rn(inner, N * inner), z=_rn(inner + 1, N * inner), s=_std(N), std=_std(N),
                a=None if p.get('null') else (rs.rand(N) * 0.9 + 0.1).astype(np.float32),
                wgt=(10.0 ** rs.uniform(-2, 3, N)).astype(np.float32), dloss=(10.0 ** rs.uniform(-3, 1, N) * (-1) ** np.arange(N)).astype(np.float32))
  if base == 'timestep_embedding':
    B, half = p['B'], p['dim'] // 2
    t = np.array([999.0] if B == 1 else [0.0, 999.0] + list(np.random.RandomState(B).rand(B - 2) * 999.0), dtype=np.float32)
    return dict(t=t, freqs=np.exp(np.arange(half, dtype=np.float32) * np.float32(-(math.log(10000.0) / max(half - 1, 1)))))
  if base in ('fourier_embedding', 'fourier_embedding_bwd'):
    B, nf = p['B'], p['nf']
    x = np.array([5.9] if B == 1 else [-4.6, 5.9] + list(np.random.RandomState(B).uniform(-4.6, 5.9, B - 2)), dtype=np.float32)
    a = dict(x=x, W=_rn(nf, nf, scale=16.0))
    if base == 'fourier_embedding_bwd':          # y is the float32 forward output
      a.update(y=R.fourier_embedding_f32(p, a), dy=_rn(nf + 1, B, 2 * nf), dx0=_rn(nf + 2, B))
    return a
  if base in ('fixed_fourier_fwd', 'fixed_fourier_bwd'):
    n = p['N'] * p['C'] * p['HW']
    x = np.random.RandomState(n).uniform(-1, 1, n).astype(np.float32)
    x[:3] = np.array([-1.0, 1.0, 0.0], dtype=np.float32)[:min(n, 3)]
    return dict(x=x, dy=_rn(n + 1, 5 * n), dx0=_rn(n + 2, n))
  if base in ('concat', 'concat_bwd'):
    N, Ca, Cb, HW = p['N'], p['Ca'], p['Cb'], p['HW']
    return dict(a=_rn(1, N * Ca * HW), b=_rn(2, N * Cb * HW), dout=_rn(3, N * (Ca + Cb) * HW), da0=_rn(4, N * Ca * HW), db0=_rn(5, N * Cb * HW))
  if base == 'resample_naive':
    n = p['planes'] * p['H'] * p['W']
    return {'in': _rn(n, n), 'out0': _rn(n + 1, 4 * n if p['mode'] == 0 else n // 4)}
  if base == 'fill_strided':
    return dict(out0=np.full((p['count'] - 1) * p['stride'] + p['len'], 7.0, dtype=np.float32))
  if base == 'samples_to_uint8':
    n = p['N'] * p['C'] * p['HW']
    ks = np.array([1, 2, 3, 127, 128, 200, 254, 255], dtype=np.float32) / np.float32(255)
    special = np.concatenate([np.array([-0.0, 0.0, -0.3, -1e-8, 1.0, np.nextafter(np.float32(1), np.float32(2)), 1.5, 300.0], dtype=np.float32),
                              ks, np.nextafter(ks, np.float32(0)), np.nextafter(ks, np.float32(2))])
    x = _rn(n, n, scale=0.4) + np.float32(0.5)
    x[:min(n, special.size)] = np.roll(special, -(n % special.size))[:min(n, special.size)]
    return dict(x=x)
  if base == 'preprocess_u8':
    return dict(img=np.random.RandomState(p['C']).randint(0, 256, p['N'] * p['H'] * p['W'] * p['C']).astype(np.uint8))
  return {}


@functools.lru_cache(maxsize=12)
def inputs(entry, p):
  return _inputs(ENTRIES[entry].base, dict(p))


@functools.lru_cache(maxsize=6)
def reference(entry, p):
  """The float64 reference of a case, computed once and shared by its placements (and by the two test modules)."""
  e, pd = ENTRIES[entry], dict(p)
  name = e.base + ('_' + pd['dtype'] if pd.get('dtype') in ('f16', 'f64') else '')
  return _as_dict(getattr(R, name)(pd, inputs(entry, p)) if hasattr(R, name) else _typed_bias_act(pd, inputs(entry, p)))


def _typed_bias_act(p, a):
  """fused_bias_act on half / double tensors, from R.fused_bias_act (k = 4).  f64: the same count in units of 2^-53.  f16: the
  float32 result rounded to half once, 2^-11 |want| + 4 u B + 2^-25 (half the spacing of the subnormal halves)."""
  want, B, k, _ = R.fused_bias_act(p, a)
  if p['dtype'] == 'f64':
    return R.Ref(want, B * 2.0 ** -29, k, 0.0)
  return R.Ref(want, (2.0 ** -11 * np.abs(want) + k * U * B + 2.0 ** -25) / U, 1, 0.0)


def restatement(entry, p):
  """The float32 numpy restatement of a case -> {output: array}."""
  e, pd, a = ENTRIES[entry], dict(p), inputs(entry, p)
  if e.base == 'fused_bias_act':
    dt = {'f32': np.float32, 'f16': np.float32, 'f64': np.float64}[pd['dtype']]
    y = R._bias_act(pd, a, dt)[0]
    return {'out': y.astype(np.float16) if pd['dtype'] == 'f16' else y}
  return _as_dict(getattr(R, e.base + '_f32')(pd, a))


def _as_dict(r):
  return r if isinstance(r, dict) else {'out': r}


# ---- launches ---------------------------------------------------------------------------------------------------------
class Launch:
  """The operands of one call, each in a Guarded buffer placed as the case says: `where` is a placement of all streamed
  operands, or 'out-one-in' / 'in-one-in' (the outputs alone / the first input alone entered one element in).  Row vectors,
  the bias and other operands read one scalar at a time are `aux`: always aligned."""

  def __init__(self, lib, where):
    self.lib, self.dev, self.where, self.guards, self.first_in = lib, dev_of(lib), where, [], True

  def _place(self, arr, role):
    if arr is None:
      return None
    if role == 'aux':
      placement = 'aligned'
    elif self.where == 'out-one-in':
      placement = 'entered-one-in' if role == 'out' else 'aligned'
    elif self.where == 'in-one-in':
      placement = 'entered-one-in' if role == 'in' and self.first_in else 'aligned'
    else:
      placement = self.where
    if role == 'in':
      self.first_in = False
    g = Guarded(arr, self.dev, placement)
    self.guards.append((g, arr if role != 'out' and arr.size <= 4099 else None))
    return g.view

  def inp(self, arr): return self._place(arr, 'in')
  def out(self, arr): return self._place(arr, 'out')
  def aux(self, arr): return self._place(arr, 'aux')

  def call(self, name, *args):
    call(self.lib, name, *args)

  def done(self, what, **outs):
    if self.lib.is_device:
      torch.cuda.synchronize()
    for g, orig in self.guards:
      g.check(what)
      if orig is not None:
        assert np.array_equal(g.view.cpu().numpy().reshape(-1), orig.reshape(-1)), f'{what}: an input was written'
    return {k: v.cpu().numpy() for k, v in outs.items() if v is not None}


def _old(p, a, name, shape):
  """An accumulated output as the call finds it: NaN at beta = 0 (it must not be read), the old values otherwise."""
  return _nan(*shape) if p['beta'] == 0.0 else a[name].reshape(shape).copy()


# One runner per entry: (L, p, a) -> {output: device tensor}.  L places the operands, p are the case's parameters, a its host
# operands.  RUNNERS maps the base name of an entry (Entry.base) to its runner; run() below does the rest.
def _run_act_fwd(L, p, a):
  n = p['n']
  x, y = L.inp(a['x']), L.out(_nan(n))
  if 'act' in p:
    L.call('act_fwd_f32', x, y, n, p['act'])
  else:
    L.call('silu_fwd_f32', x, y, n)
  return dict(out=y)


def _run_act_bwd(L, p, a):
  n = p['n']
  x, dy, dx = L.inp(a['x']), L.inp(a['dy']), L.out(_old(p, a, 'dx0', (n,)))
  if 'act' in p:
    L.call('act_bwd_f32', x, dy, dx, p['beta'], n, p['act'])
  else:
    L.call('silu_bwd_f32', x, dy, dx, p['beta'], n)
  return dict(out=dx)


def _run_axpby(L, p, a):
  n = p['n']
  x = L.inp(a['a'])
  if p['variant'] == 'separate':
    y, out = L.inp(a['b']), L.out(_nan(n))
  elif p['variant'] == 'alias':                    # out is b: NaN there at beta = 0
    out = y = L.out(_old(p, a, 'b', (n,)))
  else:                                            # b = NULL
    y, out = None, L.out(_nan(n))
  L.call('axpby_f32', x, p['alpha'], y, p['beta'], out, n)
  return dict(out=out)


def _run_add_div(L, p, a):
  x, y, out = L.inp(a['a']), L.inp(a['b']), L.out(_nan(p['n']))
  L.call('add_div_f32', x, y, p['div'], out, p['n'])
  return dict(out=out)


def _run_affine(L, p, a):
  x, out = L.inp(a['x']), L.out(_nan(p['n']))
  L.call('affine_f32', x, p['a'], p['b'], out, p['n'])
  return dict(out=out)


def _run_fill(L, p, a):
  out = L.out(_nan(p['n']))
  L.call('fill_f32', out, p['v'], p['n'])
  return dict(out=out)


def _run_dropout_mask(L, p, a):
  out = L.out(_nan(p['n']))
  L.call('dropout_mask_f32', out, p['n'], p['p'], p['seed'])
  return dict(out=out)


def _run_fused_bias_act(L, p, a):
  n = p['n']
  ops = [L.inp(a['x']), L.aux(a['b']), L.inp(a['ref']), L.out(_nan(n, dtype=a['x'].dtype))]
  out = ops[3]
  if p['dtype'] == 'f16':                          # _util.call takes no half tensors: hand it the addresses
    ops = [None if t is None else t.data_ptr() for t in ops]
  L.call('fused_bias_act_' + p['dtype'], *ops, n, p['step_b'], p['size_b'], p['act'], p['grad'], p['alpha'], p['scale'])
  return dict(out=out)


def _run_rowscale(L, p, a):
  out = L.out(_nan(p['N'] * p['inner']))
  L.call('rowscale_f32', L.inp(a['x']), L.aux(a['s']), out, p['N'], p['inner'], p['mode'])
  return dict(out=out)


def _run_perturb(L, p, a):
  out = L.out(_nan(p['N'] * p['inner']))
  L.call('perturb_f32', L.inp(a['x']), L.inp(a['z']), L.aux(a['a']), L.aux(a['s']), out, p['N'], p['inner'])
  return dict(out=out)


def _run_sm_loss_bwd(L, p, a):
  out = L.out(_nan(p['N'] * p['inner']))
  L.call('sm_loss_bwd_f32', L.inp(a['net']), L.inp(a['z']), L.aux(a['std']), L.aux(a['wgt']), L.aux(a['dloss']), out,
         p['N'], p['inner'], p['vp'], p['mode'], p['rm'])
  return dict(out=out)


def _run_sm_loss_fwd(L, p, a):
  out = L.out(_nan(p['N']))
  L.call('sm_loss_fwd_f32', L.inp(a['net']), L.inp(a['z']), L.aux(a['std']), L.aux(a['wgt']), out, p['N'], p['inner'],
         p['vp'], p['mode'], p['rm'])
  return dict(out=out)


def _run_timestep_embedding(L, p, a):
  out = L.out(_nan(p['B'], p['dim']))
  L.call('timestep_embedding_f32', L.inp(a['t']), L.inp(a['freqs']), out, p['B'], p['dim'])
  return dict(out=out)


def _run_fourier_embedding(L, p, a):
  out = L.out(_nan(p['B'], 2 * p['nf']))
  L.call('fourier_embedding_f32', L.inp(a['x']), L.inp(a['W']), out, p['B'], p['nf'])
  return dict(out=out)


def _run_fourier_embedding_bwd(L, p, a):
  dx = L.out(_old(p, a, 'dx0', (p['B'],)))
  L.call('fourier_embedding_bwd_f32', L.inp(a['W']), L.inp(a['y']), L.inp(a['dy']), dx, p['beta'], p['B'], p['nf'])
  return dict(out=dx)


def _run_fixed_fourier_fwd(L, p, a):
  N, C, HW = p['N'], p['C'], p['HW']
  out = L.out(_nan(N, 5, C * HW))
  L.call('fixed_fourier_fwd_f32', L.inp(a['x']), out, N, C, HW)
  return dict(out=out)


def _run_fixed_fourier_bwd(L, p, a):
  N, C, HW = p['N'], p['C'], p['HW']
  dx = L.out(_old(p, a, 'dx0', (N, C * HW)))
  L.call('fixed_fourier_bwd_f32', L.inp(a['x']), L.inp(a['dy']), dx, p['beta'], N, C, HW)
  return dict(out=dx)


def _run_concat(L, p, a):
  N, Ca, Cb, HW = p['N'], p['Ca'], p['Cb'], p['HW']
  out = L.out(_nan(N, (Ca + Cb) * HW))
  L.call('concat_f32', L.inp(a['a']), Ca, L.inp(a['b']), Cb, out, N, HW)
  return dict(out=out)


def _run_concat_bwd(L, p, a):
  N, Ca, Cb, HW, beta = p['N'], p['Ca'], p['Cb'], p['HW'], p['beta']
  da = None if p['null'] == 'da' else L.out(_old(p, a, 'da0', (N, Ca * HW)))
  db = None if p['null'] == 'db' else L.out(_old(p, a, 'db0', (N, Cb * HW)))
  L.call('concat_bwd_f32', L.inp(a['dout']), da, beta, Ca, db, beta, Cb, N, HW)
  return dict(da=da, db=db)


def _run_resample_naive(L, p, a):
  P, H, W = p['planes'], p['H'], p['W']
  out = L.out(_old(p, a, 'out0', (P, 2 * H, 2 * W) if p['mode'] == 0 else (P, H // 2, W // 2)))
  L.call('resample_naive_f32', L.inp(a['in']), out, P, H, W, p['mode'], p['alpha'], p['beta'])
  return dict(out=out)


def _run_fill_strided(L, p, a):
  out = L.out(a['out0'].copy())                    # the gaps between the runs must keep what they hold
  L.call('fill_strided_f32', out, p['v'], p['count'], p['len'], p['stride'])
  return dict(out=out)


def _run_samples_to_uint8(L, p, a):
  out = L.out(np.full((p['N'], p['HW'], p['C']), 0x5A, dtype=np.uint8))
  L.call('samples_to_uint8', L.inp(a['x']), out, p['N'], p['C'], p['HW'])
  return dict(out=out)


def _run_preprocess_u8(L, p, a):
  out = L.out(_nan(p['N'], p['C'], p['H'], p['W']))
  L.call('preprocess_u8', L.inp(a['img']), out, p['N'], p['C'], p['H'], p['W'], p['flip'], p['dequant'], p['centered'],
         p['seed'])
  return dict(out=out)


RUNNERS = {
  'silu_fwd': _run_act_fwd, 'act_fwd': _run_act_fwd, 'silu_bwd': _run_act_bwd, 'act_bwd': _run_act_bwd,
  'axpby': _run_axpby, 'add_div': _run_add_div, 'affine': _run_affine, 'fill': _run_fill,
  'dropout_mask': _run_dropout_mask, 'fused_bias_act': _run_fused_bias_act, 'rowscale': _run_rowscale,
  'perturb': _run_perturb, 'sm_loss_bwd': _run_sm_loss_bwd, 'sm_loss_fwd': _run_sm_loss_fwd,
  'timestep_embedding': _run_timestep_embedding, 'fourier_embedding': _run_fourier_embedding,
  'fourier_embedding_bwd': _run_fourier_embedding_bwd, 'fixed_fourier_fwd': _run_fixed_fourier_fwd,
  'fixed_fourier_bwd': _run_fixed_fourier_bwd, 'concat': _run_concat, 'concat_bwd': _run_concat_bwd,
  'resample_naive': _run_resample_naive, 'fill_strided': _run_fill_strided, 'samples_to_uint8': _run_samples_to_uint8,
  'preprocess_u8': _run_preprocess_u8,
}


def run(lib, case):
  """Run one case on lib -> {output: numpy array}; the guards are checked, and so is that no input was written."""
  L = Launch(lib, case.where)
  outs = RUNNERS[ENTRIES[case.entry].base](L, params(case), inputs(case.entry, case.p))
  return L.done(case_name(case), **outs)


# ---- the check --------------------------------------------------------------------------------------------------------
def _bits(x):
  return np.ascontiguousarray(x).reshape(-1).view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def check(case, got, show=False):
  """Hold the outputs of one case to its reference -> (worst (err - floor) / (u B) over the outputs, its k); bit for bit where
  k = 0."""
  p, what, worst = params(case), case_name(case), (0.0, 0)
  ref = reference(case.entry, case.p)
  if ENTRIES[case.entry].base == 'preprocess_u8' and p['dequant']:
    return _check_dequant(p, got['out'], ref['out'].want, what)
  for name, g in got.items():
    r = ref[name]
    if r.k == 0:
      assert g.dtype == r.want.dtype and g.size == r.want.size, (what, name, g.dtype, g.shape)
      bad = np.flatnonzero(_bits(g) != _bits(r.want))
      assert bad.size == 0, f'{what} {name}: {bad.size} elements differ in their bits, the first at {bad[0]}: ' \
                            f'{g.reshape(-1)[bad[0]]!r} for {r.want.reshape(-1)[bad[0]]!r}'
      continue
    mag = np.asarray(r.B, dtype=np.float64) + np.asarray(r.floor, dtype=np.float64) / (r.k * U)
    g64, want = np.ascontiguousarray(g).reshape(-1).astype(np.float64), np.asarray(r.want).reshape(-1)
    within(torch.from_numpy(g64), want, np.array(np.broadcast_to(mag, np.shape(r.want))).reshape(-1), r.k, f'{what} {name}', show)
    # the figure reported: what the error takes of k u B once the floor is spent (a flushed subnormal is no rounding error)
    over = np.maximum(np.abs(g64 - want) - np.broadcast_to(r.floor, np.shape(r.want)).reshape(-1), 0.0)
    B = np.broadcast_to(np.asarray(r.B, dtype=np.float64), np.shape(r.want)).reshape(-1)
    units = float((over[B > 0] / (U * B[B > 0])).max()) if (B > 0).any() else 0.0
    worst = max(worst, (units, r.k))
  _extra(case, p, got)
  return worst


def _check_dequant(p, got, v, what):
  """Uniform dequantisation: w = (255 v + r) / 256 with r in [0, 1) lies in [lo, hi] = [255 v, 255 v + 1] / 256 before
  centring.  The float32 sum may round ONTO the upper end, which is why it is closed here.  What the ends are met to: the
  product 255 v and the sum round once each, u of their own magnitude <= 256 hi, and the factor 1 / 256 is exact: 2 u hi;
  one unit more for the second-order terms: 3 u hi.  Centred, the output is 2 w - 1: 2 w is exact and the difference
  rounds once, u |2 w - 1| <= u absolute, which the inversion (got + 1) / 2 halves: u / 2 more, absolute."""
  g = got.astype(np.float64).reshape(-1)
  if p['centered']:
    g = (g + 1.0) / 2.0
  lo, hi = 255.0 * v.astype(np.float64).reshape(-1) / 256.0, (255.0 * v.astype(np.float64).reshape(-1) + 1.0) / 256.0
  tol = 3 * U * hi + (U / 2 if p['centered'] else 0.0)
  assert np.isfinite(g).all() and (g >= lo - tol).all() and (g <= hi + tol).all(), f'{what}: outside [255 v, 255 v + 1] / 256'
  assert np.unique(got).size > got.size // 4, f'{what}: the draws repeat'
  return (0.0, 0)


def _extra(case, p, got):
  if ENTRIES[case.entry].base == 'dropout_mask':
    m, n, drop = got['out'], p['n'], p['p']
    ks = np.float32(1) / (np.float32(1) - np.float32(drop))
    assert np.isin(m, (np.float32(0), ks)).all(), f'{case_name(case)}: a value outside {{0, 1 / (1 - p)}}'
    kept = float((m != 0).mean())
    assert abs(kept - (1.0 - drop)) <= 6.0 * math.sqrt(drop * (1.0 - drop) / n), f'{case_name(case)}: kept {kept}'
    assert drop != 0.0 or kept == 1.0
  if ENTRIES[case.entry].base == 'timestep_embedding' and p['dim'] % 2:
    assert not got['out'][:, -1].any() and not np.signbit(got['out'][:, -1]).any(), 'the last column of an odd dim is exactly 0'


def check_null_matches_full(lib, case):
  """concat_bwd with one output absent: the present one is bit-identical to the full call's."""
  p = params(case)
  if case.entry != 'concat_bwd' or not p['null']:
    return
  full = run(lib, case._replace(p=tuple(sorted(dict(p, null='').items()))))
  part = run(lib, case)
  assert list(part) == ['db' if p['null'] == 'da' else 'da']
  for name, g in part.items():
    assert np.array_equal(_bits(g), _bits(full[name])), f'{case_name(case)}: {name} differs from the full call'
