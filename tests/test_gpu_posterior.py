"""The entries of include/stk_posterior.h (csrc/posterior.hip) through ctypes against the restatement of tests/_posterior_ref.py,
on the device.

Each element-wise result is held to k u B per element (u = 2^-24, B the expression on absolute values, k the roundings on the
longest path, counted in _posterior_ref.py; the test holds K = k + 1 because gamma_k < (k + 1) u):
  x0 k = 4, r k = 1, seed k = 3, x_out and x_mean k = 5.
The entries use no fused multiply-add and the build divides with correct rounding, so every element-wise result must also
equal the fp32 restatement bit for bit; that is asserted too.  rnorm is held to 2 x 2^-24 relative of the float64 root of the
float64 sum of the fp32 squares (the sum's own error is some 2^-53 per term, the root is rounded to fp32 once), and must be
bit-identical over two calls.

Shapes: the 16-byte path; the same entered one element into its buffer (scalar path); rows of 105 (unaligned row starts); one
element; rows of 3072 = three blocks of 256 lanes x 4 elements on the 16-byte path and twelve on the scalar one, so partial
sums are combined; 2049 rows, more than the 33 the grid walks at once.  Measurements of k = 5 and k = 48 floats per row (k
!= n), and one of 3072 per row on both paths (several partial sums per row).

Worst measured (MI355X): see MEASURED.
"""
import math

import numpy as np
import pytest
import torch

import _posterior_ref as R
from _stream_util import case_id, place, stream as _stream, within

pytestmark = pytest.mark.gpu

MEASURED = """MI355X, one run of this file (10 passed in under 2 s), worst over the seven cases, in u B:
x0 2.67 (bound 5), r 1.00 (bound 2), seed 2.53 (bound 4), x_out and x_mean 2.32 (bound 6); rnorm 0.99 x 2^-24 relative (bound 2),
bit-identical over two calls; every element-wise result equals the fp32 restatement bit for bit."""

EINVAL, EUNSUPPORTED = -1, -3
LO, HI = -1.0, 1.0
ZETA = float(np.float32(0.7))
SHAPES = [((2, 3, 8, 8), False), ((2, 3, 8, 8), True), ((3, 3, 5, 7), False), ((1, 1, 1, 1), False), ((2, 3, 32, 32), False),
          ((2, 3, 32, 32), True), ((2049, 1, 2, 2), False)]
ROWS = (5, 48)


def _operands(shape, seed):
  """fp32 host operands of one guided step.  x0 of the seed and of the update is the fp32 restatement of the data prediction
  under the clamp [-1, 1], so a good part of it sits at either bound; sample 0 of every measurement has y = m (r = 0)."""
  g = torch.Generator().manual_seed(seed)
  N = shape[0]
  rn = lambda *s: torch.randn(*s, generator=g)
  op = dict(x=1.5 * rn(*shape), score=rn(*shape), v=rn(*shape), gnet=0.3 * rn(*shape), xp=rn(*shape), xpm=rn(*shape),
            a=torch.rand(N, generator=g) * 0.7 + 0.3, s=torch.rand(N, generator=g) * 2.95 + 0.05)
  op['x0'] = R.tweedie(op['x'], op['score'], op['a'], op['s'], LO, HI)
  for k in ROWS + ((3072,) if shape == (2, 3, 32, 32) else ()):
    op[f'y{k}'], op[f'm{k}'] = rn(N, k), rn(N, k)
    op[f'y{k}'][0] = op[f'm{k}'][0]
  return op


@pytest.fixture(scope='module')
def cases():
  """Operands per shape: computed once, never written."""
  return {shape: _operands(shape, seed=sum(shape)) for shape in sorted({s for s, _ in SHAPES})}


def _f64(op):
  return {k: v.double() for k, v in op.items()}


class _Step:
  """The device buffers of one guided step and the four launches on them."""

  def __init__(self, lib, op, dev, shifted=False):
    self.lib, self.dev, self.shifted = lib, dev, shifted
    self.shape = tuple(op['x'].shape)
    self.N, self.n = self.shape[0], int(np.prod(self.shape[1:]))
    for name, t in op.items():
      setattr(self, name, place(t, dev, shifted and t.dim() > 1))

  def fresh(self, shape=None):
    return place(torch.full(shape or self.shape, float('nan')), self.dev, self.shifted)

  def tweedie(self, lo, hi):
    out = self.fresh()
    self.lib.tweedie_f32(self.x.data_ptr(), self.score.data_ptr(), self.a.data_ptr(), self.s.data_ptr(), lo, hi, out.data_ptr(),
                         self.N, self.n, _stream())
    return out

  def workspace(self, k):
    nbytes = self.lib.posterior_ws_bytes(self.N, k)
    assert nbytes > 0 and nbytes % 8 == 0
    return torch.full((nbytes // 8,), float('nan'), dtype=torch.float64, device=self.dev), nbytes

  def residual(self, k):
    y, m = getattr(self, f'y{k}'), getattr(self, f'm{k}')
    r = self.fresh((self.N, k))
    ws, nbytes = self.workspace(k)
    self.lib.residual_f32(y.data_ptr(), m.data_ptr(), r.data_ptr(), ws.data_ptr(), nbytes, self.N, k, _stream())
    return r, ws, nbytes

  def seed(self, ws, nbytes, k, lo=LO, hi=HI):
    out = self.fresh()
    rnorm = torch.full((self.N,), float('nan'), device=self.dev)
    self.lib.guide_seed_f32(self.v.data_ptr(), self.x0.data_ptr(), self.a.data_ptr(), self.s.data_ptr(), lo, hi, ws.data_ptr(),
                            nbytes, k, out.data_ptr(), rnorm.data_ptr(), self.N, self.n, _stream())
    return out, rnorm

  def update(self, rnorm, xp=None, xpm='own', x_out=None, xmean_out=None, zeta=ZETA, lo=LO, hi=HI):
    xp = self.xp if xp is None else xp
    xpm = self.xpm if isinstance(xpm, str) else xpm
    x_out = self.fresh() if x_out is None else x_out
    if xpm is not None and xmean_out is None:
      xmean_out = self.fresh()
    self.lib.guide_update_f32(xp.data_ptr(), xpm.data_ptr() if xpm is not None else None, self.v.data_ptr(), self.gnet.data_ptr(),
                              self.x0.data_ptr(), self.a.data_ptr(), rnorm.data_ptr(), zeta, lo, hi, x_out.data_ptr(),
                              xmean_out.data_ptr() if xmean_out is not None else None, self.N, self.n, _stream())
    return x_out, xmean_out


def _same_bits(got, want, what):
  assert torch.equal(got.cpu(), want), f'{what}: not the fp32 restatement bit for bit'


@pytest.mark.parametrize('shape,shifted', SHAPES, ids=case_id)
def test_entries_match_float64(hip_lib, cases, shape, shifted):
  dev = torch.device('cuda:0')
  op = cases[shape]
  d = _f64(op)
  st = _Step(hip_lib, op, dev, shifted)
  what = f'{shape} shifted={shifted}'
  worst = {}

  # the data prediction, with and without the clamp
  mag = R.tweedie_mag(d['x'], d['score'], d['a'], d['s'])
  for lo, hi in ((-math.inf, math.inf), (LO, HI)):
    got = st.tweedie(lo, hi)
    key = 'x0' if lo == LO else 'x0 unclamped'
    worst[key] = within(got, R.tweedie(d['x'], d['score'], d['a'], d['s'], lo, hi), mag, R.K_X0, f'tweedie {what} [{lo}, {hi}]')
    _same_bits(got, R.tweedie(op['x'], op['score'], op['a'], op['s'], lo, hi), f'tweedie {what} [{lo}, {hi}]')
  assert torch.equal(got.cpu(), op['x0'])
  at_bound = (op['x0'] == LO) | (op['x0'] == HI)
  if op['x0'].numel() >= 100:
    assert bool((op['x0'] == LO).any()) and bool((op['x0'] == HI).any()) and not bool(at_bound.all())

  # the residual and its norm, for every measurement length
  norms = {}
  for k in [int(name[1:]) for name in op if name[0] == 'y']:
    y, m = d[f'y{k}'], d[f'm{k}']
    r, ws, nbytes = st.residual(k)
    assert bool(torch.isfinite(ws).all()), 'a slot of the workspace was not written'
    worst[f'r{k}'] = within(r, y - m, y.abs() + m.abs(), R.K_R, f'residual {what} k={k}')
    r32, want_norm = R.residual(op[f'y{k}'], op[f'm{k}'])
    _same_bits(r, r32, f'residual {what} k={k}')
    seed, rnorm = st.seed(ws, nbytes, k)
    got_norm = rnorm.cpu().double()
    rel = float(((got_norm - want_norm).abs() / want_norm.clamp_min(1e-300)).max())
    worst[f'rnorm{k}'] = rel / 2.0 ** -24
    assert rel <= 2 * 2.0 ** -24, f'rnorm {what} k={k}: {rel:.3e}'
    assert float(rnorm[0]) == 0.0, 'the sample with y = m'
    # a second pair of launches gives the same bits
    _, ws2, _ = st.residual(k)
    _, rnorm2 = st.seed(ws2, nbytes, k)
    assert torch.equal(ws, ws2) and torch.equal(rnorm, rnorm2), f'rnorm {what} k={k} differs between two calls'
    norms[k] = rnorm

    # the seed: the same whatever measurement the workspace belongs to
    key = f'seed{k}'
    worst[key] = within(seed, R.seed(d['v'], d['x0'], d['a'], d['s'], LO, HI), R.seed_mag(d['v'], d['a'], d['s']), R.K_SEED,
                        f'guide_seed {what} k={k}')
    _same_bits(seed, R.seed(op['v'], op['x0'], op['a'], op['s'], LO, HI), f'guide_seed {what} k={k}')
    assert bool((seed.cpu()[at_bound] == 0).all()), 'an element at a clamp bound received a seed'

  # the update, on the norm of the last measurement
  rnorm = norms[k]
  rn32, rn64 = rnorm.cpu(), rnorm.cpu().double()
  x_out, x_mean = st.update(rnorm)
  mag = R.update_mag(d['xp'], d['v'], d['gnet'], d['a'], rn64, ZETA)
  worst['x_out'] = within(x_out, R.update(d['xp'], d['v'], d['gnet'], d['x0'], d['a'], rn64, ZETA, LO, HI), mag, R.K_OUT,
                          f'guide_update {what} x')
  mag_m = R.update_mag(d['xpm'], d['v'], d['gnet'], d['a'], rn64, ZETA)
  worst['x_mean'] = within(x_mean, R.update(d['xpm'], d['v'], d['gnet'], d['x0'], d['a'], rn64, ZETA, LO, HI), mag_m, R.K_OUT,
                           f'guide_update {what} x_mean')
  want32 = R.update(op['xp'], op['v'], op['gnet'], op['x0'], op['a'], rn32, ZETA, LO, HI)
  _same_bits(x_out, want32, f'guide_update {what} x')
  _same_bits(x_mean, R.update(op['xpm'], op['v'], op['gnet'], op['x0'], op['a'], rn32, ZETA, LO, HI), f'guide_update {what} x_mean')
  # r = 0: c = 0 and the sample stays what the unconditional update gave, bit for bit
  assert torch.equal(x_out[0], st.xp[0]) and torch.equal(x_mean[0], st.xpm[0])
  if st.N > 1:
    assert not torch.equal(x_out[1], st.xp[1])
  # where x0 sits at a bound, g = gnet
  c = R.wide(R.step_size(rn32, torch.tensor(ZETA)), op['xp'])
  assert torch.equal(x_out.cpu()[at_bound], (op['xp'] + c * op['gnet'])[at_bound])
  # NULL xpm: x_out alone, the same bits
  alone, none = st.update(rnorm, xpm=None)
  assert none is None and torch.equal(alone, x_out)
  # in place: x_out = xp and xmean_out = xpm
  xp, xpm = (place(op[name], dev, shifted) for name in ('xp', 'xpm'))
  st.update(rnorm, xp=xp, xpm=xpm, x_out=xp, xmean_out=xpm)
  assert torch.equal(xp, x_out) and torch.equal(xpm, x_mean), 'in place differs from out of place'
  # the operands were not written
  for name, t in op.items():
    assert torch.equal(getattr(st, name).cpu(), t), f'{what}: operand {name} was written'
  print(f'{what}: ' + ', '.join(f'{k} {v:.2f}' for k, v in worst.items()) + '  (u B; rnorm in 2^-24 relative)')


def test_workspace_is_a_function_of_the_sizes(hip_lib):
  q = hip_lib.posterior_ws_bytes
  assert q(2, 5) == 16 and q(2, 48) == 16 and q(1, 1) == 8 and q(2049, 48) == 2049 * 8
  assert q(2, 3072) == 2 * 12 * 8        # twelve blocks of 256 scalar lanes per row: the layout does not depend on the path
  assert q(0, 5) == EINVAL and q(2, 0) == EINVAL and q(-1, 5) == EINVAL
  assert q(2, 2 ** 30) == EUNSUPPORTED and q(1, 2 ** 31) == EUNSUPPORTED
  assert q(1, 2 ** 31 - 1) > 0


def test_refusals(hip_lib, cases):
  """Every refusal of the header, returned before anything is launched: the outputs keep their NaNs."""
  dev = torch.device('cuda:0')
  op = cases[(2, 3, 8, 8)]
  st = _Step(hip_lib, op, dev)
  L = hip_lib
  N, n, k = st.N, st.n, 5
  s = _stream()
  nan, inf = float('nan'), math.inf
  out, out2 = st.fresh(), st.fresh()
  r = st.fresh((N, k))
  rnorm = torch.full((N,), nan, device=dev)
  ws, nbytes = st.workspace(k)
  p = lambda t: t.data_ptr()
  x, score, a, sd, v, x0, gnet, xp, xpm, y, m = (p(getattr(st, name)) for name in
                                                 ('x', 'score', 'a', 's', 'v', 'x0', 'gnet', 'xp', 'xpm', 'y5', 'm5'))
  big = 2 ** 31

  tweedie = lambda *, x=x, score=score, a=a, sd=sd, lo=LO, hi=HI, o=p(out), N=N, n=n: \
      L.tweedie_f32.raw(x, score, a, sd, lo, hi, o, N, n, s)
  for kw in (dict(x=None), dict(score=None), dict(a=None), dict(sd=None), dict(o=None), dict(N=0), dict(N=-2), dict(n=0),
             dict(lo=1., hi=-1.), dict(lo=nan), dict(hi=nan)):
    assert tweedie(**kw) == EINVAL, kw
  assert tweedie(n=big) == EUNSUPPORTED and tweedie(N=2 ** 16, n=2 ** 15) == EUNSUPPORTED
  assert tweedie(lo=0.5, hi=0.5) == 0 and tweedie(lo=-inf, hi=inf) == 0          # lo == hi is a clamp; no clamp
  out.fill_(nan)

  residual = lambda *, y=y, m=m, r=p(r), w=p(ws), nb=nbytes, N=N, k=k: L.residual_f32.raw(y, m, r, w, nb, N, k, s)
  for kw in (dict(y=None), dict(m=None), dict(r=None), dict(w=None), dict(N=0), dict(k=0), dict(k=-1), dict(nb=nbytes - 1),
             dict(nb=0), dict(w=p(ws) + 4)):
    assert residual(**kw) == EINVAL, kw
  assert residual(k=big) == EUNSUPPORTED and residual(N=2 ** 16, k=2 ** 15) == EUNSUPPORTED
  assert bool(torch.isnan(r).all()) and bool(torch.isnan(ws).all())
  assert residual() == 0

  seed = lambda *, v=v, x0=x0, a=a, sd=sd, lo=LO, hi=HI, w=p(ws), nb=nbytes, k=k, o=p(out), rn=p(rnorm), N=N, n=n: \
      L.guide_seed_f32.raw(v, x0, a, sd, lo, hi, w, nb, k, o, rn, N, n, s)
  for kw in (dict(v=None), dict(x0=None), dict(a=None), dict(sd=None), dict(w=None), dict(o=None), dict(rn=None), dict(N=0),
             dict(n=0), dict(k=0), dict(lo=1., hi=-1.), dict(lo=nan), dict(hi=nan), dict(nb=nbytes - 1), dict(w=p(ws) + 4),
             dict(k=3072)):           # a workspace sized for k = 5 is too small for rows of 3072
    assert seed(**kw) == EINVAL, kw
  assert seed(n=big) == EUNSUPPORTED and seed(k=big) == EUNSUPPORTED
  assert bool(torch.isnan(out).all()) and bool(torch.isnan(rnorm).all())
  assert seed() == 0

  update = lambda *, xp=xp, xpm=xpm, v=v, gnet=gnet, x0=x0, a=a, rn=p(rnorm), zeta=ZETA, lo=LO, hi=HI, o=p(out), om=p(out2), \
      N=N, n=n: L.guide_update_f32.raw(xp, xpm, v, gnet, x0, a, rn, zeta, lo, hi, o, om, N, n, s)
  out.fill_(nan)
  for kw in (dict(xp=None), dict(v=None), dict(gnet=None), dict(x0=None), dict(a=None), dict(rn=None), dict(o=None),
             dict(xpm=None), dict(om=None),          # the mean's operand and output come together or not at all
             dict(N=0), dict(n=0), dict(zeta=-1.), dict(zeta=nan), dict(lo=1., hi=-1.), dict(lo=nan), dict(hi=nan)):
    assert update(**kw) == EINVAL, kw
  assert update(n=big) == EUNSUPPORTED
  assert bool(torch.isnan(out).all()) and bool(torch.isnan(out2).all())
  assert update(zeta=0.) == 0 and update(xpm=None, om=None) == 0
  torch.cuda.synchronize()
