"""The three entries of include/stk_adaptive.h (csrc/adaptive.hip) and the adaptive-step SDE sampler built on them, on the
device.

The kernels against float64, the same fp32 coefficient rows given to both sides.  x1 and x2 are held to the forward rounding
bound gamma_k B of their expressions, not to a blanket tolerance: B is the expression on absolute values, k the number of
roundings on the longest path from an operand to the result, gamma_k = k u / (1 - k u), u = 2^-24.
  x1 = (a x + s score) + n z:                 product, sum, sum: k = 3; with the xp term one more sum: k = 4
  x2 = 0.5 (x1 + (((a x + p x1) + s s2) + n z)): product, three sums, the sum with x1: k = 5 (the halving is exact)
The test holds K = k + 1 (gamma_k < (k + 1) u).  The entries use no fused multiply-add, so x1 and x2 must also equal the
numpy fp32 restatement bit for bit; that is asserted too.

E_b against float64: the tolerance is measured, not fixed: four times the deviation of the numpy fp32 restatement
(tests/_adaptive_ref.py) from float64 on the same operands, the project's standing margin for "fp32 arithmetic alone".  Both
figures are printed.  MI355X values: see MEASURED.

The decisions: no decision is excluded from any comparison; the operands are built so that the float64 E lies away from 1 by
at least 100 times the measured E tolerance, and the test asserts that of the reference's numbers.

The loop and the sampler are compared with by-hand torch loops on the device, in float64 and again in fp32, under the same
seed and draw order (one randn_like per iteration), after asserting the precondition that the two by-hand loops take the
identical accept / reject sequence and every float64 E of the run is at least 1e-3 from 1.
"""
import numpy as np
import pytest
import torch

import _adaptive_ref as R
from _sampler_util import sampler, setup, shape_of as _shape
from _stream_util import case_id, place, stream as _stream, within

pytestmark = pytest.mark.gpu

MEASURED = """MI355X, one run of this file (17 passed in 5.5 s):
kernels, worst over the seven cases: x1 2.24 u B (bound 4), with xp 2.79 (bound 5), x2 2.06 (bound 6); x1 and x2 equal the numpy
fp32 restatement bit for bit in every case.  E against float64 (product / numpy fp32 restatement, tolerance four times the
latter): (2,3,8,8) 4.94e-7 / 3.94e-7, aligned and entered one element in alike; (3,3,5,7) 1.50e-6 / 1.50e-6; (1,1,1,1)
1.29e-6 / 1.29e-6; (2,3,32,32) 1.69e-7 / 1.69e-7 on both paths; (16,3,256,256) 6.3e-8 / 1.23e-7.
decisions: float64 E = 0.291, 2.891, 0.647; measured E tolerance 1.57e-6.
loops (product / by-hand fp32 loop, relative to the float64 loop): closed-form score VP 66 iterations, 6.4e-7 / 1.18e-6,
closest float64 E to 1 7.8e-3; VE 113 iterations, 1.42e-6 / 5.41e-6, closest 4.0e-3; tiny network VP 31 iterations,
7.7e-7 / 1.48e-6, closest 1.9e-2; VE 33 iterations, 1.96e-6 / 1.88e-6, closest 3.9e-2.
fp16 against fp32, max |difference| of the samples: 0 on the vp and ve networks (no layer of theirs takes an fp16 form),
3.3e-3 on the wide one."""

K_X1, K_X1P, K_X2 = 4, 5, 6
EPS = 1e-3
EPS32 = float(np.float32(EPS))
ATOL, RTOL = 0.0078, 0.01
EINVAL, EUNSUPPORTED = -1, -3
F09 = float(np.float32(0.9))          # the controller's constants as the entry receives them
# the vector path; rows of 105, unaligned row starts and the scalar path; one element; the vector shape entered one element
# into its buffer (scalar path); rows of 3072 = three blocks of 256 lanes x 4 elements, so partial sums are combined (and
# twelve blocks on the scalar path); 2048 blocks, each striding along its row
SHAPES = [((2, 3, 8, 8), False), ((3, 3, 5, 7), False), ((1, 1, 1, 1), False), ((2, 3, 8, 8), True), ((2, 3, 32, 32), False),
          ((2, 3, 32, 32), True), ((16, 3, 256, 256), False)]


def _rows(B):
  """fp32 coefficient rows of a VP-like step, different per sample: (stage row with an xp term, heun row)."""
  h = 0.01 * (1. + 0.3 * np.arange(B))
  beta, beta2 = 10., 9.8
  a = np.stack([1. + 0.5 * h * beta, 0.05 + 0. * h, h * beta, np.sqrt(h * beta)], axis=1).astype(np.float32)
  b = np.stack([np.ones(B), 0.5 * h * beta2, h * beta2, np.sqrt(h * beta2)], axis=1).astype(np.float32)
  return a, b


def _operands(shape, seed, k=None):
  """fp32 host operands of one iteration, as a real step has them: x1 is the stage of (x, s1, z), and s2 is built so that
  x1 - x2 = k d u with u standard normal: E is k times the root mean square of u (k per sample, default 0.6)."""
  rng = np.random.RandomState(seed)
  B = shape[0]
  k = np.full(B, 0.6) if k is None else np.asarray(k, dtype=np.float64)
  row1, row2 = _rows(B)
  x = (1.5 * rng.standard_normal(shape)).astype(np.float32)
  s1 = (-x + 0.1 * rng.standard_normal(shape)).astype(np.float32)
  z = rng.standard_normal(shape).astype(np.float32)
  xp = rng.standard_normal(shape).astype(np.float32)
  x1 = R.stage(x, None, s1, z, row1)                        # fp32, every operation rounded
  assert x1.dtype == np.float32
  x1_prev = (x + 0.05 * rng.standard_normal(shape)).astype(np.float32)
  d = np.maximum(ATOL, RTOL * np.maximum(np.abs(x1.astype(np.float64)), np.abs(x1_prev.astype(np.float64))))
  col = lambda j: row2[:, j].astype(np.float64).reshape((-1,) + (1,) * (len(shape) - 1))
  kk = k.reshape((-1,) + (1,) * (len(shape) - 1))
  x64, x164, z64 = x.astype(np.float64), x1.astype(np.float64), z.astype(np.float64)
  s2 = ((x164 - x64 - col(1) * x164 - col(3) * z64) - 2. * kk * d * rng.standard_normal(shape)) / col(2)
  return dict(x=x, xp=xp, s1=s1, z=z, x1=x1, x1_prev=x1_prev, s2=s2.astype(np.float32), row1=row1, row2=row2)


def _reference(op):
  """float64 and numpy-fp32 results of the two element-wise entries on the fp32 operands `op`."""
  f64 = {k: v.astype(np.float64) for k, v in op.items()}
  out = {}
  for tag, o in (('f64', f64), ('f32', op)):
    x1 = R.stage(o['x'], None, o['s1'], o['z'], o['row1'])
    x1p = R.stage(o['x'], o['xp'], o['s1'], o['z'], o['row1'])
    x2, E = R.heun_error(o['x'], o['x1'], o['x1_prev'], o['s2'], o['z'], o['row2'], ATOL, RTOL)
    out[tag] = dict(x1=x1, x1p=x1p, x2=x2, E=E)
  a = np.abs(f64['row1']), np.abs(f64['row2'])
  col = lambda r, j: r[:, j].reshape((-1,) + (1,) * (op['x'].ndim - 1))
  ax, axp, as1, az, ax1, as2 = (np.abs(f64[k]) for k in ('x', 'xp', 's1', 'z', 'x1', 's2'))
  out['B_x1'] = col(a[0], 0) * ax + col(a[0], 2) * as1 + col(a[0], 3) * az
  out['B_x1p'] = out['B_x1'] + col(a[0], 1) * axp
  out['B_x2'] = 0.5 * (ax1 + col(a[1], 0) * ax + col(a[1], 1) * ax1 + col(a[1], 2) * as2 + col(a[1], 3) * az)
  own = np.abs(out['f32']['E'].astype(np.float64) - out['f64']['E']) / out['f64']['E']
  out['E_own'] = float(own.max())
  return out


@pytest.fixture(scope='module')
def cases():
  """Operands and references per shape: computed once, never written."""
  out = {}
  for shape in sorted({s for s, _ in SHAPES}):
    op = _operands(shape, seed=sum(shape))
    out[shape] = (op, _reference(op))
  return out


class _Step:
  """The device buffers of one iteration and the three launches on them."""

  def __init__(self, lib, op, dev, shifted=False):
    self.lib, self.shape = lib, op['x'].shape
    self.B, self.n = self.shape[0], int(np.prod(self.shape[1:]))
    for name in ('x', 'xp', 's1', 'z', 'x1', 'x1_prev', 's2'):
      setattr(self, name, place(op[name], dev, shifted))
    self.row1, self.row2 = place(op['row1'], dev), place(op['row2'], dev)
    nan = np.full(self.shape, np.nan, dtype=np.float32)
    self.out, self.x2 = place(nan, dev, shifted), place(nan, dev, shifted)
    self.ws_bytes = lib.sde_ws_bytes(self.B, self.n)
    assert self.ws_bytes > 0 and self.ws_bytes % 8 == 0
    self.ws = torch.full((self.ws_bytes // 8,), float('nan'), dtype=torch.float64, device=dev)
    self.t_out, self.h_out, self.E = (torch.full((self.B,), float('nan'), device=dev) for _ in range(3))
    self.accept = torch.full((self.B,), -7, dtype=torch.int32, device=dev)

  def stage(self, with_xp):
    self.lib.sde_stage_f32(self.x.data_ptr(), self.xp.data_ptr() if with_xp else None, self.s1.data_ptr(), self.z.data_ptr(),
                           self.row1.data_ptr(), self.out.data_ptr(), self.B, self.n, _stream())
    return self.out

  def heun(self):
    self.lib.sde_heun_error_f32(self.x.data_ptr(), self.x1.data_ptr(), self.x1_prev.data_ptr(), self.s2.data_ptr(),
                                self.z.data_ptr(), self.row2.data_ptr(), ATOL, RTOL, self.x2.data_ptr(), self.ws.data_ptr(),
                                self.ws_bytes, self.B, self.n, _stream())
    return self.x2

  def commit(self, t, h, x=None, x1_prev=None, safety=0.9, exponent=0.9):
    """On copies of x and x1_prev unless given: the operands stay as they are."""
    x = self.x.clone() if x is None else x
    x1_prev = self.x1_prev.clone() if x1_prev is None else x1_prev
    self.lib.sde_commit_f32(x.data_ptr(), x1_prev.data_ptr(), self.x2.data_ptr(), self.x1.data_ptr(), t.data_ptr(), h.data_ptr(),
                            EPS32, safety, exponent, self.ws.data_ptr(), self.ws_bytes, self.t_out.data_ptr(),
                            self.h_out.data_ptr(), self.E.data_ptr(), self.accept.data_ptr(), self.B, self.n, _stream())
    return x, x1_prev


@pytest.mark.parametrize('shape,shifted', SHAPES, ids=case_id)
def test_kernels_match_float64(hip_lib, cases, shape, shifted):
  dev = torch.device('cuda:0')
  op, ref = cases[shape]
  st = _Step(hip_lib, op, dev, shifted)
  what = f'{shape} shifted={shifted}'
  worst = {}
  for with_xp, key, K in ((False, 'x1', K_X1), (True, 'x1p', K_X1P)):
    got = st.stage(with_xp)
    worst[key] = within(got, ref['f64'][key], ref['B_' + key], K, f'stage {what} xp={with_xp}')
    assert np.array_equal(got.cpu().numpy(), ref['f32'][key]), f'stage {what} xp={with_xp}: not the fp32 restatement bit for bit'
  x2 = st.heun()
  worst['x2'] = within(x2, ref['f64']['x2'], ref['B_x2'], K_X2, f'heun_error {what}')
  assert np.array_equal(x2.cpu().numpy(), ref['f32']['x2']), f'heun_error {what}: x2 is not the fp32 restatement bit for bit'
  t = torch.full((st.B,), 0.5, device=dev)
  h = torch.full((st.B,), 0.01, device=dev)
  st.commit(t, h)
  E = st.E.cpu().double().numpy()
  err = float((np.abs(E - ref['f64']['E']) / ref['f64']['E']).max())
  print(f'{what}: x1 {worst["x1"]:.2f} u B (bound {K_X1}), with xp {worst["x1p"]:.2f} (bound {K_X1P}), x2 {worst["x2"]:.2f} '
        f'(bound {K_X2}); E deviates {err:.3e} from float64, the numpy fp32 restatement {ref["E_own"]:.3e}: tolerance '
        f'{4 * ref["E_own"]:.3e}; E64 = {ref["f64"]["E"][:3]}')
  assert err <= 4 * ref['E_own']
  # the operands were not written
  for name in ('x', 'xp', 's1', 'z', 'x1', 'x1_prev', 's2'):
    assert np.array_equal(getattr(st, name).cpu().numpy(), op[name]), f'{what}: operand {name} was written'
  assert np.array_equal(st.row1.cpu().numpy(), op['row1']) and np.array_equal(st.row2.cpu().numpy(), op['row2'])


@pytest.fixture(scope='module')
def decision_case():
  """Three samples: float64 E about 0.3 (accepted), about 3 (rejected), and a finished one (t = eps, h = 0)."""
  shape = (3, 3, 8, 8)
  op = _operands(shape, seed=7, k=[0.3, 3., 0.6])
  return op, _reference(op)


def _ulp_close(got, want):
  """Equal to within one unit in the last place of fp32 (the float64 powers of two libraries, rounded once)."""
  return abs(float(got) - float(want)) <= 2.0 ** -23 * abs(float(want))


def test_decisions(hip_lib, decision_case):
  dev = torch.device('cuda:0')
  op, ref = decision_case
  E64 = ref['f64']['E']
  tol = 4 * ref['E_own']
  print(f'decisions: E64 = {E64}, measured E tolerance {tol:.3e}')
  assert 0.25 < E64[0] < 0.35 and 2.5 < E64[1] < 3.5
  assert bool((np.abs(E64 - 1.) >= 100 * tol * E64).all()), 'a decision of the reference lies within 100 tolerances of 1'
  st = _Step(hip_lib, op, dev)
  st.heun()
  t = torch.tensor([0.5, 0.5, EPS32], device=dev)
  h = torch.tensor([0.01, 0.02, 0.], device=dev)
  x, x1_prev = st.commit(t, h)
  assert st.accept.cpu().tolist() == [1, 0, 0]
  E = st.E.cpu().double().numpy()
  assert float((np.abs(E - E64) / E64).max()) <= tol
  assert torch.equal(x[0], st.x2[0]) and torch.equal(x1_prev[0], st.x1[0]), 'the accepted row is not x2 / x1'
  for b in (1, 2):
    assert torch.equal(x[b], st.x[b]) and torch.equal(x1_prev[b], st.x1_prev[b]), f'row {b} was written'
  t32, h32 = t.cpu().numpy(), h.cpu().numpy()
  t_out, h_out = st.t_out.cpu().numpy(), st.h_out.cpu().numpy()
  assert t_out[0] == t32[0] - h32[0] and t_out[1] == t32[1] and t_out[2] == np.float32(EPS32)
  assert h_out[2] == 0.
  for b in (0, 1):
    grown = np.float32(F09 * float(h32[b]) * E[b] ** -F09)
    assert grown < t_out[b] - np.float32(EPS32) and _ulp_close(h_out[b], grown), (b, h_out[b], grown)
  # other controller constants reach the rule
  st.commit(t, h, safety=0.5, exponent=0.25)
  assert _ulp_close(st.h_out[0].item(), np.float32(0.5 * float(h32[0]) * E[0] ** -0.25))     # 0.5 and 0.25 are fp32 numbers
  # a clamped accepted step lands on eps exactly, and the sample is finished; a growing step is clamped to what is left
  t = torch.tensor([0.011, 0.5, 0.0125], device=dev)
  h = torch.stack([t[0] - EPS32, t[1] - EPS32, torch.tensor(0.008, device=dev)])
  x, x1_prev = st.commit(t, h)
  assert st.accept.cpu().tolist() == [1, 0, 1]
  t_out, h_out = st.t_out.cpu().numpy(), st.h_out.cpu().numpy()
  assert t_out[0] == np.float32(EPS32) and h_out[0] == 0. and t_out[1] == np.float32(0.5)
  assert t_out[2] == np.float32(0.0125) - np.float32(0.008)
  assert np.float32(F09 * 0.008 * E[2] ** -F09) > t_out[2] - np.float32(EPS32) and h_out[2] == t_out[2] - np.float32(EPS32)
  assert torch.equal(x[2], st.x2[2]) and torch.equal(x[1], st.x[1])


def test_launches_are_deterministic(hip_lib, cases):
  """Two launches on the same operands: bit-identical E, x2, t and h (the partial sums are combined in a fixed order)."""
  dev = torch.device('cuda:0')
  for shape in ((2, 3, 32, 32), (16, 3, 256, 256)):
    op, _ = cases[shape]
    runs = []
    for _ in range(2):
      st = _Step(hip_lib, op, dev)
      st.heun()
      t = torch.full((st.B,), 0.5, device=dev)
      h = torch.full((st.B,), 0.01, device=dev)
      st.commit(t, h)
      runs.append((st.E.clone(), st.x2.clone(), st.t_out.clone(), st.h_out.clone(), st.ws.clone()))
    for a, b in zip(*runs):
      assert torch.equal(a, b), f'{shape}: two launches differ'
    assert bool(torch.isfinite(runs[0][4]).all()), 'a workspace slot was not written'


def test_return_codes_and_nothing_written(hip_lib, cases):
  """Every refusal returns before any launch: the outputs keep their sentinels."""
  dev = torch.device('cuda:0')
  op, _ = cases[(2, 3, 8, 8)]
  st = _Step(hip_lib, op, dev)
  B, n, p = st.B, st.n, (lambda t: None if t is None else t.data_ptr())
  t, h = torch.full((B,), 0.5, device=dev), torch.full((B,), 0.01, device=dev)
  st.ws.fill_(3.0)
  xc, pc = st.x.clone(), st.x1_prev.clone()

  def untouched():
    torch.cuda.synchronize()
    assert bool(torch.isnan(st.out).all()) and bool(torch.isnan(st.x2).all()) and bool((st.ws == 3.0).all())
    assert bool(torch.isnan(st.t_out).all()) and bool(torch.isnan(st.h_out).all()) and bool(torch.isnan(st.E).all())
    assert bool((st.accept == -7).all()) and torch.equal(xc, st.x) and torch.equal(pc, st.x1_prev)

  def stage(x=st.x, s=st.s1, z=st.z, c=st.row1, out=st.out, B=B, n=n):
    rc = hip_lib.sde_stage_f32.raw(p(x), None, p(s), p(z), p(c), p(out), B, n, _stream())
    untouched()
    return rc

  def heun(x=st.x, x1=st.x1, pv=st.x1_prev, s=st.s2, z=st.z, c=st.row2, atol=ATOL, rtol=RTOL, x2=st.x2, ws=st.ws, wb=st.ws_bytes, B=B, n=n):
    rc = hip_lib.sde_heun_error_f32.raw(p(x), p(x1), p(pv), p(s), p(z), p(c), atol, rtol, p(x2), p(ws), wb, B, n, _stream())
    untouched()
    return rc

  def commit(x=xc, pv=pc, x2=st.x2, x1=st.x1, t=t, h=h, eps=EPS32, safety=0.9, r=0.9, ws=st.ws, wb=st.ws_bytes, t_out=st.t_out,
             h_out=st.h_out, E=st.E, acc=st.accept, B=B, n=n):
    rc = hip_lib.sde_commit_f32.raw(p(x), p(pv), p(x2), p(x1), p(t), p(h), eps, safety, r, p(ws), wb, p(t_out), p(h_out), p(E),
                                    p(acc), B, n, _stream())
    untouched()
    return rc

  nan = float('nan')
  for name in ('x', 's', 'z', 'c', 'out'):
    assert stage(**{name: None}) == EINVAL, name
  for name in ('x', 'x1', 'pv', 's', 'z', 'c', 'x2', 'ws'):
    assert heun(**{name: None}) == EINVAL, name
  for name in ('x', 'pv', 'x2', 'x1', 't', 'h', 'ws', 't_out', 'h_out', 'E', 'acc'):
    assert commit(**{name: None}) == EINVAL, name
  for fn in (stage, heun, commit):
    assert fn(B=0) == EINVAL and fn(B=-1) == EINVAL and fn(n=0) == EINVAL and fn(n=-4) == EINVAL
    assert fn(n=2 ** 31) == EUNSUPPORTED and fn(n=2 ** 30) == EUNSUPPORTED and fn(n=2 ** 40) == EUNSUPPORTED
  assert heun(atol=-1.) == EINVAL and heun(rtol=-1.) == EINVAL and heun(atol=0., rtol=0.) == EINVAL
  assert heun(atol=nan) == EINVAL and heun(rtol=nan) == EINVAL
  assert heun(wb=st.ws_bytes - 8) == EINVAL and commit(wb=st.ws_bytes - 8) == EINVAL and heun(wb=0) == EINVAL
  odd = torch.empty(st.ws_bytes // 4 + 1, dtype=torch.float32, device=dev)[1:]
  assert odd.data_ptr() % 8 == 4 and heun(ws=odd) == EINVAL and commit(ws=odd) == EINVAL
  assert commit(t_out=t) == EINVAL and commit(h_out=h) == EINVAL and commit(t_out=h) == EINVAL and commit(h_out=t) == EINVAL
  assert commit(eps=-1.) == EINVAL and commit(eps=nan) == EINVAL and commit(safety=0.) == EINVAL and commit(safety=nan) == EINVAL
  assert commit(r=-0.5) == EINVAL and commit(r=nan) == EINVAL
  # the workspace query refuses the same sizes with the same codes
  q = hip_lib.sde_ws_bytes
  assert q(0, n) == EINVAL and q(-1, n) == EINVAL and q(B, 0) == EINVAL and q(B, 2 ** 31) == EUNSUPPORTED and q(B, 2 ** 30) == EUNSUPPORTED
  # the checked binding raises the package's error
  with pytest.raises(RuntimeError, match='stk_sde_stage_f32 failed'):
    hip_lib.sde_stage_f32(None, None, p(st.s1), p(st.z), p(st.row1), p(st.out), B, n, _stream())
  with pytest.raises(RuntimeError, match='stk_sde_heun_error_f32 failed'):
    hip_lib.sde_heun_error_f32(p(st.x), p(st.x1), p(st.x1_prev), p(st.s2), p(st.z), p(st.row2), 0., 0., p(st.x2), p(st.ws),
                               st.ws_bytes, B, n, _stream())
  with pytest.raises(RuntimeError, match='stk_sde_commit_f32 failed'):
    hip_lib.sde_commit_f32(p(xc), p(pc), p(st.x2), p(st.x1), p(t), p(h), EPS32, 0.9, 0.9, p(st.ws), st.ws_bytes, p(t), p(st.h_out),
                           p(st.E), p(st.accept), B, n, _stream())
  untouched()


# ---- by-hand loops on the device --------------------------------------------------------------------------------------
def _coefficients(kind, params, t):
  """(c, g) in closed form, torch, in the dtype of t."""
  if kind == 'vp':
    beta = params[0] + t * (params[1] - params[0])
    return -0.5 * beta, torch.sqrt(beta)
  lo, hi = params
  return torch.zeros_like(t), lo * (hi / lo) ** t * float(np.sqrt(2. * (np.log(hi) - np.log(lo))))


def _by_hand(score, x0, kind, params, dtype, rtol, atol, seed, max_iters=2000):
  """The algorithm in torch `dtype` on the device: score(x fp32-or-dtype, t) -> dtype.  One torch.randn_like of the fp32
  state per iteration, as the product draws it.  -> (x, iterations, accept rows, E rows)."""
  if isinstance(seed, tuple):                               # (host, device) generator states to restart from
    torch.set_rng_state(seed[0])
    torch.cuda.set_rng_state(seed[1])
  else:
    torch.manual_seed(seed)
  x = x0.clone().to(dtype)
  B = x.shape[0]
  bc = lambda v: v.reshape((-1,) + (1,) * (x.dim() - 1))
  eps = torch.tensor(EPS32, dtype=dtype, device=x.device)
  t = torch.ones(B, dtype=dtype, device=x.device)
  h = torch.minimum(torch.full_like(t, 0.01), t - eps)
  x1_prev = x.clone()
  accepts, Es = [], []
  while not bool((t <= eps).all()):
    assert len(Es) < max_iters
    z = torch.randn_like(x0).to(dtype)
    c, g = _coefficients(kind, params, t)
    x1 = bc(1 - h * c) * x + bc(h * g * g) * score(x, t) + bc(torch.sqrt(h) * g) * z
    t_next = torch.where(h >= t - eps, eps.expand_as(t), t - h)
    c2, g2 = _coefficients(kind, params, t_next)
    xt = x + bc(-(h * c2)) * x1 + bc(h * g2 * g2) * score(x1, t_next) + bc(torch.sqrt(h) * g2) * z
    x2 = 0.5 * (x1 + xt)
    d = torch.clamp(rtol * torch.maximum(x1.abs(), x1_prev.abs()), min=atol)
    E = torch.sqrt((((x1 - x2) / d) ** 2).reshape(B, -1).mean(dim=1))
    active = t > eps
    accept = active & (E <= 1)
    sel = bc(accept)
    x, x1_prev = torch.where(sel, x2, x), torch.where(sel, x1, x1_prev)
    t = torch.where(accept, t_next, t)
    h = torch.where(active, torch.minimum(t - eps, 0.9 * h * E ** -0.9), torch.zeros_like(h))
    accepts.append(accept.cpu().tolist())
    Es.append(E.double().cpu().numpy()[active.cpu().numpy()])
  return x, len(Es), accepts, Es


def _compare_with_by_hand(run_product, score64, score32, x0, kind, params, rtol, atol, seed, what, post=lambda v: v):
  """The precondition on the two by-hand loops, then the product against them.  run_product() -> (x, iterations, accept rows)."""
  x64, it64, acc64, E64 = _by_hand(score64, x0, kind, params, torch.float64, rtol, atol, seed)
  x32, it32, acc32, _ = _by_hand(score32, x0, kind, params, torch.float32, rtol, atol, seed)
  gap = min(float(np.abs(e - 1.).min()) for e in E64 if e.size)
  rejected = sum(1 for row in acc64 for a in row if not a)
  print(f'{what}: {it64} iterations, {rejected} rejected or idle sample-steps, closest float64 E to 1: {gap:.2e}')
  assert acc64 == acc32 and it64 == it32, f'{what}: the float64 and fp32 by-hand loops decide differently: choose another seed'
  assert gap >= 1e-3, f'{what}: a float64 E lies {gap:.1e} from 1: choose another seed'
  got, iterations, accepts = run_product()
  assert iterations == it64 and accepts == acc64, f'{what}: the product decides differently from the by-hand loops'
  ref = post(x64).cpu().numpy()
  own, err = R.rel(post(x32).double().cpu().numpy(), ref), R.rel(got.double().cpu().numpy(), ref)
  print(f'{what}: the product deviates {err:.2e} from the float64 loop; the by-hand fp32 loop deviates {own:.2e}: tolerance {4 * own:.2e}')
  assert err <= 4 * own
  return iterations


# the seeds were chosen from the by-hand loops alone (seeds 1..8 tried on an MI355X: all take the same decisions in float64 and
# fp32; the closest float64 E to 1 is 7.8e-3 for VP seed 7 and 4.0e-3 for VE seed 3, below 1e-3 for six of the VE seeds)
LOOP = {'vp': dict(params=(0.1, 20.), seed=7), 've': dict(params=(0.01, 50.), seed=3)}
MU, S0 = 0.3, 0.5


def _gaussian_score(kind, params, dtype):
  def score(x, t):
    t = t.to(dtype)
    if kind == 'vp':
      la = -0.25 * t ** 2 * (params[1] - params[0]) - 0.5 * t * params[0]
      a, var = torch.exp(la), 1. - torch.exp(2. * la)
    else:
      a, var = torch.ones_like(t), (params[0] * (params[1] / params[0]) ** t) ** 2
    bc = lambda v: v.reshape((-1,) + (1,) * (x.dim() - 1))
    return -(x.to(dtype) - bc(a) * MU) / bc(a * a * S0 * S0 + var)
  return score


@pytest.mark.parametrize('family', ['vp', 've'])
def test_loop_with_a_closed_form_score(st, hip_lib, family):
  ada, S = st.adaptive_sde, st.sde_lib
  dev = torch.device('cuda:0')
  params, seed = LOOP[family]['params'], LOOP[family]['seed']
  sde = S.VPSDE(beta_min=0.1, beta_max=20) if family == 'vp' else S.VESDE(sigma_min=0.01, sigma_max=50)
  g = torch.Generator().manual_seed(11)
  x0 = (torch.randn(2, 3, 8, 8, generator=g) * (1. if family == 'vp' else 50.) + MU).to(dev)
  score32 = _gaussian_score(family, params, torch.float32)
  rtol, atol = 0.05, 0.0078

  def run_product():
    times = []

    def score_fn(x, t):
      assert t.shape == (2,) and t.dtype == torch.float32 and t.device == x.device
      times.append(t.clone())
      return score32(x, t)

    torch.manual_seed(seed)
    x = x0.clone()
    out, iterations, info = ada.adaptive_sample(score_fn, x, sde, rtol=rtol, atol=atol, eps=EPS)
    assert out is x and len(times) == 2 * iterations
    assert torch.equal(info['t'], torch.full((2,), EPS32, device=dev)), 'a sample did not end at eps exactly'
    starts = times[0::2] + [info['t']]
    accepts = [(starts[i + 1] != starts[i]).cpu().tolist() for i in range(iterations)]
    assert [sum(col) for col in zip(*accepts)] == info['accepted'].cpu().tolist()
    idle = [sum(1 for i in range(iterations) if float(starts[i][b]) == EPS32) for b in range(2)]
    assert [iterations - a - i for a, i in zip(info['accepted'].cpu().tolist(), idle)] == info['rejected'].cpu().tolist()
    return out, iterations, accepts

  _compare_with_by_hand(run_product, _gaussian_score(family, params, torch.float64), score32, x0, family, params, rtol, atol, seed,
                        f'closed-form score, {family}')


# ---- the sampler on the tiny networks -----------------------------------------------------------------------------------
# tolerances for a few dozen iterations on the random tiny networks (rtol 0.3 gives 8, rtol 1.0 gives 4)
SAMPLER = {f: dict(rtol=0.03, atol=0.0078, seed=3) for f in ('vp', 've', 'wide')}


def _setup(st, lib, family):
  return setup(st, lib, family, dict(method='adaptive', noise_removal=True, adaptive_rtol=SAMPLER[family]['rtol'],
                                     adaptive_atol=SAMPLER[family]['atol']))


def _sampler(st, cfg, sde, **options):
  return sampler(st, cfg, sde, EPS, **options)


@pytest.mark.parametrize('family', ['vp', 've'])
def test_sampler_matches_by_hand_loops(st, hip_lib, family):
  cfg, sde, model = _setup(st, hip_lib, family)
  opt = SAMPLER[family]
  seed = opt['seed']
  kind, params = ('ve', (sde.sigma_min, sde.sigma_max)) if isinstance(sde, st.sde_lib.VESDE) else ('vp', (sde.beta_0, sde.beta_1))
  net = st.models.utils.get_score_fn(cfg, sde, model, train=False, continuous=cfg.training.continuous)
  torch.manual_seed(seed)
  x0 = sde.prior_sampling(_shape(cfg)).to(cfg.device)
  state = (torch.get_rng_state(), torch.cuda.get_rng_state())

  def run_product():
    """The sampler without denoising returns inverse_scaler(state); the accept rows come from the times the network saw."""
    times = []

    def spy(x, t):
      times.append(t.clone())
      return net(x, t)

    with pytest.MonkeyPatch.context() as mp:
      mp.setattr(st.models.utils, 'get_score_fn', lambda *a, **k: spy)
      torch.manual_seed(seed)
      got, nfe = _sampler(st, cfg, sde, noise_removal=False)(model)
    n = len(times) // 2
    assert nfe == 2 * n == len(times)
    starts = times[0::2] + [torch.full_like(times[0], EPS32)]
    return got, n, [(starts[i + 1] != starts[i]).cpu().tolist() for i in range(n)]

  inv = st.datasets.get_data_inverse_scaler(cfg)

  def by_hand_score(dtype):
    return lambda x, t: net(x.float(), t.float()).to(dtype)

  with torch.no_grad():
    # the by-hand loops restart from the generator states the prior draw left, as the product's loop does
    n = _compare_with_by_hand(run_product, by_hand_score(torch.float64), by_hand_score(torch.float32), x0, kind, params,
                              opt['rtol'], opt['atol'], state, f'tiny network, {family}', post=inv)
  assert 8 <= n <= 200, f'{n} iterations: choose tolerances that give a few dozen'
  # with denoising: one more evaluation; two runs under one seed are bit-identical
  torch.manual_seed(seed)
  a, nfe = _sampler(st, cfg, sde)(model)
  assert nfe == 2 * n + 1 and a.shape == _shape(cfg) and a.dtype == torch.float32 and bool(torch.isfinite(a).all())
  torch.manual_seed(seed)
  b, _ = _sampler(st, cfg, sde)(model)
  assert torch.equal(a, b), 'two runs under one seed differ'
  # the generators after a run without the denoising step (which draws once more, as in get_pc_sampler): the prior draw plus
  # one randn_like of the state per iteration, nothing else
  torch.manual_seed(seed)
  _, nfe = _sampler(st, cfg, sde, noise_removal=False)(model)
  assert nfe == 2 * n
  after_run = (torch.get_rng_state(), torch.cuda.get_rng_state())
  torch.manual_seed(seed)
  x = sde.prior_sampling(_shape(cfg)).to(cfg.device)
  for _ in range(n):
    torch.randn_like(x)
  assert torch.equal(after_run[0], torch.get_rng_state()) and torch.equal(after_run[1], torch.cuda.get_rng_state())
  torch.randn_like(x)
  assert not torch.equal(after_run[1], torch.cuda.get_rng_state()), 'randn_like does not move the generator'
  with pytest.raises(RuntimeError, match='max_iters = 1'):
    torch.manual_seed(seed)
    st.adaptive_sde.get_adaptive_sampler(cfg, sde, _shape(cfg), inv, rtol=opt['rtol'], atol=opt['atol'], eps=EPS, device=cfg.device,
                                         max_iters=1)(model)


@pytest.mark.parametrize('family', ['vp', 've', 'wide'])
def test_fp16_runs(st, hip_lib, family):
  """precision = 'fp16' (the network only): runs and is finite; on the wide network, whose layers take the fp16 forms, the
  result differs from fp32.  No threshold on the difference: sample quality in that mode is unmeasured."""
  cfg, sde, model = _setup(st, hip_lib, family)
  outs = {}
  for precision in ('fp32', 'fp16'):
    torch.manual_seed(9)
    outs[precision], nfe = _sampler(st, cfg, sde, precision=precision)(model)
    assert nfe % 2 == 1 and bool(torch.isfinite(outs[precision]).all())
  diff = float((outs['fp16'] - outs['fp32']).abs().max())
  print(f'{family}: fp16 against fp32: max |difference| {diff:.3e}')
  if family == 'wide':
    assert diff > 0, 'the fp16 mode did not reach the network'
