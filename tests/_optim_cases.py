"""Optimizer-side kernels of csrc/reduce_optim.hip (sumsq -> clip + Adam / amsgrad -> EMA) against the float64 reference and
the per-element bounds of tests/_optim_ref.py.  tests/test_optim_cases_cpu.py runs every case on the plain-C checker (which
proves, without a GPU, that an fp32 implementation of the step stays inside the bounds), tests/test_gpu_optim.py on the HIP
library.

Host dispatch restated (`branch`, asserted per case against the label in the table):
  stk_adam_f32          p, g, m, v all 16-byte aligned -> adam_kernel: float4 body over n / 4 ("vec"), scalar tail over
                        n % 4 ("tail");  any of the four misaligned -> adam_kernel_scalar
  stk_adam_amsgrad_f32  adam_amsgrad_kernel, one scalar loop whatever the alignment
  stk_ema_f32           shadow and p aligned -> ema_kernel vec (+ tail), else ema_kernel scalar
  stk_sumsq_f32         nb = min(ceil(n / 4096), 1024) workgroups ("cap": the 1024 limit cut the grid) of sumsq_stage1, which
                        takes float4s (+ tail) when x is aligned and single floats otherwise; then sumsq_stage2

Case table (name: what it is for -> branch).  Sizes, all aligned, each of adam (plain, clip on at 3 x max_norm), amsgrad,
ema and sumsq:
  n = 1, 3                  -> :tail                  nb=1
  n = 4                     -> :vec                   nb=1
  n = 5, 1023               -> :vec+tail              nb=1
  n = 4099                  -> :vec+tail              nb=2
  n = 1 << 20               -> :vec                   nb=256
  n = 1024 * 4096 - 1       -> :vec+tail              nb=1024      (the last uncapped grid)
  n = 1024 * 4096 + 5       -> :vec+tail              nb=1024cap   (1025 wanted)
  n = (1 << 22) + 3         -> :vec+tail              nb=1024cap
Misaligned views (n = 4099, one tensor on a buf[1:] view, 4 bytes past a 16-byte boundary):
  adam_mis_p / _g / _m / _v         -> adam_kernel_scalar
  amsgrad_mis_vmax                  -> adam_amsgrad_kernel
  ema_mis_s / ema_mis_p             -> ema_kernel:scalar
  sumsq_mis_x, sumsq_mis_x_cap      -> sumsq_stage1:scalar  nb=2 / nb=1024cap (the longest chain: 17 per thread)
Adam variants (n = 4099): plain, L2 weight decay, AdamW, and each on amsgrad, whose vmax is above v in half the elements.
Clipping (n = 4099): sumsq NULL; max_norm < 0 with a sumsq given; norm < max_norm (coef == 1: g bit-equal); norm = 3 x
  max_norm; max_norm = 0 (g becomes 0).
Steps: step 1 (bc1 = 0.1, bc2 = 1e-3, m = v = 0) and step 10^6 (both corrections are 1 in fp32), adam and amsgrad.
Gradient range: |g| = 10^U(-12, 2) within one tensor; g = 0 with m = v = 0, without weight decay (p bit-identical), with L2
  and with AdamW.
Non-finite gradients: one NaN in g; with clipping every p is NaN afterwards, without it only that element
  (`nonfinite`, all three kernels).
Trajectory: 50 steps, n = 4096, lr = 2e-4 * min(step / warmup, 1) as optimize_fn sets it (warmup = 25, so that the ramp
  and the plateau both lie inside the 50 steps), clipping on with the norm below max_norm; at every step one float64
  step from the library's own state (`trajectory`), then the drift of the whole run against a pure float64 trajectory.
"""
import numpy as np
import torch

import _optim_ref as R
from _util import call, dev_of

U = R.U
SIZES = [1, 3, 4, 5, 1023, 4099, 1 << 20, 1024 * 4096 - 1, 1024 * 4096 + 5, (1 << 22) + 3]
_SIZE_FORM = {1: 'tail', 3: 'tail', 4: 'vec', 5: 'vec+tail', 1023: 'vec+tail', 4099: 'vec+tail', 1 << 20: 'vec',
              1024 * 4096 - 1: 'vec+tail', 1024 * 4096 + 5: 'vec+tail', (1 << 22) + 3: 'vec+tail'}
_SIZE_NB = {1: '1', 3: '1', 4: '1', 5: '1', 1023: '1', 4099: '2', 1 << 20: '256', 1024 * 4096 - 1: '1024',
            1024 * 4096 + 5: '1024cap', (1 << 22) + 3: '1024cap'}


def _case(name, op, n, label, mis=None, variant='plain', clip='null', step=3, grad='normal', omd=1 - 0.9999):
  return dict(name=name, op=op, n=n, label=label, mis=mis, variant=variant, clip=clip, step=step, grad=grad, omd=omd)


CASES = []
for _n in SIZES:
  _f, _nb = _SIZE_FORM[_n], _SIZE_NB[_n]
  CASES += [
    _case(f'adam_n{_n}', 'adam', _n, f'adam_kernel:{_f}', clip='above3'),
    _case(f'amsgrad_n{_n}', 'amsgrad', _n, 'adam_amsgrad_kernel', clip='above3'),
    _case(f'ema_n{_n}', 'ema', _n, f'ema_kernel:{_f}'),
    _case(f'sumsq_n{_n}', 'sumsq', _n, f'sumsq_stage1:{_f} nb={_nb}'),
  ]
M = 4099
CASES += [
  _case('adam_mis_p', 'adam', M, 'adam_kernel_scalar', mis='p', clip='above3'),
  _case('adam_mis_g', 'adam', M, 'adam_kernel_scalar', mis='g', clip='above3', variant='l2'),
  _case('adam_mis_m', 'adam', M, 'adam_kernel_scalar', mis='m', clip='below', variant='adamw'),
  _case('adam_mis_v', 'adam', M, 'adam_kernel_scalar', mis='v'),
  _case('adam_mis_g_n5', 'adam', 5, 'adam_kernel_scalar', mis='g', clip='above3'),
  _case('amsgrad_mis_vmax', 'amsgrad', M, 'adam_amsgrad_kernel', mis='vmax', clip='above3'),
  _case('ema_mis_s', 'ema', M, 'ema_kernel:scalar', mis='s'),
  _case('ema_mis_p', 'ema', M, 'ema_kernel:scalar', mis='p', omd=1 - 0.999),
  _case('sumsq_mis_x', 'sumsq', M, 'sumsq_stage1:scalar nb=2', mis='x'),
  _case('sumsq_mis_x_cap', 'sumsq', (1 << 22) + 3, 'sumsq_stage1:scalar nb=1024cap', mis='x'),
]
for _op, _lab in (('adam', 'adam_kernel:vec+tail'), ('amsgrad', 'adam_amsgrad_kernel')):
  CASES += [
    _case(f'{_op}_plain', _op, M, _lab),
    _case(f'{_op}_l2', _op, M, _lab, variant='l2'),
    _case(f'{_op}_adamw', _op, M, _lab, variant='adamw'),
    _case(f'{_op}_step1', _op, M, _lab, step=1, clip='above3'),
    _case(f'{_op}_step1e6', _op, M, _lab, step=10 ** 6, clip='above3'),
  ]
CASES += [
  _case('clip_null', 'adam', M, 'adam_kernel:vec+tail', clip='null', variant='l2'),
  _case('clip_negative', 'adam', M, 'adam_kernel:vec+tail', clip='neg'),
  _case('clip_below', 'adam', M, 'adam_kernel:vec+tail', clip='below'),
  _case('clip_above3', 'adam', M, 'adam_kernel:vec+tail', clip='above3', variant='adamw'),
  _case('clip_zero', 'adam', M, 'adam_kernel:vec+tail', clip='zero'),
  _case('clip_below_scalar', 'adam', M, 'adam_kernel_scalar', clip='below', mis='p'),
  _case('clip_below_amsgrad', 'amsgrad', M, 'adam_amsgrad_kernel', clip='below'),
  _case('clip_zero_amsgrad', 'amsgrad', M, 'adam_amsgrad_kernel', clip='zero'),
  _case('range', 'adam', M, 'adam_kernel:vec+tail', grad='range'),
  _case('range_step1', 'adam', M, 'adam_kernel:vec+tail', grad='range', step=1),
  _case('range_amsgrad', 'amsgrad', M, 'adam_amsgrad_kernel', grad='range'),
  _case('range_scalar', 'adam', M, 'adam_kernel_scalar', grad='range', mis='v'),
  _case('zero_grad', 'adam', M, 'adam_kernel:vec+tail', grad='zero', step=1),
  _case('zero_grad_l2', 'adam', M, 'adam_kernel:vec+tail', grad='zero', step=1, variant='l2'),
  _case('zero_grad_adamw', 'adam', M, 'adam_kernel:vec+tail', grad='zero', step=1, variant='adamw'),
  _case('zero_grad_amsgrad', 'amsgrad', M, 'adam_amsgrad_kernel', grad='zero', step=1),
  _case('zero_grad_scalar', 'adam', M, 'adam_kernel_scalar', grad='zero', step=1, mis='m'),
]
CASE_IDS = [c['name'] for c in CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)

# every form of every optimizer-side __global__ kernel of csrc/reduce_optim.hip (sumsq_stage2 runs behind every stage 1)
ALL_BRANCHES = {
  'adam_kernel:vec', 'adam_kernel:tail', 'adam_kernel:vec+tail', 'adam_kernel_scalar', 'adam_amsgrad_kernel',
  'ema_kernel:vec', 'ema_kernel:tail', 'ema_kernel:vec+tail', 'ema_kernel:scalar',
  'sumsq_stage1:vec', 'sumsq_stage1:tail', 'sumsq_stage1:vec+tail', 'sumsq_stage1:scalar',
}
ALL_GRIDS = {'nb=1', 'nb=2', 'nb=256', 'nb=1024', 'nb=1024cap'}

VARIANTS = {'plain': dict(), 'l2': dict(wd=0.01), 'adamw': dict(wd=0.01, adamw=True, lr=1e-3, b2=0.99)}


def _form(n):
  return '+'.join(f for f, on in (('vec', n >= 4), ('tail', n % 4)) if on)


def branch(case, tensors):
  """The kernel form the host wrapper takes, from n and the addresses actually passed (module text)."""
  n, op = case['n'], case['op']
  al = {k: t.data_ptr() % 16 == 0 for k, t in tensors.items()}
  if op == 'adam':
    return f'adam_kernel:{_form(n)}' if all(al[k] for k in 'pgmv') else 'adam_kernel_scalar'
  if op == 'amsgrad':
    return 'adam_amsgrad_kernel'
  if op == 'ema':
    return f'ema_kernel:{_form(n)}' if al['s'] and al['p'] else 'ema_kernel:scalar'
  want = -(-n // 4096)
  nb = f"nb={min(want, 1024)}{'cap' if want > 1024 else ''}"
  return f"sumsq_stage1:{_form(n) if al['x'] else 'scalar'} {nb}"


def place(t, d, misaligned):
  """A copy of the CPU tensor `t` on device `d`; misaligned: a buf[1:] view, 4 bytes past a 16-byte boundary."""
  if not misaligned:
    out = t.to(d).contiguous().clone()
    assert out.data_ptr() % 16 == 0
    return out
  buf = torch.empty(t.numel() + 1, device=d)
  assert buf.data_ptr() % 16 == 0
  buf[1:] = t.to(d)
  v = buf[1:]
  assert v.data_ptr() % 16 == 4 and v.is_contiguous()
  return v


def _gen(seed):
  return torch.Generator().manual_seed(seed)


def inputs(case):
  """CPU fp32 tensors of one case: p ~ N(0,1); g, m ~ 0.01 N(0,1); v ~ (0.01 N(0,1))^2."""
  n, gen = case['n'], _gen(4000 + len(case['name']) + case['n'] % 977)
  rn = lambda s: torch.randn(n, generator=gen) * s
  t = {'p': rn(1.0), 'g': rn(0.01), 'm': rn(0.01), 'v': rn(0.01) ** 2, 's': rn(1.0)}
  if case['grad'] == 'range':
    e = torch.rand(n, generator=gen) * 14 - 12
    t['g'] = torch.sign(t['g']) * 10.0 ** e
    t['g'][0], t['g'][-1] = 1e-12, -1e2
  if case['grad'] == 'zero':
    t['g'] = torch.zeros(n)
  if case['step'] == 1 or case['grad'] == 'zero':
    t['m'], t['v'] = torch.zeros(n), torch.zeros(n)
  if case['op'] == 'amsgrad':
    even = torch.arange(n) % 2 == 0
    t['vmax'] = torch.where(even, 4 * t['v'] + 1e-6, 0.25 * t['v'])
    if case['step'] == 1 or case['grad'] == 'zero':
      t['vmax'] = torch.where(even, torch.full((n,), 1e-6), torch.zeros(n))
  return t


def hyper(case, norm):
  kw = dict(VARIANTS[case['variant']])
  max_norm = {'null': None, 'neg': -1.0, 'below': 10.0 * norm + 1.0, 'above3': norm / 3.0, 'zero': 0.0}[case['clip']]
  return R.Hyper(t=case['step'], max_norm=max_norm, **kw)


def _np(t):
  return t.detach().cpu().numpy().astype(np.float64)


def _ratio(err, bound):
  """max of err / bound, where 0 / 0 counts as 0 and any non-finite error as inf."""
  err, bound = np.atleast_1d(np.asarray(err, np.float64)), np.atleast_1d(np.asarray(bound, np.float64))
  bound = np.broadcast_to(bound, err.shape)
  r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300))
  r = np.where(np.isfinite(err), r, np.inf)
  return float(r.max()) if r.size else 0.0


def check_sumsq(lib, x_dev, x_cpu, n, ss=None, ws=None):
  """Run stk_sumsq_f32 and return (the device scalar, figure)."""
  d = x_dev.device
  ss = torch.full((1,), float('nan'), device=d) if ss is None else ss
  ws = torch.full((2048,), float('nan'), device=d) if ws is None else ws
  call(lib, 'sumsq_f32', x_dev, n, ss, ws)
  ref = R.sumsq_ref(_np(x_cpu))
  got = float(ss.cpu()[0])
  vec = x_dev.data_ptr() % 16 == 0
  rel = abs(got - ref) / ref if ref > 0 else abs(got)
  return ss, _ratio(rel, R.sumsq_bound(n, vec))


def adam_call(lib, op, t, n, h, ss):
  args = [t['p'], t['g'], t['m'], t['v']] + ([t['vmax']] if op == 'amsgrad' else [])
  use_ss = h.max_norm is not None
  call(lib, 'adam_amsgrad_f32' if op == 'amsgrad' else 'adam_f32', *args, n, *h.abi_tail(),
       ss if use_ss else None, h.max_norm if use_ss else -1.0)


def step_figures(old, new, h, ss_value, op):
  """Figures (worst error / bound per quantity) of one library step old -> new (dicts of CPU fp32 tensors), ss_value the
  sum of squares the library was given (None: clipping off).  The float64 step starts from the library's clipped g."""
  fig = {}
  g_in, g_out = _np(old['g']), _np(new['g'])
  clipping = ss_value is not None and h.max_norm is not None and h.max_norm >= 0
  coef = R.clip_coef(ss_value, h.max_norm) if clipping else 1.0
  if coef == 1.0:
    same = torch.equal(old['g'].view(torch.int32), new['g'].view(torch.int32))
    fig['g_bit_equal'] = 0.0 if same else float('inf')
  else:
    g_ref = g_in * coef
    fig['g'] = _ratio(np.abs(g_out - g_ref), R.clip_bound(g_ref))
  ref = R.adam_step(_np(old['p']), g_out, _np(old['m']), _np(old['v']), h,
                    vmax=_np(old['vmax']) if op == 'amsgrad' else None)
  b = R.adam_bounds(_np(old['p']), g_out, _np(old['m']), h, ref)
  for k in ('m', 'v') + (('vmax',) if op == 'amsgrad' else ()):
    fig[k] = _ratio(np.abs(_np(new[k]) - ref[k]), b[k])
  dp = _np(new['p']) - _np(old['p'])
  fig['dp'] = _ratio(np.abs(dp - ref['dp']), b['dp'])
  return fig, ref


def run_case(lib, case):
  """Run one case on `lib`; returns (figures, the branch reached)."""
  d = dev_of(lib)
  n, op, mis = case['n'], case['op'], case['mis']
  cpu = inputs(case)
  if op == 'sumsq':
    x = place(cpu['g'], d, mis == 'x')
    reached = branch(case, {'x': x})
    _, f = check_sumsq(lib, x, cpu['g'], n)
    return {'sumsq': f}, reached
  if op == 'ema':
    s, p = place(cpu['s'], d, mis == 's'), place(cpu['p'], d, mis == 'p')
    reached = branch(case, {'s': s, 'p': p})
    call(lib, 'ema_f32', s, p, n, case['omd'])
    ref = R.ema_step(_np(cpu['s']), _np(cpu['p']), case['omd'])
    fig = {'ema': _ratio(np.abs(_np(s) - ref), R.ema_bound(cpu['s'].numpy(), cpu['p'].numpy())),
           'p_untouched': 0.0 if torch.equal(p.cpu(), cpu['p']) else float('inf')}
    return fig, reached
  names = ['p', 'g', 'm', 'v'] + (['vmax'] if op == 'amsgrad' else [])
  t = {k: place(cpu[k], d, mis == k) for k in names}
  reached = branch(case, t)
  norm = float(np.sqrt(R.sumsq_ref(_np(cpu['g']))))
  h = hyper(case, norm)
  fig, ss, ss_value = {}, None, None
  if h.max_norm is not None:
    ss, fig['sumsq'] = check_sumsq(lib, t['g'], cpu['g'], n)
    ss_value = float(ss.cpu()[0])
  adam_call(lib, op, t, n, h, ss)
  new = {k: t[k].cpu() for k in names}
  f, ref = step_figures(cpu, new, h, ss_value, op)
  fig.update(f)
  if case['clip'] == 'below':
    assert 'g_bit_equal' in fig, 'norm < max_norm must leave the coefficient at exactly 1'
  if case['clip'] in ('above3', 'zero') and norm > 0:
    assert 'g' in fig, 'the case must clip'
  if case['clip'] == 'zero':
    fig['g_is_zero'] = 0.0 if float(new['g'].abs().max()) == 0.0 else float('inf')
  if op == 'amsgrad' and n >= 64:
    frac = float((ref['vmax'] > ref['v']).mean())
    assert 0.4 < frac < 0.6, f'vmax must be above v in half the elements, is in {frac:.2f}'
  if case['grad'] == 'zero' and case['variant'] == 'plain':
    fig['p_bit_identical'] = 0.0 if torch.equal(new['p'].view(torch.int32), cpu['p'].view(torch.int32)) else float('inf')
  if case['grad'] == 'zero' and case['variant'] != 'plain':
    assert float((new['p'] - cpu['p']).abs().max()) > 0, 'weight decay must move the parameter'
  return fig, reached


def report(fig, what):
  """Print every figure, return the misses."""
  bad = []
  for k, r in fig.items():
    print(f'  {what} {k}: worst error / bound = {r:.3g}')
    if not r <= 1.0:
      bad.append((k, r))
  return bad


# ---- non-finite gradients ---------------------------------------------------------------------------------------------
def nonfinite(lib, op, mis=None):
  """One NaN in g.  clip_grad_norm_ multiplies every gradient by clamp(max_norm / (norm + 1e-6), max=1.0), and clamp keeps a
  NaN: under clipping every gradient, and with it every parameter, is NaN afterwards.  Without clipping only the element
  with the NaN is, as in torch.optim.Adam."""
  d = dev_of(lib)
  n, at = 4099, 1234
  case = _case('nonfinite', op, n, None)
  cpu = inputs(case)
  cpu['g'][at] = float('nan')
  names = ['p', 'g', 'm', 'v'] + (['vmax'] if op == 'amsgrad' else [])
  out = {}
  for clip in (True, False):
    t = {k: place(cpu[k], d, mis == k) for k in names}
    h = R.Hyper(t=3, max_norm=1.0 if clip else None)
    ss = None
    if clip:
      ss = torch.zeros(1, device=d)
      call(lib, 'sumsq_f32', t['g'], n, ss, torch.zeros(2048, device=d))
      assert bool(torch.isnan(ss.cpu()[0])), 'the sum of squares of a gradient with a NaN is NaN'
    adam_call(lib, op, t, n, h, ss)
    out[clip] = {k: torch.isnan(t[k].cpu()) for k in names}
  for k in names:
    assert bool(out[True][k].all()), f'{op}: clipping with a NaN norm must make every {k} NaN, as clip_grad_norm_ does'
    only = torch.zeros(n, dtype=torch.bool)
    only[at] = True
    assert torch.equal(out[False][k], only), f'{op}: without clipping only element {at} of {k} may be NaN'


# ---- trajectory ---------------------------------------------------------------------------------------------------------
T_STEPS, T_N, T_LR, T_WARMUP, T_CLIP = 50, 4096, 2e-4, 25, 1.0


def _traj_grads():
  gen = _gen(77)
  return [torch.randn(T_N, generator=gen) * 0.01 for _ in range(T_STEPS)]


def _traj_lr(step):
  return T_LR * float(np.minimum(step / T_WARMUP, 1.0))        # losses.py optimize_fn, step = 0, 1, ...


def trajectory(lib):
  """50 library steps.  At every step: one float64 step from the library's state, checked with the one-step bounds.
  Returns (worst figures over the steps, p_0, p_T, v_T) as CPU tensors."""
  d = dev_of(lib)
  p0 = torch.randn(T_N, generator=_gen(78))
  t = {'p': place(p0, d, False), 'm': torch.zeros(T_N, device=d), 'v': torch.zeros(T_N, device=d)}
  ss, ws = torch.zeros(1, device=d), torch.zeros(2048, device=d)
  worst = {}
  for i, g in enumerate(_traj_grads()):
    h = R.Hyper(lr=_traj_lr(i), t=i + 1, max_norm=T_CLIP)
    old = {k: t[k].cpu().clone() for k in 'pmv'}
    old['g'] = g
    t['g'] = place(g, d, False)
    _, f_ss = check_sumsq(lib, t['g'], g, T_N, ss, ws)
    adam_call(lib, 'adam', t, T_N, h, ss)
    new = {k: t[k].cpu() for k in 'pgmv'}
    fig, _ = step_figures(old, new, h, float(ss.cpu()[0]), 'adam')
    fig['sumsq'] = f_ss
    for k, r in fig.items():
      worst[k] = max(worst.get(k, 0.0), r) if r == r else float('inf')
  return worst, p0, t['p'].cpu(), t['v'].cpu()


def trajectory_f64():
  """The same 50 steps in float64 throughout (scalars rounded as the ABI rounds them): (p_T - p_0, v_T)."""
  p = _np(torch.randn(T_N, generator=_gen(78)))
  p0, m, v = p.copy(), np.zeros(T_N), np.zeros(T_N)
  for i, g in enumerate(_traj_grads()):
    h = R.Hyper(lr=_traj_lr(i), t=i + 1, max_norm=T_CLIP)
    g = _np(g)
    g = g * R.clip_coef(R.sumsq_ref(g), T_CLIP)
    r = R.adam_step(p, g, m, v, h)
    p, m, v = r['p'], r['m'], r['v']
  return p - p0, v


def trajectory_torch_fp32():
  """torch.optim.Adam + clip_grad_norm_ in fp32 on the CPU on the same inputs: p_T - p_0 (the independent fp32 baseline)."""
  p0 = torch.randn(T_N, generator=_gen(78))
  p = torch.nn.Parameter(p0.clone())
  opt = torch.optim.Adam([p], lr=T_LR, betas=(0.9, 0.999), eps=1e-8)
  for i, g in enumerate(_traj_grads()):
    for grp in opt.param_groups:
      grp['lr'] = _traj_lr(i)
    p.grad = g.clone()
    torch.nn.utils.clip_grad_norm_([p], max_norm=T_CLIP)
    opt.step()
  return _np(p.detach()) - _np(p0)


def drift(p0, pT, vT):
  """(displacement error of the library, of torch fp32, signed mean relative error of v), all against float64."""
  dp64, v64 = trajectory_f64()
  scale = np.abs(dp64).max()
  e_lib = np.abs((_np(pT) - _np(p0)) - dp64).max() / scale
  e_torch = np.abs(trajectory_torch_fp32() - dp64).max() / scale
  v_bias = float(np.mean((_np(vT) - v64) / v64))
  return e_lib, e_torch, v_bias
