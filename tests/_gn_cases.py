"""Ill-conditioned GroupNorm inputs, a float64 reference and per-group metrics (tests/test_gpu_groupnorm_conditioning.py on
the HIP library, tests/test_groupnorm_conditioning_cpu.py on the plain-C checker).

Why per group: the output of a normalisation has scale ~1 in every (sample, group) whatever the input, so one badly
normalised group must be judged against ITS OWN result, not against the largest value of the tensor.

Inputs.  Every (sample, group) of one tensor is filled by one VARIANT, so that the groups of one launch are hard in
different ways.  Families (the number the tests are parametrised by):
  1  leading outlier: x[first element of the group] = A, the rest randn or zeros; |A| = 1e2 .. 1e4, both signs.  With two
     sources the groups that begin in x2 and the groups that straddle x1 / x2 get such variants too (`_rotation`).
  2  the same outlier elsewhere (middle, last, first element of the second channel, first element of the second 4096-float
     chunk): the control that shows family 1 is about position, not magnitude.
  3  offset: mean / std = 1, 10, OFFSET_MAX and -OFFSET_MAX, first element typical.
  4  constant groups (var = 0, rstd = eps^-1/2) and nearly constant ones (std^2 << eps).
  5  scales far apart (a tensor of its own, `kind='scales'`): group g is randn * 10^k(g), k over 6.5 decades, and the second
     source is 1e4 times the first, so straddling groups mix both.

Condition (c) of the inputs (asserted in the CPU half for every case): a plain fp32 two-pass GroupNorm (torch float32 on the
CPU: mean, then mean of (x - mean)^2) stays within HALF the tolerance against float64.  That fixes the constants:
  * OFFSET_MAX = 50.  The mean alone carries half an ulp, 2^-24 * (mean / std) sigma, and its summation a little more:
    the fp32 two-pass measures 3.6e-6 .. 5.4e-6 at 50 and 1.1e-5 .. 1.3e-5 > TOL / 2 at 100 (two of the shapes below), so
    50 is the ratio used; the 1e4 of raw-moment folklore would ask 6e-4 of fp32.
  * constant groups hold 3.0, -0.75 and 0: L copies of them sum exactly in fp32 for every L here (L * 3 < 2^24), so an fp32
    mean is exact and xhat = 0; a constant with a full mantissa is off by an ulp of the mean times rstd = 1000.
  * nearly constant groups are 2^-6 + 1e-4 randn and 1e-5 randn: var <= 1e-8 << eps = 1e-6, and half an ulp of the mean,
    9e-10, times rstd ~ 1000 is 1e-6.

Tolerance: TOL = 2e-5, the bar tests/test_gpu_kernels.py::test_groupnorm holds GroupNorm to, applied per group:
  mean   |mean - mean64| * rstd64                        (error of the mean in standard deviations)
  rstd   |rstd / rstd64 - 1|
  y, dx  max over the group of |got - f64| / max over the group of |f64|   (dx1 and dx2 of a straddling group together)
  dgamma, dbeta   per channel, |got - f64| / sum of |terms| of that channel (their condition): sum |du| for dbeta and
                  sum |du xhat| + sum |du| for dgamma, whose xhat carries the absolute error of the mean (in sigmas) too
For dx the bound is TOL * cond(group): dx = rstd (du g - m1 - xhat m2) is a sum of three terms that cancel at a spike
(xhat ~ sqrt(L)), so fp32 evaluates it to eps * rstd (|du g| + |m1| + |xhat m2|), not to eps |dx|.  cond(group) = the maximum
of that sum of absolute terms over the group / the maximum of |dx| over the group, both from the float64 reference; >= 1.
"""
import numpy as np
import torch
import torch.nn.functional as F

from _util import call, dev_of

EPS = 1e-6
TOL = 2e-5
OFFSET_MAX = 50.0
FAMILIES = (1, 2, 3, 4, 5)

# (family, tag, kind, A / ratio / constant, rest)
VARIANTS = [
  (1, 'lead+1e2 randn', 'spike', 1e2, 'randn'), (1, 'lead-1e3 randn', 'spike', -1e3, 'randn'),
  (1, 'lead+1e4 randn', 'spike', 1e4, 'randn'), (1, 'lead-1e4 randn', 'spike', -1e4, 'randn'),
  (1, 'lead-1e2 zeros', 'spike', -1e2, 'zeros'), (1, 'lead+1e3 zeros', 'spike', 1e3, 'zeros'),
  (1, 'lead+1e4 zeros', 'spike', 1e4, 'zeros'), (1, 'lead-1e4 zeros', 'spike', -1e4, 'zeros'),
  (2, 'middle+1e4 randn', 'spike', 1e4, 'randn'), (2, 'last-1e4 randn', 'spike', -1e4, 'randn'),
  (2, 'chan2+1e4 randn', 'spike', 1e4, 'randn'), (2, 'chunk2+1e4 zeros', 'spike', 1e4, 'zeros'),
  (2, 'last+1e3 zeros', 'spike', 1e3, 'zeros'),
  (3, 'offset 1', 'offset', 1.0, None), (3, 'offset 10', 'offset', 10.0, None),
  (3, 'offset +max', 'offset', OFFSET_MAX, None), (3, 'offset -max', 'offset', -OFFSET_MAX, None),
  (4, 'const 3', 'const', 3.0, None), (4, 'const -0.75', 'const', -0.75, None), (4, 'const 0', 'const', 0.0, None),
  (4, 'near 2^-6 + 1e-4', 'near', (2.0 ** -6, 1e-4), None), (4, 'near 0 + 1e-5', 'near', (0.0, 1e-5), None),
]
NV = len(VARIANTS)


def _spike_pos(tag, L, HW, cpg):
  where = tag.split('+')[0].split('-')[0]
  return {'lead': 0, 'middle': L // 2 + 1, 'last': L - 1, 'chan2': HW if cpg > 1 else 1,
          'chunk2': 4096 if L > 4096 else L // 4}[where]


def _fill(v, L, HW, cpg, gen):
  fam, tag, kind, a, rest = VARIANTS[v]
  r = torch.randn(L, generator=gen)
  if kind == 'spike':
    x = r if rest == 'randn' else torch.zeros(L)
    x[_spike_pos(tag, L, HW, cpg)] = a
    return x
  if kind == 'offset':
    return 0.5 * r + 0.5 * a                           # std 0.5, mean / std = a
  if kind == 'const':
    return torch.full((L,), a)
  return a[0] + a[1] * r


def _rotation(N, C1, C2, G, cpg):
  """Variant of group ng is (ng + rot) % NV; rot is chosen so that a group that straddles x1 / x2 (if the shape has one)
  and a group that begins in x2 (if there is an x2) are leading-outlier variants."""
  if not C2:
    return 0
  strad = [g for g in range(G) if g * cpg < C1 < (g + 1) * cpg]
  in2 = [g for g in range(G) if g * cpg >= C1]
  lead = lambda rot, gs: any(VARIANTS[(n * G + g + rot) % NV][0] == 1 for n in range(N) for g in gs)
  for rot in range(NV):
    if (not strad or lead(rot, strad)) and lead(rot, in2):
      return rot
  raise AssertionError('no rotation puts a leading outlier into a straddling group and into a group of x2')


class Inputs:
  pass


_INPUTS = {}


def inputs(N, C1, C2, HW, G, act, kind):
  """kind 'mixed': families 1-4 by (sample, group); kind 'scales': family 5.  Cached, with the float64 reference."""
  key = (N, C1, C2, HW, G, act, kind)
  if key in _INPUTS:
    return _INPUTS[key]
  C = C1 + C2
  cpg = C // G
  L = cpg * HW
  gen = torch.Generator().manual_seed(1000 + 7 * HW + C + (kind == 'scales'))
  x = torch.empty(N, G, L)
  fam = torch.zeros(N, G, dtype=torch.long)
  tags = {}
  if kind == 'mixed':
    assert N * G >= NV, 'every variant must appear'
    rot = _rotation(N, C1, C2, G, cpg)
    for n in range(N):
      for g in range(G):
        v = (n * G + g + rot) % NV
        x[n, g] = _fill(v, L, HW, cpg, gen)
        fam[n, g] = VARIANTS[v][0]
        tags[(n, g)] = VARIANTS[v][1]
    x = x.reshape(N, C, HW)
  else:
    k = torch.linspace(-3.25, 3.25, G)                 # 6.5 decades over the groups of one tensor
    for n in range(N):
      for g in range(G):
        kk = float(k[(g + 5 * n) % G])
        x[n, g] = (torch.randn(L, generator=gen) + 0.3) * 10.0 ** kk
        fam[n, g] = 5
        tags[(n, g)] = f'scale 1e{kk:+.1f}'
    x = x.reshape(N, C, HW)
    x[:, C1:] *= 1e4                                   # the second source: straddling groups mix s and 1e4 s
  inp = Inputs()
  inp.shape = (N, C1, C2, HW, G, act)
  inp.x1 = x[:, :C1].contiguous()
  inp.x2 = x[:, C1:].contiguous() if C2 else None
  inp.gamma = torch.randn(C, generator=gen) * 0.5 + 1.0
  inp.beta = torch.randn(C, generator=gen) * 0.2
  inp.dy = torch.randn(N, C, HW, generator=gen)
  inp.family, inp.tags = fam, tags
  inp.ref = reference(inp)
  _INPUTS[key] = inp
  return inp


def act_fn(act, u):
  """The activation by the `act` code of include/stk.h: 0 none, 1 SiLU, 2 ReLU, 3 LeakyReLU(0.2), 4 ELU."""
  if act == 1:
    return u * torch.sigmoid(u)
  if act == 2:
    return torch.clamp(u, min=0)
  if act == 3:
    return torch.where(u > 0, u, 0.2 * u)
  if act == 4:
    return torch.where(u > 0, u, torch.expm1(torch.clamp(u, max=0)))
  return u


def reference(inp):
  """float64, plain torch on the CPU: F.group_norm on the concatenated input, the activation by code, autograd for the
  gradients; plus the condition numbers the bounds need."""
  N, C1, C2, HW, G, act = inp.shape
  C = C1 + C2
  a1 = inp.x1.double().requires_grad_()
  leaves = [a1]
  if C2:
    a2 = inp.x2.double().requires_grad_()
    leaves.append(a2)
    x = torch.cat([a1, a2], 1)
  else:
    x = a1
  ga, be = inp.gamma.double().requires_grad_(), inp.beta.double().requires_grad_()
  u = F.group_norm(x, G, ga, be, EPS)
  u.retain_grad()
  y = act_fn(act, u)
  (y * inp.dy.double()).sum().backward()
  r = {'y': y.detach(), 'dgamma': ga.grad, 'dbeta': be.grad}
  r['dx'] = torch.cat([t.grad for t in leaves], 1)
  with torch.no_grad():
    xg = x.reshape(N, G, -1)
    mean = xg.mean(2)
    var = ((xg - mean[:, :, None]) ** 2).mean(2)
    rstd = (var + EPS).rsqrt()
    r['mean'], r['rstd'] = mean, rstd
    xhat = (xg - mean[:, :, None]) * rstd[:, :, None]
    du = u.grad.reshape(N, C, HW)                                  # dy * act'(u)
    dug = (du * ga.detach()[None, :, None]).reshape(N, G, -1)
    m1, m2 = dug.mean(2, keepdim=True), (dug * xhat).mean(2, keepdim=True)
    terms = rstd[:, :, None] * (dug.abs() + m1.abs() + (xhat * m2).abs())
    dxg = r['dx'].reshape(N, G, -1)
    assert torch.allclose(dxg, rstd[:, :, None] * (dug - m1 - xhat * m2), rtol=1e-9, atol=1e-12 * float(terms.max()))
    r['dx_cond'] = terms.amax(2) / dxg.abs().amax(2).clamp_min(1e-300)
    # (xhat itself is known to TOL absolute -- the mean metric -- and TOL relative -- the rstd metric)
    r['dgamma_abs'] = (du * xhat.reshape(N, C, HW)).abs().sum((0, 2)) + du.abs().sum((0, 2))
    r['dbeta_abs'] = du.abs().sum((0, 2))
  return r


def two_pass_fp32(inp):
  """Plain fp32 two-pass GroupNorm on the CPU (condition (c) of the inputs)."""
  N, C1, C2, HW, G, act = inp.shape
  C = C1 + C2
  x = torch.cat([inp.x1, inp.x2], 1) if C2 else inp.x1
  xg = x.reshape(N, G, -1)
  mean = xg.mean(2)
  d = xg - mean[:, :, None]
  rstd = 1.0 / torch.sqrt((d * d).mean(2) + torch.tensor(EPS))
  u = inp.gamma[None, :, None] * (d * rstd[:, :, None]).reshape(N, C, HW) + inp.beta[None, :, None]
  return {'mean': mean, 'rstd': rstd, 'y': act_fn(act, u)}


def group_errors(got, ref, G):
  """name -> [N, G] (mean, rstd, y, dx) or [C] (dgamma, dbeta): error in units of the bound's scale, see the module text."""
  e = {}
  N = ref['mean'].shape[0]
  if 'mean' in got:
    e['mean'] = (got['mean'].double().reshape(N, G) - ref['mean']).abs() * ref['rstd']
    e['rstd'] = (got['rstd'].double().reshape(N, G) / ref['rstd'] - 1).abs()
  for k in ('y', 'dx'):
    if k in got:
      a, b = got[k].double().reshape(N, G, -1), ref[k].reshape(N, G, -1)
      e[k] = (a - b).abs().amax(2) / b.abs().amax(2).clamp_min(1e-300)
      e[k][~torch.isfinite(a).all(2)] = float('inf')
  for k in ('dgamma', 'dbeta'):
    if k in got:
      e[k] = (got[k].double() - ref[k]).abs() / ref[k + '_abs'].clamp_min(1e-300)
      e[k][~torch.isfinite(got[k])] = float('inf')
  for k in ('mean', 'rstd'):
    if k in e:
      e[k][~torch.isfinite(e[k])] = float('inf')
  return e


def bounds(ref):
  """name -> bound of group_errors' figure ([N, G] for dx, a number otherwise)."""
  return {'mean': TOL, 'rstd': TOL, 'y': TOL, 'dx': TOL * ref['dx_cond'], 'dgamma': TOL, 'dbeta': TOL}


def decode_planes(pl, rec, N, C, HW):
  """(hi + lo) / s of a planes buffer [split][n][c / 32][pixel][c % 32] fp16 -> float64 [N, C, HW], and s."""
  m = float(rec.max())
  s = 2.0 ** (13 - int(np.floor(np.log2(m))))
  p = pl.cpu().numpy().view(np.float16).reshape(2, N, (C + 31) // 32, HW, 32)
  dec = (p[0].astype(np.float64) + p[1].astype(np.float64)) / s
  return torch.from_numpy(dec.transpose(0, 1, 3, 2).reshape(N, -1, HW)[:, :C].copy()), s


# ---- dispatch sites -------------------------------------------------------------------------------------------------
# name, entry, N, C1, C2, HW, G, act, options, the kernel(s) that must compute the statistics, the backward kernel
#   entry: 'fwd' stk_gn_fwd_f32, 'pl' stk_gn_fwd_pl_f32, 'pl_max' stk_gn_fwd_pl_max_f32
#   options: 'nows' (ws = NULL), 'off4' (x1 starts 4 bytes past a 16-byte boundary: no float4 loads)
SITES = [
  ('flat1', 'fwd', 2, 128, 0, 64, 32, 1, '', 'gn_fwd_flat_kernel<1>', 'flat'),                 # L = 256
  ('flat2_two_sources', 'fwd', 2, 128, 128, 64, 32, 1, '', 'gn_fwd_flat_kernel<2>', 'flat'),   # L = 512, groups 16.. in x2
  ('flat3_straddle', 'fwd', 2, 256, 128, 64, 32, 1, '', 'gn_fwd_flat_kernel<3>', 'flat'),      # L = 768, group 21 straddles
  ('flat4', 'fwd', 2, 128, 0, 1024, 32, 1, '', 'gn_fwd_flat_kernel<4>', 'flat'),               # L = 4096
  ('flat4_16384', 'fwd', 1, 128, 0, 4096, 32, 0, '', 'gn_fwd_flat_kernel<4>', 'flat'),         # L = 16384, no activation
  ('loop4', 'fwd', 3, 64, 0, 2304, 8, 1, '', 'gn_fwd_kernel<4>', 'loop'),                      # L = 18432, HW % 4096 != 0
  ('loop4_nows', 'fwd', 3, 32, 0, 8192, 8, 1, 'nows', 'gn_fwd_kernel<4>', 'split'),            # a split shape without ws
  ('loop1_straddle', 'fwd', 2, 30, 18, 25, 12, 1, '', 'gn_fwd_kernel<1>', 'loop'),             # HW % 4 != 0, group 7 straddles
  ('loop1_off4', 'fwd', 2, 128, 0, 64, 32, 3, 'off4', 'gn_fwd_kernel<1>', 'loop'),             # misaligned x1
  ('split_two_sources', 'fwd', 3, 32, 32, 4096, 8, 1, '', 'gn_split_stats+gn_split_fwd', 'split'),   # L = 32768
  ('split_262144', 'fwd', 1, 128, 0, 65536, 32, 1, '', 'gn_split_stats+gn_split_fwd', 'split'),      # the 256 x 256 maps
  ('pl_fused16', 'pl', 2, 128, 0, 16, 32, 1, '', 'gn_fwd_pl_kernel hw16', 'flat'),             # cpg 4
  ('pl_fused64_two_sources', 'pl_max', 2, 128, 128, 64, 32, 1, '', 'gn_fwd_pl_kernel hw64', 'flat'),   # cpg 8: lo / hi halves
  ('pl_fused256', 'pl', 2, 256, 0, 256, 32, 0, 'off4', 'gn_fwd_pl_kernel hw256', 'loop'),      # cpg 8 (off4: not the 2-kernel route)
  ('pl_fused1024', 'pl', 1, 128, 0, 1024, 32, 1, 'off4', 'gn_fwd_pl_kernel hw1024', 'loop'),   # cpg 4, 8 passes
  ('pl_stats', 'pl', 1, 128, 0, 1024, 32, 1, '', 'gn_stats_kernel', 'flat'),                   # two kernels, L = 4096
  ('pl_stats_two_sources', 'pl_max', 2, 128, 128, 256, 32, 1, '', 'gn_stats_kernel', 'flat'),  # cpg 8, groups 16.. in x2
  ('pl_fold', 'pl', 3, 64, 0, 4096, 8, 1, '', 'gn_split_stats+gn_fold_stats', 'split'),        # L = 32768
  ('pl_fold_262144', 'pl', 1, 128, 0, 65536, 32, 1, '', 'gn_split_stats+gn_fold_stats', 'split'),
  ('pl_unfused', 'pl', 2, 256, 128, 64, 32, 1, '', 'unfused:gn_fwd_flat_kernel<3>', 'flat'),   # cpg 12
]
SITE_IDS = [s[0] for s in SITES]
# the places that compute statistics (csrc/groupnorm.hip), each form of them counted once
STAT_SITES = {'gn_fwd_flat_kernel<1>', 'gn_fwd_flat_kernel<2>', 'gn_fwd_flat_kernel<3>', 'gn_fwd_flat_kernel<4>',
              'gn_fwd_kernel<4>', 'gn_fwd_kernel<1>', 'gn_split_stats+gn_split_fwd', 'gn_fwd_pl_kernel hw16',
              'gn_fwd_pl_kernel hw64', 'gn_fwd_pl_kernel hw256', 'gn_fwd_pl_kernel hw1024', 'gn_stats_kernel',
              'gn_split_stats+gn_fold_stats', 'unfused:gn_fwd_flat_kernel<3>'}
BWD_SITES = {'flat', 'split', 'loop'}


def _split_ok(HW, cpg):
  return cpg * HW > 16384 and HW % 4096 == 0


def _fwd_kernel(HW, cpg, aligned, ws):
  """The dispatch of stk_gn_fwd_f32, by the shape rules of csrc/groupnorm.hip."""
  L = cpg * HW
  vec = HW % 4 == 0 and aligned
  if ws and vec and _split_ok(HW, cpg):
    return 'gn_split_stats+gn_split_fwd'
  if vec and L <= 16384:
    L4, T = L // 4, 64
    while T < 1024 and T * 4 < L4:
      T *= 2
    return f'gn_fwd_flat_kernel<{min(-(-L4 // T), 4)}>'
  return 'gn_fwd_kernel<4>' if vec else 'gn_fwd_kernel<1>'


def kernel_reached(lib, site):
  """(statistics kernel, backward kernel) the library takes for `site`: the shape rules, cross-checked with the library's
  own predicates wherever it has one (stk_gn_ws_bytes, stk_gn_fwd_pl_fused, stk_gn_bwd_out_ok)."""
  name, entry, N, C1, C2, HW, G, act, opt, _, _ = site
  C = C1 + C2
  cpg = C // G
  L = cpg * HW
  aligned, ws = 'off4' not in opt, 'nows' not in opt
  split = _split_ok(HW, cpg)
  if lib.is_device:                # (the checker needs no partials: its stk_gn_ws_bytes is the backward's 8 N C only)
    assert (int(lib.gn_ws_bytes(N, C, HW, G)) > 8 * N * C) == split, name
  pow2 = HW >= 16 and HW & (HW - 1) == 0
  flat_shape = pow2 and L <= 16384 and cpg <= 512 and not split
  assert int(lib.gn_bwd_out_ok(C1, C2, HW, G)) == int(flat_shape), name
  bwd = 'split' if aligned and split else 'flat' if aligned and flat_shape else 'loop'
  if entry == 'fwd':
    return _fwd_kernel(HW, cpg, aligned, ws), bwd
  blocks = C % 32 == 0 and C1 % 32 == 0 and cpg <= 32 and 32 % cpg == 0
  two_k = blocks and HW % 128 == 0 and (L <= 16384 or split)
  fused = blocks and cpg >= 4 and HW in (16, 64, 256, 1024)
  if lib.is_device:                # (the checker has no two-kernel route: its predicate is the fused shapes alone)
    assert int(lib.gn_fwd_pl_fused(C1, C2, HW, G)) == int(two_k or fused), name
  if two_k and aligned:
    return ('gn_stats_kernel' if L <= 16384 else 'gn_split_stats+gn_fold_stats'), bwd
  if fused:
    return f'gn_fwd_pl_kernel hw{HW}', bwd
  return 'unfused:' + _fwd_kernel(HW, cpg, aligned, ws), bwd


def run(lib, site, inp):
  """Forward by the site's entry, then stk_gn_bwd_f32 (and stk_gn_bwd_out_f32 where the shape has it) with the mean / rstd
  the forward has just written.  Outputs, records and workspaces start as NaN, the caller-zeroed ones as zero."""
  name, entry, N, C1, C2, HW, G, act, opt, _, _ = site
  C = C1 + C2
  d = dev_of(lib)
  nan = lambda *s: torch.full(s, float('nan'), device=d)

  def place(t):
    if t is None:
      return None
    if 'off4' in opt and t is inp.x1:                              # 4 bytes past a 16-byte boundary
      buf = torch.empty(t.numel() + 1, device=d)
      assert buf.data_ptr() % 16 == 0
      buf[1:] = t.reshape(-1).to(d)
      v = buf[1:].view(t.shape)
      assert v.data_ptr() % 16 == 4 and v.is_contiguous()
      return v
    return t.to(d).contiguous()

  a1, a2, ga, be, dy = place(inp.x1), place(inp.x2), place(inp.gamma), place(inp.beta), place(inp.dy)
  nws = max(int(lib.gn_ws_bytes(N, C, HW, G)) // 4, 2 * N * C) + 64
  ws = None if 'nows' in opt else nan(nws)
  y, mean, rstd = nan(N, C, HW), nan(N * G), nan(N * G)
  out = {}
  if entry == 'fwd':
    call(lib, 'gn_fwd_f32', a1, C1, a2, C2, ga, be, y, mean, rstd, N, HW, G, EPS, act, 0.0, 0, None, ws)
  else:
    rec = nan(256)
    pl = torch.full((int(lib.planes_bytes(N, C, HW)),), 0xAA, dtype=torch.uint8, device=d)
    if entry == 'pl':
      call(lib, 'gn_fwd_pl_f32', a1, C1, a2, C2, ga, be, y, pl, rec, mean, rstd, N, HW, G, EPS, act, 0.0, 0, None, ws)
    else:
      xm = torch.zeros(768, device=d)                              # caller-zeroed (include/stk.h)
      call(lib, 'gn_fwd_pl_max_f32', a1, C1, a2, C2, ga, be, y, pl, rec, mean, rstd, N, HW, G, EPS, act, 0.0, 0, None, ws,
           xm, xm[256:] if C2 else None)
      out['xmax1'], out['xmax2'], out['xmax_rest'] = xm[:256].cpu(), xm[256:512].cpu(), xm[512:].cpu()
    out['rec'] = rec.cpu()
    out['planes'] = pl.cpu()
  out.update(y=y.cpu(), mean=mean.cpu(), rstd=rstd.cpu())
  bws = nan(nws)
  dx1, dx2 = nan(N, C1, HW), (nan(N, C2, HW) if C2 else None)
  dg, db = torch.zeros(C, device=d), torch.zeros(C, device=d)      # accumulated into (include/stk.h)
  call(lib, 'gn_bwd_f32', dy, a1, C1, a2, C2, ga, be, mean, rstd, dx1, 0.0, dx2, 0.0, dg, db, bws, N, HW, G, act, 0.0, 0, None)
  out['dx'] = torch.cat([dx1, dx2], 1).cpu() if C2 else dx1.cpu()
  out['dgamma'], out['dbeta'] = dg.cpu(), db.cpu()
  if int(lib.gn_bwd_out_ok(C1, C2, HW, G)) and 'off4' not in opt:
    ows = nan(nws)
    ex1, ex2 = nan(N, C1, HW), (nan(N, C2, HW) if C2 else None)
    dsum, amax = nan(N, C1, 2), torch.zeros(256, device=d)         # the record: caller-zeroed
    call(lib, 'gn_bwd_out_f32', dy, a1, C1, a2, C2, ga, be, mean, rstd, ex1, 0.0, ex2, 0.0, None, None, ows, N, HW, G, act,
         0.0, 0, None, None, 0.0, dsum, 1.0, None, 0, amax)
    out['dx_out'] = torch.cat([ex1, ex2], 1).cpu() if C2 else ex1.cpu()
    out['dx_out_sum'], out['dx_out_amax'] = dsum.cpu(), amax.cpu()
  if lib.is_device:
    torch.cuda.synchronize()
  return out


def evaluate(out, inp, site):
  """The figures of one launch: name -> (error tensor, bound); the by-products are asserted here."""
  name, entry, N, C1, C2, HW, G, act, opt, _, _ = site
  C = C1 + C2
  ref = inp.ref
  e = group_errors(out, ref, G)
  b = bounds(ref)
  fig = {k: (e[k], b[k]) for k in e}
  if 'dx_out' in out:
    fig['dx_out'] = (group_errors({'dx': out['dx_out']}, ref, G)['dx'], b['dx'])
    s64 = ref['dx'][:, :C1].sum(2)
    sabs = ref['dx'][:, :C1].abs().sum(2).clamp_min(1e-300)
    assert torch.equal(out['dx_out_sum'][:, :, 0], out['dx_out_sum'][:, :, 1])
    # sums of dx1 values that each carry up to bound(group) * max|dx| of their group
    gmax = ref['dx'].reshape(N, G, -1).abs().amax(2).repeat_interleave(C // G, 1)[:, :C1]
    slack = (b['dx'].repeat_interleave(C // G, 1)[:, :C1] * gmax * HW + TOL * sabs)
    fig['dx_out_sum'] = ((out['dx_out_sum'][:, :, 0].double() - s64).abs() / slack, 1.0)
    assert float(out['dx_out_amax'].max()) == float(out['dx_out'][:, :C1].abs().max()), name      # exact: a maximum
  if 'planes' in out:
    want = (float(inp.gamma.abs().max()) * np.sqrt(C // G * HW - 1.0) + float(inp.beta.abs().max()))
    rec = out['rec']
    assert want <= float(rec[0]) <= want * (1 + 2e-5) and float(rec[1:].abs().max()) == 0, name
    assert float(out['y'].abs().max()) <= float(rec[0]), (name, 'the a-priori bound must hold')
    dec, s = decode_planes(out['planes'], rec, N, C, HW)
    ymax = ref['y'].reshape(N, G, -1).abs().amax(2)
    err = (dec - ref['y']).reshape(N, G, -1).abs().amax(2)
    # float64 y at the GroupNorm tolerance plus the planes' own precision: 2^-22 relative, 2^-25 absolute in scaled units
    fig['planes'] = (err / ((TOL + 2.0 ** -22) * ymax + 2.0 ** -25 / s), 1.0)
  if 'xmax1' in out:
    assert float(out['xmax1'].max()) == float(inp.x1.abs().max()), name
    if C2:
      assert float(out['xmax2'].max()) == float(inp.x2.abs().max()), name
    assert float(out['xmax_rest'].abs().max()) == 0.0, name
  return fig


def report(fig, family_mask, what):
  """Print every figure of the groups in `family_mask`, then return the list of misses."""
  bad = []
  for k, (err, bound) in fig.items():
    if err.shape != family_mask.shape:                 # per channel: not of one family (asserted by the caller)
      continue
    bnd = bound if torch.is_tensor(bound) else torch.full_like(err, bound)
    ratio = (err / bnd)[family_mask]
    worst = float(ratio.max())
    print(f'  {what} {k}: worst error / bound = {worst:.3g} (error {float(err[family_mask].max()):.3g})')
    if not worst <= 1.0:
      bad.append((k, worst))
  return bad
