"""Scale-shift GroupNorm conditioning restated for the tests (include/stk_adagn.h; the oracle's RefNet has no such switch):

  xhat = (x - mean_ng) rstd_ng ;  u = gamma_c xhat + beta_c ;  v = u (1 + s_nc) + b_nc ;  y = mask * act(v)

in float64, with its gradients twice -- the closed forms the header states, and autograd on the definition -- the identity
"per sample it equals F.group_norm with (gamma', beta')", the kernel-test cases with their inputs, an AdaRefNet whose
residual blocks modulate GroupNorm_1 when config.model.scale_shift_norm is set, and the same for a stand-alone block.

The metric of the kernel tests is that of tests/_gn_cases.py, judged per (sample, group) / per (sample, channel) / per
channel against the sum of the absolute terms of each figure; `figures` computes every one of them."""
import numpy as np
import torch
import torch.nn.functional as F

import _block_ref
import ref_torch

EPS = 1e-6
TOL = 2e-5          # tests/_gn_cases.py


def act_fn(act, u):
  """STK_ACT_* of include/stk.h"""
  if act == 1:
    return F.silu(u)
  if act == 2:
    return F.relu(u)
  if act == 3:
    return F.leaky_relu(u, 0.2)
  if act == 4:
    return F.elu(u)
  return u


def act_slope(act, u):
  if act == 1:
    sg = torch.sigmoid(u)
    return sg * (1 + u * (1 - sg))
  if act == 2:
    return (u > 0).to(u.dtype)
  if act == 3:
    return torch.where(u > 0, torch.ones_like(u), torch.full_like(u, 0.2))
  if act == 4:
    return torch.where(u > 0, torch.ones_like(u), torch.exp(u))
  return torch.ones_like(u)


def layer(x, gamma, beta, s, b, G, act, mask=None, eps=EPS):
  """The definition, on tensors of any float type: x [N, C, HW], gamma / beta [C], s / b [N, C].  mask [N, C, HW] holds the
  dropout factors (1 / (1 - p) or 0)."""
  N, C, HW = x.shape
  xg = x.reshape(N, G, -1)
  mean = xg.mean(2)
  var = ((xg - mean[:, :, None]) ** 2).mean(2)
  rstd = 1 / torch.sqrt(var + eps)
  xhat = ((xg - mean[:, :, None]) * rstd[:, :, None]).reshape(N, C, HW)
  u = gamma[None, :, None] * xhat + beta[None, :, None]
  v = u * (1 + s[:, :, None]) + b[:, :, None]
  y = act_fn(act, v)
  if mask is not None:
    y = y * mask
  return y, mean, rstd, xhat, v


def folded(x, gamma, beta, s, b, G, act, mask=None, eps=EPS):
  """The same layer as N calls of F.group_norm with the per-sample pair gamma' = gamma (1 + s), beta' = beta (1 + s) + b."""
  out = []
  for n in range(x.shape[0]):
    ga, be = gamma * (1 + s[n]), beta * (1 + s[n]) + b[n]
    out.append(act_fn(act, F.group_norm(x[n:n + 1], G, ga, be, eps)))
  y = torch.cat(out)
  return y * mask if mask is not None else y


def closed_form(x, gamma, beta, s, b, dy, G, act, mask=None, eps=EPS, dtype=torch.float64):
  """Outputs and gradients by the closed forms of include/stk_adagn.h, and the sums of absolute terms that condition each
  figure, in float64 (the reference) or, with dtype=torch.float32, as a plain fp32 evaluation."""
  x, gamma, beta, s, b, dy = (t.to(dtype) for t in (x, gamma, beta, s, b, dy))
  mask = mask.to(dtype) if mask is not None else None
  N, C, HW = x.shape
  y, mean, rstd, xhat, v = layer(x, gamma, beta, s, b, G, act, mask, eps)
  dv = dy * act_slope(act, v)
  if mask is not None:
    dv = dv * mask
  gp = gamma[None, :] * (1 + s)                                # gamma' [N, C]
  dbp, dgp = dv.sum(2), (dv * xhat).sum(2)                     # dbeta', dgamma' [N, C]
  a_db, a_dg = dv.abs().sum(2), (dv * xhat).abs().sum(2)
  t = dv * gp[:, :, None]
  m1 = t.reshape(N, G, -1).mean(2)
  m2 = (t * xhat).reshape(N, G, -1).mean(2)
  rep = lambda m: m.repeat_interleave(C // G, 1)[:, :, None]
  r3 = rep(rstd)
  dx = r3 * (t - rep(m1) - xhat * rep(m2))
  dx_terms = r3 * (t.abs() + rep(m1).abs() + (xhat * rep(m2)).abs())
  return dict(
    y=y, mean=mean, rstd=rstd, dx=dx, dx_terms=dx_terms,
    ds=dgp * gamma[None, :] + dbp * beta[None, :], db=dbp,
    ds_cond=a_dg * gamma.abs()[None, :] + a_db * beta.abs()[None, :], db_cond=a_db,
    dgamma=(dgp * (1 + s)).sum(0), dbeta=(dbp * (1 + s)).sum(0),
    dgamma_cond=((a_dg + a_db) * (1 + s).abs()).sum(0), dbeta_cond=(a_db * (1 + s).abs()).sum(0))


def by_autograd(x, gamma, beta, s, b, dy, G, act, mask=None, eps=EPS):
  """float64 gradients of sum(y * dy) by autograd on the definition: dx, ds, db, dgamma, dbeta."""
  leaves = [t.double().clone().requires_grad_(True) for t in (x, gamma, beta, s, b)]
  y = layer(*leaves, G, act, mask.double() if mask is not None else None, eps)[0]
  g = torch.autograd.grad((y * dy.double()).sum(), leaves)
  return dict(y=y.detach(), dx=g[0], dgamma=g[1], dbeta=g[2], ds=g[3], db=g[4])


# ---- the kernel-test cases -------------------------------------------------------------------------------------------
# (id, N, C, HW, G, act, options): the smallest shapes that reach every route the entries dispatch to
#   flat   register-resident kernels: L = (C / G) HW <= 16384, HW a power of two >= 16 (backward), 16-byte aligned
#   loop   the looping kernels: HW % 4 != 0, or operands off the 16-byte alignment ('off4')
#   split  groups above 16384 elements in whole 4096-float chunks, through ws
# options: 'off4' every operand entered 4 bytes into its buffer, 'x10' x = randn + 10, 's4' s = 4 randn, 'drop' p = 0.1
CASES = [
  ('flat_small', 2, 8, 16, 2, 1, ''),
  ('flat_mid_x10', 3, 128, 64, 32, 2, 'x10'),
  ('flat_largest_n1', 1, 128, 4096, 32, 1, 's4'),          # L = 16384, the largest one-workgroup group; N = 1
  ('split', 2, 32, 8192, 8, 3, 'x10 s4'),
  ('loop_hw25', 2, 48, 25, 12, 4, 's4'),
  ('loop_off4', 2, 32, 64, 8, 1, 'off4 x10'),
  ('flat_drop', 3, 64, 256, 16, 1, 'drop'),
  ('flat_linear_n1', 1, 16, 64, 4, 0, 's4 x10'),
]
CASE_IDS = [c[0] for c in CASES]


def route(case):
  """(forward, backward) route of a case by the shape rules of csrc/groupnorm.hip."""
  _, N, C, HW, G, act, opt = case
  cpg = C // G
  L = cpg * HW
  aligned = 'off4' not in opt
  split = L > 16384 and HW % 4096 == 0
  vec = aligned and HW % 4 == 0
  fwd = 'split' if vec and split else 'flat' if vec and L <= 16384 else 'loop'
  pow2 = HW >= 16 and HW & (HW - 1) == 0
  bwd = 'split' if aligned and split else 'flat' if aligned and pow2 and L <= 16384 and cpg <= 512 else 'loop'
  return fwd, bwd


_INPUTS = {}


def inputs(case):
  """fp32 CPU operands of a case, made once: x, gamma, beta, s, b, dy, the pre-existing dx / dgamma / dbeta.  Some entries
  of s are exactly -1 (gamma' = 0), and the last sample's rows of s and b are all zero."""
  if case[0] in _INPUTS:
    return _INPUTS[case[0]]
  _, N, C, HW, G, act, opt = case
  g = torch.Generator().manual_seed(1 + CASE_IDS.index(case[0]))
  r = lambda *sh: torch.randn(*sh, generator=g)
  x = r(N, C, HW) + (10.0 if 'x10' in opt else 0.0)
  s = r(N, C) * (4.0 if 's4' in opt else 1.0)
  b = r(N, C)
  s[0, ::5] = -1.0
  if N > 1:
    s[-1] = 0.0
    b[-1] = 0.0
  d = dict(x=x, gamma=1 + 0.2 * r(C), beta=0.3 * r(C), s=s, b=b, dy=r(N, C, HW), dx0=r(N, C, HW), dgamma0=r(C), dbeta0=r(C))
  _INPUTS[case[0]] = d
  return d


def figures(got, ref, G):
  """Every figure of the kernel test as {name: worst value / its bound}: <= 1 passes.  got: dict of tensors (any device /
  float type) with any of mean, rstd, y, dx, ds, db, dgamma, dbeta; ref: closed_form's dict (dx of `got` must be compared
  against the caller's own ref['dx'], which may include dx_beta * dx0)."""
  out = {}
  tiny = 1e-300
  g64 = {k: v.detach().cpu().double() for k, v in got.items()}
  N, C, HW = ref['y'].shape
  grp = lambda t: t.reshape(N, G, -1)
  if 'mean' in g64:
    out['mean'] = ((g64['mean'].reshape(N, G) - ref['mean']).abs() * ref['rstd']).max().item() / TOL
  if 'rstd' in g64:
    out['rstd'] = (g64['rstd'].reshape(N, G) / ref['rstd'] - 1).abs().max().item() / TOL
  if 'y' in g64:
    e = grp((g64['y'] - ref['y']).abs()).amax(2) / (grp(ref['y'].abs()).amax(2) + tiny)
    out['y'] = e.max().item() / TOL
  if 'dx' in g64:
    den = grp(ref['dx'].abs()).amax(2) + tiny
    cond = torch.clamp(grp(ref['dx_terms']).amax(2) / den, min=1.0)
    e = grp((g64['dx'] - ref['dx']).abs()).amax(2) / den
    out['dx'] = (e / cond).max().item() / TOL
  for k in ('ds', 'db', 'dgamma', 'dbeta'):
    if k in g64:
      out[k] = ((g64[k] - ref[k]).abs() / (ref[k + '_cond'] + tiny)).max().item() / TOL
  return out


# ---- the network and the stand-alone blocks --------------------------------------------------------------------------
class AdaRefNet(ref_torch.RefNet):
  """RefNet whose residual blocks, under config.model.scale_shift_norm, take Dense_0(act(temb)) [B, 2 out_ch] as the
  (scale, shift) of GroupNorm_1 instead of adding it to Conv_0's output."""

  def _res(self, i, a, x, temb):
    m = self.config.model
    if not getattr(m, 'scale_shift_norm', False):
      return super()._res(i, a, x, temb)
    pre = f'all_modules.{i}'
    fir, k = m.fir, m.fir_kernel
    h = self._act(self._gn(pre + '.GroupNorm_0', x))
    if m.resblock_type.lower() == 'biggan':
      if a['up']:
        h, x = (ref_torch.upsample_2d(h, k), ref_torch.upsample_2d(x, k)) if fir else \
          (ref_torch.naive_upsample_2d(h), ref_torch.naive_upsample_2d(x))
      elif a['down']:
        h, x = (ref_torch.downsample_2d(h, k), ref_torch.downsample_2d(x, k)) if fir else \
          (ref_torch.naive_downsample_2d(h), ref_torch.naive_downsample_2d(x))
    h = self._conv(pre + '.Conv_0', h)
    mod = F.linear(self._act(temb), self.P(pre + '.Dense_0.weight'), self.P(pre + '.Dense_0.bias'))
    C = h.shape[1]
    assert mod.shape[1] == 2 * C
    h = self._gn(pre + '.GroupNorm_1', h) * (1 + mod[:, :C, None, None]) + mod[:, C:, None, None]
    h = self._dropout(self._act(h), m.dropout)
    h = self._conv(pre + '.Conv_1', h)
    if self.has(pre + '.Conv_2.weight'):
      x = self._conv(pre + '.Conv_2', x)
    elif self.has(pre + '.NIN_0.W'):
      x = self._nin(pre + '.NIN_0', x)
    return (x + h) / np.sqrt(2.) if m.skip_rescale else x + h


def block_forward(m, P, x, temb):
  """A stand-alone ResnetBlockBigGANpp / ResnetBlockDDPMpp with scale_shift_norm on float64 tensors (tests/_block_ref.py
  restates the block without the switch)."""
  R = _block_ref
  act = R.act_fn(m.act)
  h = act(R._gn(P, 'GroupNorm_0.', m.GroupNorm_0, x))
  if getattr(m, 'up', False) or getattr(m, 'down', False):
    if m.up:
      rs = (lambda t: R.upsample_2d(t, m.fir_kernel)) if m.fir else R.naive_upsample_2d
    else:
      rs = (lambda t: R.downsample_2d(t, m.fir_kernel)) if m.fir else R.naive_downsample_2d
    h, x = rs(h), rs(x)
  h = R._conv(P, 'Conv_0.', m.Conv_0, h)
  mod = F.linear(act(temb), P('Dense_0.weight'), P('Dense_0.bias'))
  C = h.shape[1]
  h = act(R._gn(P, 'GroupNorm_1.', m.GroupNorm_1, h) * (1 + mod[:, :C, None, None]) + mod[:, C:, None, None])
  h = R._conv(P, 'Conv_1.', m.Conv_1, h)
  if hasattr(m, 'Conv_2'):
    x = R._conv(P, 'Conv_2.', m.Conv_2, x)
  elif hasattr(m, 'NIN_0'):
    x = R._nin(P, 'NIN_0.', x)
  return (x + h) / R.SQRT2 if m.skip_rescale else x + h


def block_run(m, x, temb, gout):
  """(out, {input grads}, {parameter grads}) in float64 for the loss sum(out * gout)."""
  P = _block_ref._Params(m)
  xs = {'x': x.detach().cpu().double().requires_grad_(True), 'temb': temb.detach().cpu().double().requires_grad_(True)}
  out = block_forward(m, P, xs['x'], xs['temb'])
  names = list(xs) + [n for n, t in P.t.items() if t.requires_grad]
  leaves = list(xs.values()) + [t for t in P.t.values() if t.requires_grad]
  grads = dict(zip(names, torch.autograd.grad(out, leaves, gout.detach().cpu().double())))
  return out.detach(), {n: grads[n] for n in xs}, {n: g for n, g in grads.items() if n not in xs}
