"""DPM-Solver++ in its data-prediction form: a few-step deterministic sampler (Lu et al., "DPM-Solver++: Fast Solver for
Guided Sampling of Diffusion Probabilistic Models", 2022).  Order 1 is DDIM; order 2 is the multistep form 2M, one network
evaluation per step.  Twenty to fifty evaluations stand where ``sampling.get_pc_sampler`` takes one to two thousand.

With alpha_t, sigma_t the mean coefficient and the std of ``sde.marginal_prob``, lambda = log(alpha / sigma) and
h_i = lambda_{i+1} - lambda_i, one step from t_i to t_{i+1} is

  d_i     = (x_i + sigma_i^2 score(x_i, t_i)) / alpha_i            the data prediction, optionally clamped to `clip`
  D_i     = d_i + h_i / (2 h_{i-1}) (d_i - d_{i-1})                second order (1 / (2 r) with r = h_{i-1} / h_i);  D_i = d_i first order
  x_{i+1} = sigma_{i+1} / sigma_i x_i - alpha_{i+1} expm1(-h_i) D_i

``dpm_schedule`` turns an SDE and a step count into the host coefficients ``(cx, cs, g, A, B)`` of every step, in float64
from times rounded to fp32 first (the network sees exactly the t the coefficients were computed at);  ``dpm_sample`` is the
loop over any score function: per step ONE ``score_fn(x, ones(B) * t_i)`` and ONE launch of ``stk_dpm_update_f32``
(include/stk_solver.h, csrc/solver.hip), state and history updated in place;  ``get_dpm_sampler`` binds both to a model the
way ``sampling.get_pc_sampler`` does.  Order 2 takes a first-order step first (there is no history yet) and, below 15 steps,
a first-order last step as well (the solver's published ``lower_order_final``; ``lower_order_final=False`` switches it off).

The only random draw of a whole run is the single ``sde.prior_sampling(shape)``: that is part of the interface.  The network
evaluations follow the engine's conventions as ``get_pc_sampler`` does: ``torch.no_grad``, weights prepared once per run
(``models.utils.frozen_weights``), ``precision`` ('fp16' applies to the network only: the update is always fp32).
Everything runs on the device: host tensors raise the package's device error, there is no CPU path; a library without
include/stk_solver.h is refused when the sampler is built.  Sample quality (FID) at any step count is unmeasured.
"""
import math

import numpy as np
import torch

from . import sde_lib
from .engine import lib as stk_lib
from .models import utils as mutils

SKIPS = ('logsnr', 'time', 'time_quadratic')
LOWER_ORDER_FINAL_BELOW = 15     # order 2 ends with a first-order step when steps < 15 (DPM-Solver's lower_order_final)
_INF = float('inf')


def _library():
  return mutils.require('has_solver', 'stk_solver.h', 'stk_dpm_update_f32', 'the DPM-Solver++ sampler needs')


def alpha_sigma(sde, t):
  """(alpha, sigma) of ``sde.marginal_prob`` at the float64 times `t` (any array-like), as float64 numpy vectors: the mean
  and the std of a tensor of ones.  reciprocal_VESDE's marginal_prob rounds its std to fp32, so its alpha = 1 and
  sigma = sqrt(c b^(2/t) + c2 b2^(2/t)) are restated here from the SDE's own constants."""
  t = torch.as_tensor(np.asarray(t, dtype=np.float64)).reshape(-1)
  if isinstance(sde, sde_lib.reciprocal_VESDE):
    alpha, sigma = torch.ones_like(t), torch.sqrt(sde._variance(t))
  else:
    mean, sigma = sde.marginal_prob(torch.ones((t.shape[0], 1, 1, 1), dtype=torch.float64), t)
    alpha = mean.reshape(-1)
  if alpha.dtype != torch.float64 or sigma.dtype != torch.float64:
    raise TypeError(f'{type(sde).__name__}.marginal_prob does not carry float64 through ({alpha.dtype}, {sigma.dtype})')
  return alpha.numpy().copy(), sigma.reshape(-1).numpy().copy()


def _lam(sde, t):
  alpha, sigma = alpha_sigma(sde, t)
  with np.errstate(divide='ignore', invalid='ignore'):
    return np.log(alpha) - np.log(sigma)


def _fp32(v):
  return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def _invert_lambda(sde, targets, lo, hi):
  """t in [lo, hi] with lambda(t) = target, by bisection in float64 (lambda falls as t grows)."""
  a, b = np.full_like(targets, lo), np.full_like(targets, hi)
  for _ in range(200):
    mid = 0.5 * (a + b)
    above = _lam(sde, mid) > targets            # lambda(mid) still too large: the root lies at a later time
    a, b = np.where(above, mid, a), np.where(above, b, mid)
  return 0.5 * (a + b)


class DpmSchedule:
  """The host record of one run, float64 numpy throughout.  ``times`` [steps + 1] from T down to eps, every entry
  fp32-representable; ``alpha``, ``sigma``, ``lam`` there; ``h`` [steps]; ``orders`` [steps] (1 or 2);  ``coeffs``
  [steps, 5], the rows ``(cx, cs, g, A, B)`` of include/stk_solver.h;  ``final`` the row of the optional last evaluation at
  eps, which returns the data prediction itself (A = 0, B = 1, g = 0)."""

  def __init__(self, **fields):
    self.__dict__.update(fields)

  def __repr__(self):
    return (f'DpmSchedule({self.sde_name}, steps={self.steps}, order={self.order}, skip={self.skip!r}, '
            f'T={float(self.times[0])!r}, eps={float(self.times[-1])!r})')


def dpm_schedule(sde, steps, order=2, skip='logsnr', eps=None, T=None, lower_order_final=True):
  """The time grid and the per-step coefficients of DPM-Solver++ (module docstring) for `sde`, as a :class:`DpmSchedule`.

  skip: 'logsnr' (uniform in lambda), 'time' (uniform in t) or 'time_quadratic' (uniform in sqrt(t)).  eps, T: the ends of
  the grid (default ``sde.eps``, or 1e-3 for an SDE without one, and ``sde.T``), rounded to fp32 like every other time.
  lambda must rise strictly along the grid and on [eps, T], and sigma must stay positive: otherwise ValueError."""
  name = type(sde).__name__
  if order not in (1, 2):
    raise ValueError(f'order must be 1 or 2, got {order!r}')
  if int(steps) != steps or steps < 1:
    raise ValueError(f'steps must be a positive integer, got {steps!r}')
  steps = int(steps)
  if skip not in SKIPS:
    raise ValueError(f'skip must be one of {SKIPS}, got {skip!r}')
  t_hi = float(_fp32(sde.T if T is None else T))
  t_lo = float(_fp32(getattr(sde, 'eps', 1e-3) if eps is None else eps))
  if not 0. < t_lo < t_hi:
    raise ValueError(f'{name}: the grid must run from T down to eps with 0 < eps < T, got T = {t_hi!r}, eps = {t_lo!r}: '
                     f'lambda would not rise from time {t_hi!r} on')
  # lambda must be monotone on the whole interval, not only on the grid: the inversion below relies on it
  dense = np.exp(np.linspace(math.log(t_hi), math.log(t_lo), 513))
  dense[0], dense[-1] = t_hi, t_lo
  _check_grid(name, dense, *alpha_sigma(sde, dense))
  if skip == 'logsnr':
    ends = _lam(sde, [t_hi, t_lo])
    times = _invert_lambda(sde, np.linspace(ends[0], ends[1], steps + 1), t_lo, t_hi)
  elif skip == 'time':
    times = np.linspace(t_hi, t_lo, steps + 1)
  else:
    times = np.linspace(math.sqrt(t_hi), math.sqrt(t_lo), steps + 1) ** 2
  times = _fp32(times)
  times[0], times[-1] = t_hi, t_lo
  alpha, sigma = alpha_sigma(sde, times)
  lam = _check_grid(name, times, alpha, sigma)
  h = np.diff(lam)
  orders = np.ones(steps, dtype=np.int64)
  if order == 2:
    orders[1:] = 2
    if lower_order_final and steps < LOWER_ORDER_FINAL_BELOW:
      orders[-1] = 1
  g = np.zeros(steps)
  second = np.nonzero(orders == 2)[0]
  g[second] = h[second] / (2. * h[second - 1])
  coeffs = np.stack([1. / alpha[:-1], sigma[:-1] ** 2 / alpha[:-1], g, sigma[1:] / sigma[:-1], -alpha[1:] * np.expm1(-h)],
                    axis=1)
  final = np.array([1. / alpha[-1], sigma[-1] ** 2 / alpha[-1], 0., 0., 1.])
  return DpmSchedule(sde_name=name, steps=steps, order=order, skip=skip, lower_order_final=bool(lower_order_final),
                     times=times, alpha=alpha, sigma=sigma, lam=lam, h=h, orders=orders, coeffs=coeffs, final=final)


def _check_grid(name, times, alpha, sigma):
  """lambda on `times` (falling); ValueError naming the SDE and the first offending time."""
  bad = np.nonzero(~(np.isfinite(sigma) & (sigma > 0.) & np.isfinite(alpha) & (alpha > 0.)))[0]
  if bad.size:
    i = bad[0]
    raise ValueError(f'{name}: alpha = {alpha[i]!r}, sigma = {sigma[i]!r} at time {times[i]!r}: both must be positive')
  lam = np.log(alpha) - np.log(sigma)
  bad = np.nonzero(~(np.diff(lam) > 0.))[0]
  if bad.size:
    i = bad[0]
    raise ValueError(f'{name}: lambda = log(alpha / sigma) does not rise from time {times[i]!r} (lambda {lam[i]!r}) to '
                     f'time {times[i + 1]!r} (lambda {lam[i + 1]!r}): DPM-Solver++ needs a strictly monotone lambda')
  return lam


def _clip_bounds(clip):
  if clip is None:
    return -_INF, _INF
  lo, hi = (float(v) for v in clip)
  if not lo <= hi:
    raise ValueError(f'clip must be (lo, hi) with lo <= hi, got {clip!r}')
  return lo, hi


def _update(lib, x, score, d_prev, row, bounds, x_out, d_out):
  """One launch of stk_dpm_update_f32 on contiguous fp32 device tensors.  row: (cx, cs, g, A, B)."""
  cx, cs, g, A, B = (float(v) for v in row)
  with stk_lib.device_guard(x.device):
    lib.dpm_update_f32(x.data_ptr(), score.data_ptr(), d_prev.data_ptr() if d_prev is not None else None, cx, cs, g, A, B,
                       bounds[0], bounds[1], x_out.data_ptr(), d_out.data_ptr() if d_out is not None else None, x.numel(),
                       stk_lib.stream_ptr(x.device))
  return x_out


def dpm_sample(score_fn, x, schedule, clip=None, denoise=False):
  """The loop: `x` (a contiguous fp32 device tensor drawn from the prior at the schedule's T) is advanced IN PLACE to the
  schedule's eps and returned.  Per step one ``score_fn(x, ones(B) * t_i)`` and one launch; the previous data prediction
  lives in one buffer, overwritten in place.  clip = (lo, hi) clamps every data prediction.  denoise: one more evaluation
  at eps, after which `x` holds the data prediction there."""
  lib = _library()
  mutils.check_inplace_state(x, lib)
  bounds = _clip_bounds(clip)
  rows = list(schedule.coeffs) + ([schedule.final] if denoise else [])
  times = list(schedule.times[:-1]) + ([schedule.times[-1]] if denoise else [])
  ones = torch.ones(x.shape[0], dtype=torch.float32, device=x.device)
  hist = None
  for i, (row, t) in enumerate(zip(rows, times)):
    score = mutils.checked_score(score_fn, x, ones * float(t), lib)
    keep = i + 1 < len(rows) and rows[i + 1][2] != 0.       # the next step extrapolates from this data prediction
    if keep and hist is None:
      hist = torch.empty_like(x)
    _update(lib, x, score, hist if row[2] != 0. else None, row, bounds, x, hist if keep else None)
  return x


def get_dpm_sampler(config, sde, shape, inverse_scaler, steps=20, order=2, skip='logsnr', denoise=True, clip=None, eps=1e-3,
                    device='cuda', precision='fp32', lower_order_final=True):
  """``dpm_sampler(model) -> (samples, nfe)`` with ``nfe = steps + (1 if denoise else 0)``: DPM-Solver++ of `order` over
  `steps` steps from ``sde.T`` down to `eps`.  denoise: return the data prediction at eps (one more evaluation) instead of
  the state there.  precision='fp16': every network evaluation runs in the engine's fp16 mode (models.utils.precision)."""
  lib = _library()
  schedule = dpm_schedule(sde, steps, order=order, skip=skip, eps=eps, lower_order_final=lower_order_final)
  _clip_bounds(clip)
  mutils.check_precision(precision)
  nfe = schedule.steps + (1 if denoise else 0)

  def dpm_sampler(model):
    with mutils.sampling_run(model, precision):
      score_fn, x = mutils.score_and_prior(config, sde, model, shape, device, lib)
      x = dpm_sample(score_fn, x, schedule, clip=clip, denoise=denoise)
      return inverse_scaler(x), nfe

  return dpm_sampler


def sampling_options(config):
  """(steps, order, skip, clip) of ``config.sampling.dpm_steps / dpm_order / dpm_skip / dpm_clip``: 20, 2, 'logsnr' and None
  where a key is absent (the reference's configs have none)."""
  read = lambda key, default: mutils.config_option(config, 'sampling', key, default)
  clip = read('dpm_clip', None)
  return read('dpm_steps', 20), read('dpm_order', 2), read('dpm_skip', 'logsnr'), None if clip is None else tuple(clip)
