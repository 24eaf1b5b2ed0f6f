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

Dynamic thresholding (Saharia et al. 2022, "Imagen", section 2.3; opt-in: ``threshold=(p, floor)``,
``config.sampling.dpm_threshold / dpm_threshold_floor``) replaces the static clamp for guided sampling at large weights: per
sample, s = max(floor, the p-quantile of |d_i|) and d_i <- clamp(d_i, -s, s) / s.  The quantile is the order statistic of
rank ``threshold_rank(p, n)`` = min(n - 1, ceil(p (n - 1))) of the n = C H W absolute values -- the "higher" of the two
order statistics a linearly interpolated percentile (``torch.quantile``, numpy's default) lies between, so it differs from
that percentile by less than one spacing of order statistics.  A thresholded step is four streaming launches of
include/stk_guided.h (csrc/guided.hip): ``stk_dpm_predict_f32``, two levels of ``stk_abs_select_f32`` and
``stk_dpm_threshold_update_f32``, on a scratch, a q[B] and a workspace allocated once per run; the final ``denoise``
evaluation is thresholded too.  It is defined on centred data (``config.data.centered``), excludes ``clip``, and needs a
library with include/stk_guided.h (refused when the sampler is built).  Without ``threshold`` the loop is launch for launch
the one above.  ``dynamic_threshold`` is the same thresholding for a user's own loop.  Not covered: the DPS sampler's
``stk_tweedie_f32`` (its backward seed treats the clamp's bounds as constants) and the PC, ODE and adaptive samplers, which
form no data prediction.  Sample quality under thresholding is unmeasured: no class-conditional checkpoint exists.
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


_fp32 = mutils.fp32_levels


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


def _guided_library():
  return mutils.require('has_guided', 'stk_guided.h', 'stk_dpm_predict_f32, stk_abs_select_f32 and stk_dpm_threshold_update_f32',
                        'dynamic thresholding needs')


def threshold_rank(p, n):
  """The 0-based rank min(n - 1, ceil(p (n - 1))) among n sorted absolute values that stands for the p-quantile: in float64,
  the "higher" order statistic (module docstring)."""
  return min(int(n) - 1, int(math.ceil(float(p) * (int(n) - 1))))


def _threshold_pair(threshold):
  """None, or (p, floor) as floats: ValueError unless 0 < p <= 1 and floor is positive and finite."""
  if threshold is None:
    return None
  try:
    p, floor = (float(v) for v in threshold)
  except (TypeError, ValueError):
    raise ValueError(f'threshold must be (p, floor), got {threshold!r}') from None
  if not 0. < p <= 1.:
    raise ValueError(f'threshold: p must lie in (0, 1], got {p!r}')
  if not (floor > 0. and math.isfinite(floor)):
    raise ValueError(f'threshold: floor must be positive and finite, got {floor!r}')
  return p, floor


def _check_threshold(threshold, clip):
  pair = _threshold_pair(threshold)
  if pair is not None and clip is not None:
    raise ValueError(f'threshold={threshold!r} and clip={clip!r} exclude each other: dynamic thresholding replaces the static clamp')
  return pair


class _Thresholder:
  """What a thresholded run allocates once: the d_raw scratch, q[B] and the workspace of include/stk_guided.h."""

  def __init__(self, lib, x, p, floor):
    self.lib, self.floor = lib, float(floor)
    self.B, self.n = x.shape[0], x.numel() // x.shape[0]
    self.rank = threshold_rank(p, self.n)
    self.ws_bytes = int(lib.guided_ws_bytes(self.B, self.n))
    if self.ws_bytes < 0:
      raise ValueError(f'stk_guided_ws_bytes refuses a state of {self.B} rows of {self.n} (rc={self.ws_bytes})')
    self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=x.device)
    self.q = torch.empty(self.B, dtype=torch.float32, device=x.device)
    self.d_raw = torch.empty_like(x)

  def select(self, v, first_level_done):
    """q[b] = the rank-th smallest |v[b]|."""
    self.lib.abs_select_f32(v.data_ptr(), self.B, self.n, self.rank, self.q.data_ptr(), self.ws.data_ptr(), self.ws_bytes,
                            1 if first_level_done else 0, stk_lib.stream_ptr(v.device))

  def apply(self, x, d_raw, d_prev, g, A, B, x_out, d_out):
    ptr = lambda t: None if t is None else t.data_ptr()
    self.lib.dpm_threshold_update_f32(ptr(x), d_raw.data_ptr(), ptr(d_prev), self.q.data_ptr(), self.floor, float(g), float(A),
                                      float(B), ptr(x_out), ptr(d_out), self.B, self.n, stk_lib.stream_ptr(d_raw.device))

  def update(self, x, score, d_prev, row, x_out, d_out):
    """One thresholded step: predict, two select levels, update.  row: (cx, cs, g, A, B)."""
    cx, cs, g, A, B = (float(v) for v in row)
    with stk_lib.device_guard(x.device):
      self.lib.dpm_predict_f32(x.data_ptr(), score.data_ptr(), cx, cs, self.d_raw.data_ptr(), self.B, self.n, self.ws.data_ptr(),
                               self.ws_bytes, stk_lib.stream_ptr(x.device))
      self.select(self.d_raw, True)
      self.apply(x, self.d_raw, d_prev, g, A, B, x_out, d_out)
    return x_out


def dynamic_threshold(x0, p, floor=1.0):
  """Dynamic thresholding of a data prediction for a user's own loop -> ``(x0_thresholded, s)``: per sample
  s = max(floor, the order statistic of rank ``threshold_rank(p, n)`` of |x0|) as a [B] tensor (NaN for a sample that holds
  a NaN at or below that rank) and x0_thresholded = clamp(x0, -s, s) / s, a new tensor.  x0: a contiguous float32 device
  tensor [B, ...].  One selection (``stk_abs_select_f32``) and one streaming pass, on the device only."""
  p, floor = _threshold_pair((p, floor))
  lib = _guided_library()
  mutils.check_inplace_state(x0, lib, why='the kernels read it in place')
  th = _Thresholder(lib, x0, p, floor)
  out = th.d_raw
  with stk_lib.device_guard(x0.device):
    th.select(x0, False)
    th.apply(None, x0, None, 0., 0., 1., None, out)
  q = th.q
  return out, torch.where(torch.isnan(q), q, q.clamp_min(floor))


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


def dpm_sample(score_fn, x, schedule, clip=None, denoise=False, threshold=None):
  """The loop: `x` (a contiguous fp32 device tensor drawn from the prior at the schedule's T) is advanced IN PLACE to the
  schedule's eps and returned.  Per step one ``score_fn(x, ones(B) * t_i)`` and one launch; the previous data prediction
  lives in one buffer, overwritten in place.  clip = (lo, hi) clamps every data prediction.  denoise: one more evaluation
  at eps, after which `x` holds the data prediction there.  threshold = (p, floor): every data prediction, the one of
  `denoise` included, is thresholded dynamically instead (module docstring): four launches per step."""
  lib = _library()
  pair = _check_threshold(threshold, clip)
  if pair is not None:
    _guided_library()
  mutils.check_inplace_state(x, lib)
  bounds = _clip_bounds(clip)
  th = _Thresholder(lib, x, *pair) if pair is not None else None
  rows = list(schedule.coeffs) + ([schedule.final] if denoise else [])
  times = list(schedule.times[:-1]) + ([schedule.times[-1]] if denoise else [])
  ones = torch.ones(x.shape[0], dtype=torch.float32, device=x.device)
  hist = None
  for i, (row, t) in enumerate(zip(rows, times)):
    score = mutils.checked_score(score_fn, x, ones * float(t), lib)
    keep = i + 1 < len(rows) and rows[i + 1][2] != 0.       # the next step extrapolates from this data prediction
    if keep and hist is None:
      hist = torch.empty_like(x)
    if th is None:
      _update(lib, x, score, hist if row[2] != 0. else None, row, bounds, x, hist if keep else None)
    else:
      th.update(x, score, hist if row[2] != 0. else None, row, x, hist if keep else None)
  return x


def get_dpm_sampler(config, sde, shape, inverse_scaler, steps=20, order=2, skip='logsnr', denoise=True, clip=None, eps=1e-3,
                    device='cuda', precision='fp32', lower_order_final=True, threshold=None):
  """``dpm_sampler(model) -> (samples, nfe)`` with ``nfe = steps + (1 if denoise else 0)``: DPM-Solver++ of `order` over
  `steps` steps from ``sde.T`` down to `eps`.  denoise: return the data prediction at eps (one more evaluation) instead of
  the state there.  precision='fp16': every network evaluation runs in the engine's fp16 mode (models.utils.precision).
  threshold = (p, floor): dynamic thresholding of every data prediction (module docstring); ValueError together with `clip`
  or with ``config.data.centered`` false."""
  lib = _library()
  schedule = dpm_schedule(sde, steps, order=order, skip=skip, eps=eps, lower_order_final=lower_order_final)
  _clip_bounds(clip)
  if _check_threshold(threshold, clip) is not None:
    _guided_library()
    if not config.data.centered:
      raise ValueError('dynamic thresholding is defined on centred data: config.data.centered is false')
  mutils.check_precision(precision)
  nfe = schedule.steps + (1 if denoise else 0)

  def dpm_sampler(model):
    with mutils.sampling_run(model, precision):
      score_fn, x = mutils.score_and_prior(config, sde, model, shape, device, lib)
      x = dpm_sample(score_fn, x, schedule, clip=clip, denoise=denoise, threshold=threshold)
      return inverse_scaler(x), nfe

  return dpm_sampler


def sampling_options(config):
  """(steps, order, skip, clip) of ``config.sampling.dpm_steps / dpm_order / dpm_skip / dpm_clip``: 20, 2, 'logsnr' and None
  where a key is absent (the reference's configs have none)."""
  read = lambda key, default: mutils.config_option(config, 'sampling', key, default)
  clip = read('dpm_clip', None)
  return read('dpm_steps', 20), read('dpm_order', 2), read('dpm_skip', 'logsnr'), None if clip is None else tuple(clip)


def threshold_options(config):
  """``threshold`` of ``config.sampling.dpm_threshold`` (p; None where absent: no thresholding) and
  ``config.sampling.dpm_threshold_floor`` (1.0 where absent): None or (p, floor)."""
  p = mutils.config_option(config, 'sampling', 'dpm_threshold', None)
  if p is None:
    return None
  return float(p), float(mutils.config_option(config, 'sampling', 'dpm_threshold_floor', 1.0))
