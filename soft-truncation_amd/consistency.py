"""Consistency training and consistency sampling on ``sde_lib.EDM`` (Song et al., "Consistency Models", 2023, with the recipe
of Song & Dhariwal, "Improved Techniques for Training Consistency Models", 2023 -- iCT): the network of the EDM family is
trained from scratch to map any noise level straight to data, without a teacher, a perceptual metric or an EMA target, and a
sample costs one network evaluation (or one per level of a short decreasing list), where the Heun sampler of edm.py takes 35.

With s = sigma_data and e = sigma_min the consistency function is f(x; sigma) = c_skip x + c_out F(c_in x; c_noise),

  c_in = 1 / sqrt(sigma^2 + s^2),  c_skip = s^2 / ((sigma - e)^2 + s^2),  c_out = s (sigma - e) / sqrt(sigma^2 + s^2),
  c_noise = ln(sigma) / 4,

so that f(x; e) = x (include/stk_consistency.h).  This module holds the host definitions, float64 numpy throughout --
``ct_levels`` (the rho-grid of N levels), ``ct_num_levels`` (the doubling curriculum N(k)), ``ct_index_pmf`` (the discretised
log-normal over neighbouring pairs) and ``ct_coefficients`` -- and the sampler: ``consistency_schedule`` turns a list of levels
into the scalars of every launch, ``consistency_sample`` is the loop over any ``F(x_in, c_noise)``, one evaluation and one
``stk_ct_step_f32`` per level, and ``get_consistency_sampler`` binds both to a model the way ``edm.get_edm_sampler`` does.  The
loss is ``losses.get_consistency_loss_fn``.

The random draws of a sampling run are ``noise_fn(x)`` (``torch.randn_like`` where None) once for the start and once per
further level, in level order: that is part of the interface.  The network evaluations follow the engine's conventions:
``torch.no_grad``, weights prepared once per run, ``precision`` ('fp16' applies to the network only: the updates are always
fp32).  Everything runs on the device: host tensors raise the package's device error, there is no CPU path; a library without
include/stk_consistency.h is refused when the sampler is built.  Sample quality is unmeasured: no checkpoint exists.
"""
import math

import numpy as np
import torch
from scipy import special

from . import sde_lib
from .engine import lib as stk_lib
from .models import utils as mutils
from .op import _backend

RHO = 7.
_INF = float('inf')


def _library():
  return mutils.require('has_consistency', 'stk_consistency.h', 'stk_ct_step_f32', 'the consistency sampler needs')


_fp32, _ptr = mutils.fp32_levels, mutils.optional_ptr


def _need_edm(sde, who):
  if not isinstance(sde, sde_lib.EDM):
    raise ValueError(f'{who} needs sde_lib.EDM (config.training.sde = \'edm\'), got {type(sde).__name__}')


def ct_coefficients(sigma, sigma_data, sigma_min):
  """(c_in, c_in sigma, c_skip, c_out, c_noise) at the float64 levels `sigma` (any array-like), float64 numpy, in the
  operation order of include/stk_consistency.h."""
  S, d, e = np.asarray(sigma, dtype=np.float64), float(sigma_data), float(sigma_min)
  v = S * S + d * d
  q = np.sqrt(v)
  g = S - e
  w = g * g + d * d
  return 1. / q, S / q, (d * d) / w, (d * g) / q, np.log(S) / 4.


def ct_levels(sde, N, rho=RHO):
  """sigma_1 < ... < sigma_N, float64 numpy: sigma_i = (sigma_min^(1/rho) + (i - 1) / (N - 1) (sigma_max^(1/rho) -
  sigma_min^(1/rho)))^rho, each rounded to fp32, the two ends set to (the fp32 values of) sigma_min and sigma_max exactly.
  ValueError: N not an integer >= 2, two levels that coincide in fp32."""
  _need_edm(sde, 'ct_levels')
  if isinstance(N, bool) or int(N) != N or N < 2:
    raise ValueError(f'N must be an integer >= 2 (sigma_min and sigma_max are both on the grid), got {N!r}')
  N = int(N)
  lo, hi = float(_fp32(sde.sigma_min)), float(_fp32(sde.sigma_max))
  ramp = np.arange(N, dtype=np.float64) / (N - 1)
  sig = _fp32((lo ** (1. / rho) + ramp * (hi ** (1. / rho) - lo ** (1. / rho))) ** rho)
  sig[0], sig[-1] = lo, hi
  if not bool((np.diff(sig) > 0.).all()):
    raise ValueError(f'N = {N}: two noise levels coincide in fp32')
  return sig


def ct_num_levels(k, K, s0=10, s1=1280):
  """N(k) = min(s0 2^floor(k / K'), s1) + 1 with K' = floor(K / (log2(s1 / s0) + 1)) (at least 1): the number of levels at
  training step k of K, doubling from s0 + 1 to s1 + 1."""
  k, K, s0, s1 = int(k), int(K), int(s0), int(s1)
  if not (0 < s0 <= s1) or K < 1 or k < 0:
    raise ValueError(f'ct_num_levels needs 0 < s0 <= s1, K >= 1 and k >= 0, got k={k}, K={K}, s0={s0}, s1={s1}')
  per = max(1, int(math.floor(K / (math.log2(s1 / s0) + 1.))))
  doublings = min(k // per, 64)                           # 2^64 s0 exceeds any s1 an int holds here
  return min(s0 * 2 ** doublings, s1) + 1


def ct_index_pmf(levels, p_mean=-1.1, p_std=2.0):
  """p(i), i = 1 .. N - 1, of the pair (sigma_i, sigma_{i+1}): the mass a log-normal(p_mean, p_std) gives to
  [sigma_i, sigma_{i+1}], erf((ln sigma_{i+1} - p_mean) / (sqrt(2) p_std)) - erf((ln sigma_i - p_mean) / (sqrt(2) p_std)),
  normalised to sum 1 (the raw differences sum to twice the mass of [sigma_min, sigma_max]).  float64 numpy [N - 1]."""
  if not p_std > 0:
    raise ValueError(f'p_std must be positive, got {p_std!r}')
  edge = special.erf((np.log(np.asarray(levels, dtype=np.float64)) - float(p_mean)) / (math.sqrt(2.) * float(p_std)))
  raw = np.diff(edge)
  return raw / raw.sum()


class ConsistencySchedule:
  """The host record of one sampling run, float64 numpy, every level fp32-representable.  ``levels`` [n] strictly decreasing
  in (sigma_min, sigma_max];  ``rows`` [n, 5] = ``(cs, co, c_z, c_in_next, c_noise)``: c_skip and c_out at the level, then
  sqrt(next^2 - sigma_min^2) and c_in(next) (both 0 in the last row), and the conditioning of the evaluation in front of the
  launch;  ``c_in_first``;  ``lo``, ``hi``: the clamp;  ``nfe`` = n."""

  def __init__(self, **fields):
    self.__dict__.update(fields)

  def __repr__(self):
    return f'ConsistencySchedule(levels={[float(v) for v in self.levels]!r}, clip=({self.lo!r}, {self.hi!r}), nfe={self.nfe})'


def consistency_schedule(sde, levels=None, clip=True):
  """The scalars of every launch of the consistency sampler for `sde` at `levels` (``(sigma_max,)`` where None: one step;
  ``(80, 0.821)`` is the two-step CIFAR-10 setting of the paper), each rounded to fp32 first: the network sees exactly the
  level the coefficients were computed at.  clip: clamp every x0 to the data range [-1, 1].  ValueError: levels empty, not
  strictly decreasing, or outside (sigma_min, sigma_max]."""
  _need_edm(sde, 'the consistency sampler')
  e, top = mutils.ct_sigma_min(sde), float(_fp32(sde.sigma_max))
  if levels is None:
    levels = (top,)
  try:
    lv = _fp32([float(v) for v in levels])
  except TypeError:
    raise ValueError(f'levels must be a sequence of noise levels, got {levels!r}') from None
  if lv.ndim != 1 or lv.size == 0:
    raise ValueError(f'levels must hold at least one noise level, got {levels!r}')
  if not bool(np.isfinite(lv).all()) or not bool((lv > e).all()) or not bool((lv <= top).all()):
    raise ValueError(f'levels must lie in (sigma_min, sigma_max] = ({e!r}, {top!r}], got {[float(v) for v in lv]!r}')
  if not bool((np.diff(lv) < 0.).all()):
    raise ValueError(f'levels must be strictly decreasing in fp32, got {[float(v) for v in lv]!r}')
  c_in, _, c_skip, c_out, c_noise = ct_coefficients(lv, sde.sigma_data, e)
  c_z = np.concatenate([np.sqrt(lv[1:] * lv[1:] - e * e), [0.]])
  rows = np.stack([c_skip, c_out, c_z, np.concatenate([c_in[1:], [0.]]), c_noise], axis=1)
  lo, hi = (-1., 1.) if clip else (-_INF, _INF)
  return ConsistencySchedule(levels=lv, rows=rows, c_in_first=float(c_in[0]), lo=lo, hi=hi, sigma_min=e,
                             sigma_data=float(sde.sigma_data), nfe=int(lv.size))


def _step(lib, x, F, z, row, lo, hi, x0_out, x_out, xin_out):
  """One launch of stk_ct_step_f32 on contiguous fp32 device tensors.  row: (cs, co, c_z, c_in_next, ...)."""
  cs, co, c_z, c_next = (float(v) for v in row[:4])
  with stk_lib.device_guard(x.device):
    lib.ct_step_f32(x.data_ptr(), F.data_ptr(), _ptr(z), cs, co, float(lo), float(hi), c_z, c_next, _ptr(x0_out), _ptr(x_out),
                    _ptr(xin_out), x.numel(), stk_lib.stream_ptr(x.device))


def consistency_sample(model_fn, schedule, x, noise_fn=None):
  """The loop: `x` (a contiguous fp32 device tensor of the run's shape; its values are not read) receives
  levels[0] noise_fn(x), is advanced IN PLACE through the levels and returned as the last x0.  model_fn: any ``F(x_in,
  c_noise)`` with c_noise a [B] fp32 tensor (``models.utils.get_edm_model_fn``).  noise_fn(x) -> a standard normal tensor like
  x (``torch.randn_like`` where None), called ``schedule.nfe`` times.  ``schedule.nfe`` evaluations and as many launches."""
  lib = _library()
  mutils.check_inplace_state(x, lib)
  draw = torch.randn_like if noise_fn is None else noise_fn
  n, B = schedule.nfe, x.shape[0]
  z = draw(x)
  mutils.check_inplace_state(z, lib, why='the kernels read it in place')
  torch.mul(z, float(schedule.levels[0]), out=x)
  xin = x * float(schedule.c_in_first)
  cond = mutils.level_conditioning(schedule.rows[:, 4], B, x.device)       # the conditioning vectors of all evaluations
  for j in range(n):
    F = mutils.checked_score(model_fn, xin, cond[j], lib)
    if j == n - 1:
      _step(lib, x, F, None, schedule.rows[j], schedule.lo, schedule.hi, x, None, None)
      break
    z = draw(x)
    mutils.check_inplace_state(z, lib, why='the kernels read it in place')
    _step(lib, x, F, z, schedule.rows[j], schedule.lo, schedule.hi, None, x, xin)
  return x


def get_consistency_sampler(config, sde, shape, inverse_scaler, levels=None, clip=True, noise_fn=None, device='cuda',
                            precision='fp32'):
  """``consistency_sampler(model) -> (samples, nfe)`` with ``nfe = len(levels)``: x = levels[0] z, then per level one network
  evaluation and x0 = f(x; level), renoised to the next level by x = x0 + sqrt(next^2 - sigma_min^2) z.  levels None: the
  single level sigma_max.  precision='fp16': every network evaluation runs in the engine's fp16 mode.  ValueError for an `sde`
  other than sde_lib.EDM, for a config the family refuses (models.utils.check_edm_config) and for invalid levels;
  NotImplementedError for a library without include/stk_consistency.h -- all when the sampler is built."""
  lib = _library()
  schedule = consistency_schedule(sde, levels, clip=clip)
  mutils.check_edm_config(config)
  mutils.check_precision(precision)

  def consistency_sampler(model):
    with mutils.sampling_run(model, precision):
      model_fn = mutils.get_edm_model_fn(config, model, train=False)
      x = torch.empty(tuple(shape), dtype=torch.float32, device=device)
      _backend.check(x, lib)
      x = consistency_sample(model_fn, schedule, x, noise_fn=noise_fn)
      return inverse_scaler(x), schedule.nfe

  return consistency_sampler


def sampling_options(config):
  """(levels, clip) of ``config.sampling.ct_levels / ct_clip``: None (the single level sigma_max) and True where a key is
  absent."""
  read = lambda key, default: mutils.config_option(config, 'sampling', key, default)
  return read('ct_levels', None), bool(read('ct_clip', True))


# ---- what the training loss reads (losses.get_consistency_loss_fn) ---------------------------------------------------------------
def training_options(config):
  """(p_mean, p_std, s0, s1, huber_c) of ``config.training.ct_p_mean / ct_p_std / ct_s0 / ct_s1 / ct_huber_c`` (-1.1, 2.0, 10,
  1280 and 0.00054 where absent); ValueError naming the key for ct_s0 or ct_s1 non-positive or not an integer, ct_s0 > ct_s1,
  ct_p_std <= 0, ct_huber_c <= 0, anything NaN."""
  read = lambda key, default: mutils.config_option(config, 'training', key, default)
  p_mean, p_std, huber_c = float(read('ct_p_mean', -1.1)), float(read('ct_p_std', 2.0)), float(read('ct_huber_c', 0.00054))
  s0, s1 = read('ct_s0', 10), read('ct_s1', 1280)
  for key, v in (('ct_s0', s0), ('ct_s1', s1)):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v <= 0:
      raise ValueError(f'config.training.{key} must be a positive integer, got {v!r}')
  if s0 > s1:
    raise ValueError(f'config.training.ct_s0 = {s0!r} must not exceed config.training.ct_s1 = {s1!r}')
  if not math.isfinite(p_mean):
    raise ValueError(f'config.training.ct_p_mean must be finite, got {p_mean!r}')
  if not (p_std > 0 and math.isfinite(p_std)):
    raise ValueError(f'config.training.ct_p_std must be positive and finite, got {p_std!r}')
  if not (huber_c > 0 and math.isfinite(huber_c)):
    raise ValueError(f'config.training.ct_huber_c must be positive and finite, got {huber_c!r}')
  return p_mean, p_std, int(s0), int(s1), huber_c
