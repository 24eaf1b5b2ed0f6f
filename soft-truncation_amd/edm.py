"""The EDM sampler: the rho-schedule and the (optionally stochastic) second-order Heun loop of Karras et al., "Elucidating
the Design Space of Diffusion-Based Generative Models", 2022, Algorithm 2, on ``sde_lib.EDM``.  Eighteen steps are 35
network evaluations, where ``sampling.get_pc_sampler`` takes one to two thousand.

With the noise levels sigma_0 = sigma_max > ... > sigma_{steps-1} = sigma_min, sigma_steps = 0 and the denoiser
D(x; sigma) = c_skip x + c_out F(c_in x; c_noise) around the network F (include/stk_edm.h), one step from t_i = sigma_i is

  t^   = t_i + gamma_i t_i;  x^ = x + s_noise sqrt(t^^2 - t_i^2) eps        only where gamma_i > 0 (the churn)
  d    = (x^ - D(x^; t^)) / t^;  x' = x^ + (t_{i+1} - t^) d                   the Euler stage
  d'   = (x' - D(x'; t_{i+1})) / t_{i+1};  x = x^ + (t_{i+1} - t^) (d + d') / 2   the correction, unless t_{i+1} = 0

``edm_schedule`` turns an SDE and a step count into the host coefficients of every launch, in float64 from times rounded to
fp32 first (the network sees exactly the level the coefficients were computed at);  ``edm_sample`` is the loop over any
``F(x_in, c_noise)``: per step an optional ``stk_edm_churn_f32``, one evaluation, one ``stk_edm_step_f32`` and, unless
t_{i+1} = 0, a second evaluation and a second ``stk_edm_step_f32`` (include/stk_edm.h, csrc/edm.hip).  Each launch writes the
input c_in x of the evaluation that follows it, so no separate scaling pass runs in front of the network; one churn launch
without noise writes the input of the first evaluation.  The state, the Euler point, the slope and the network input live in
four buffers allocated once per run.  ``get_edm_sampler`` binds both to a model the way ``dpm_solver.get_dpm_sampler`` does.

With ``s_churn = 0`` the only random draw of a whole run is the single ``sde.prior_sampling(shape)``; with churn, one
``torch.randn_like`` per churned step follows it, in step order: that is part of the interface.  The network evaluations
follow the engine's conventions: ``torch.no_grad``, weights prepared once per run, ``precision`` ('fp16' applies to the
network only: the updates are always fp32).  Everything runs on the device: host tensors raise the package's device error,
there is no CPU path; a library without include/stk_edm.h is refused when the sampler is built.  Sample quality (FID) at any
step count is unmeasured: no checkpoint trained under this formulation exists.
"""
import math

import numpy as np
import torch

from . import sde_lib
from .engine import lib as stk_lib
from .models import utils as mutils
from .op import _backend

GAMMA_MAX = math.sqrt(2.) - 1.
_INF = float('inf')


def _library():
  return mutils.require('has_edm', 'stk_edm.h', 'stk_edm_churn_f32 and stk_edm_step_f32', 'the EDM sampler needs')


_fp32, _ptr = mutils.fp32_levels, mutils.optional_ptr


def denoiser_coefficients(sigma, sigma_data):
  """(c_in, c_skip, c_out, c_noise) at the float64 levels `sigma` (any array-like), float64 numpy, in the operation order of
  include/stk_edm.h; c_in = 0 and c_noise = -inf at sigma = 0 (never used there)."""
  S, d = np.asarray(sigma, dtype=np.float64), float(sigma_data)
  v = S * S + d * d
  q = np.sqrt(v)
  with np.errstate(divide='ignore'):
    c_noise = np.log(S) / 4.
  return np.where(S > 0., 1. / q, 0.), (d * d) / v, (S * d) / q, c_noise


class EdmSchedule:
  """The host record of one run, float64 numpy throughout, every time fp32-representable.  ``sigmas`` [steps + 1] from
  sigma_max down to sigma_min, then 0;  ``gamma``, ``t_hat``, ``c_eps``, ``c_in_hat`` [steps] (the churn);  ``euler``
  [steps, 6] and ``correct`` [steps - 1, 6], the rows ``(cs, co, t, h, c_next, c_noise)`` of the two stages: the first five
  are the scalars of stk_edm_step_f32, c_noise conditions the evaluation in front of the launch;  ``nfe`` = 2 steps - 1;
  ``launches``: the kernel launches of a run."""

  def __init__(self, **fields):
    self.__dict__.update(fields)

  def __repr__(self):
    return (f'EdmSchedule(steps={self.steps}, rho={self.rho!r}, s_churn={self.s_churn!r}, sigma_max={float(self.sigmas[0])!r}, '
            f'sigma_min={float(self.sigmas[-2])!r}, nfe={self.nfe})')


def edm_schedule(sde, steps, rho=7, s_churn=0, s_tmin=0, s_tmax=_INF, s_noise=1):
  """The noise levels and the per-launch coefficients of the EDM sampler (module docstring) for `sde`, as an
  :class:`EdmSchedule`:  sigma_i = (sigma_max^(1/rho) + i / (steps - 1) (sigma_min^(1/rho) - sigma_max^(1/rho)))^rho, rounded
  to fp32;  gamma_i = min(s_churn / steps, sqrt(2) - 1) where s_tmin <= sigma_i <= s_tmax, else 0;
  t^_i = fp32(sigma_i + gamma_i sigma_i);  c_eps_i = s_noise sqrt(t^_i^2 - sigma_i^2).  ValueError naming the option: steps
  not an integer >= 2, rho not positive, s_churn or s_tmin or s_noise negative, s_tmax below s_tmin, anything NaN."""
  if not isinstance(sde, sde_lib.EDM):
    raise ValueError(f'the EDM sampler needs sde_lib.EDM (config.training.sde = \'edm\'), got {type(sde).__name__}')
  if isinstance(steps, bool) or int(steps) != steps or steps < 2:
    raise ValueError(f'steps must be an integer >= 2 (sigma_max and sigma_min are both on the grid), got {steps!r}')
  steps = int(steps)
  rho, s_churn, s_tmin, s_tmax, s_noise = (float(v) for v in (rho, s_churn, s_tmin, s_tmax, s_noise))
  if not (rho > 0. and math.isfinite(rho)):
    raise ValueError(f'rho must be positive and finite, got {rho!r}')
  if not (s_churn >= 0. and math.isfinite(s_churn)):
    raise ValueError(f's_churn must be non-negative and finite, got {s_churn!r}')
  if not s_tmin >= 0.:
    raise ValueError(f's_tmin must be non-negative, got {s_tmin!r}')
  if not s_tmax >= s_tmin:
    raise ValueError(f's_tmax must not lie below s_tmin = {s_tmin!r}, got {s_tmax!r}')
  if not (s_noise >= 0. and math.isfinite(s_noise)):
    raise ValueError(f's_noise must be non-negative and finite, got {s_noise!r}')
  hi, lo = float(_fp32(sde.sigma_max)), float(_fp32(sde.sigma_min))
  ramp = np.arange(steps, dtype=np.float64) / (steps - 1)
  sig = _fp32((hi ** (1. / rho) + ramp * (lo ** (1. / rho) - hi ** (1. / rho))) ** rho)
  sig[0], sig[-1] = hi, lo
  sigmas = np.concatenate([sig, [0.]])
  if not bool((np.diff(sigmas) < 0.).all()):
    raise ValueError(f'steps = {steps}: two noise levels coincide in fp32')
  gamma = np.where((sig >= s_tmin) & (sig <= s_tmax), min(s_churn / steps, GAMMA_MAX), 0.)
  t_hat = _fp32(sig + gamma * sig)
  gamma = np.where(t_hat > sig, gamma, 0.)                # a churn that fp32 rounds away is no churn
  c_eps = s_noise * np.sqrt(t_hat * t_hat - sig * sig)
  s = sde.sigma_data
  cin_h, cs_h, co_h, cn_h = denoiser_coefficients(t_hat, s)
  cin_n, cs_n, co_n, cn_n = denoiser_coefficients(sigmas[1:], s)
  h = sigmas[1:] - t_hat
  euler = np.stack([cs_h, co_h, t_hat, h, cin_n, cn_h], axis=1)
  correct = np.stack([cs_n[:-1], co_n[:-1], sigmas[1:-1], h[:-1], cin_h[1:], cn_n[:-1]], axis=1)
  churned = gamma > 0.
  launches = 1 + int(churned[1:].sum()) + steps + (steps - 1)
  return EdmSchedule(steps=steps, rho=rho, s_churn=s_churn, s_tmin=s_tmin, s_tmax=s_tmax, s_noise=s_noise, sigma_data=float(s),
                     sigmas=sigmas, gamma=gamma, t_hat=t_hat, c_eps=c_eps, c_in_hat=cin_h, euler=euler, correct=correct,
                     nfe=2 * steps - 1, launches=launches)


def _churn(lib, x, eps, c_eps, c_in_hat, x_hat_out, xin_out):
  """One launch of stk_edm_churn_f32 on contiguous fp32 device tensors; eps None: no noise."""
  with stk_lib.device_guard(x.device):
    lib.edm_churn_f32(x.data_ptr(), _ptr(eps), float(c_eps), float(c_in_hat), _ptr(x_hat_out), xin_out.data_ptr(), x.numel(),
                      stk_lib.stream_ptr(x.device))


def _step(lib, xb, xe, F, d_prev, row, x_out, d_out, xin_out):
  """One launch of stk_edm_step_f32 on contiguous fp32 device tensors.  row: (cs, co, t, h, c_next, ...)."""
  cs, co, t, h, c_next = (float(v) for v in row[:5])
  with stk_lib.device_guard(xb.device):
    lib.edm_step_f32(xb.data_ptr(), xe.data_ptr(), F.data_ptr(), _ptr(d_prev), cs, co, t, h, c_next, x_out.data_ptr(), _ptr(d_out),
                     _ptr(xin_out), xb.numel(), stk_lib.stream_ptr(xb.device))


def edm_sample(model_fn, schedule, x, noise_fn=None):
  """The loop: `x` (a contiguous fp32 device tensor drawn from the prior at the schedule's sigma_max) is advanced IN PLACE
  to noise level 0 and returned.  model_fn: any ``F(x_in, c_noise)`` with c_noise a [B] fp32 tensor (the raw network under
  the EDM conditioning: ``models.utils.get_edm_model_fn``).  noise_fn(x) -> eps of a churned step (``torch.randn_like``
  where None).  ``schedule.nfe`` evaluations and ``schedule.launches`` launches (module docstring)."""
  lib = _library()
  mutils.check_inplace_state(x, lib)
  draw = torch.randn_like if noise_fn is None else noise_fn
  steps, B = schedule.steps, x.shape[0]
  x1, d, xin = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
  # the conditioning vectors of all evaluations: row 2 i for t^_i, row 2 i + 1 for t_{i+1}
  levels = np.stack([schedule.euler[:, 5], np.concatenate([schedule.correct[:, 5], [0.]])], axis=1).reshape(-1)[:schedule.nfe]
  cond = mutils.level_conditioning(levels, B, x.device)
  for i in range(steps):
    if schedule.gamma[i] > 0.:
      eps = draw(x)
      mutils.check_inplace_state(eps, lib, why='the kernels read it in place')
      _churn(lib, x, eps, schedule.c_eps[i], schedule.c_in_hat[i], x, xin)
    elif i == 0:
      _churn(lib, x, None, 0., schedule.c_in_hat[0], None, xin)
    F = mutils.checked_score(model_fn, xin, cond[2 * i], lib)
    if i == steps - 1:                                    # t_{i+1} = 0: the Euler point is the result
      _step(lib, x, x, F, None, schedule.euler[i], x, None, None)
      break
    _step(lib, x, x, F, None, schedule.euler[i], x1, d, xin)
    F = mutils.checked_score(model_fn, xin, cond[2 * i + 1], lib)
    feeds_next = not schedule.gamma[i + 1] > 0.           # a churned step writes its own network input
    _step(lib, x, x1, F, d, schedule.correct[i], x, None, xin if feeds_next else None)
  return x


def get_edm_sampler(config, sde, shape, inverse_scaler, steps=18, rho=7, s_churn=0, s_tmin=0, s_tmax=_INF, s_noise=1,
                    device='cuda', precision='fp32'):
  """``edm_sampler(model) -> (samples, nfe)`` with ``nfe = 2 steps - 1``: the Heun sampler of EDM over `steps` noise levels
  from ``sde.sigma_max`` down to ``sde.sigma_min`` and on to 0.  precision='fp16': every network evaluation runs in the
  engine's fp16 mode (models.utils.precision).  ValueError for an `sde` other than sde_lib.EDM, for a config the family
  refuses (models.utils.check_edm_config) and for invalid options; NotImplementedError for a library without
  include/stk_edm.h -- all when the sampler is built."""
  lib = _library()
  schedule = edm_schedule(sde, steps, rho=rho, s_churn=s_churn, s_tmin=s_tmin, s_tmax=s_tmax, s_noise=s_noise)
  mutils.check_edm_config(config)
  mutils.check_precision(precision)

  def edm_sampler(model):
    with mutils.sampling_run(model, precision):
      model_fn = mutils.get_edm_model_fn(config, model, train=False)
      x = sde.prior_sampling(shape).to(device).contiguous()
      _backend.check(x, lib)
      x = edm_sample(model_fn, schedule, x)
      return inverse_scaler(x), schedule.nfe

  return edm_sampler


def sampling_options(config):
  """(steps, rho, s_churn, s_tmin, s_tmax, s_noise) of ``config.sampling.edm_steps / edm_rho / edm_s_churn / edm_s_tmin /
  edm_s_tmax / edm_s_noise``: 18, 7, 0, 0, inf and 1 where a key is absent."""
  read = lambda key, default: mutils.config_option(config, 'sampling', key, default)
  return (read('edm_steps', 18), read('edm_rho', 7), read('edm_s_churn', 0), read('edm_s_tmin', 0), read('edm_s_tmax', _INF),
          read('edm_s_noise', 1))
