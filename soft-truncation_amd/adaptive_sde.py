"""The adaptive-step SDE sampler of Jolicoeur-Martineau et al., "Gotta Go Fast When Generating Data with Score-Based Models"
(2021): a stochastic sampler whose step size is chosen per sample from an error estimate, where ``sampling.get_pc_sampler``
walks a fixed ladder of one to two thousand steps.

Every SDE of ``sde_lib`` has a linear drift: dx = c(t) x dt + g(t) dw.  Every sample b carries its own time t_b and step
h_b > 0, fp32 vectors on the device.  One iteration, with t' = t - h:

  z   ~ N(0, I)                                        one torch.randn_like(x) per iteration, accepted or not
  s1  = score(x, t)
  x1  = (1 - h c(t)) x + h g(t)^2 s1 + sqrt(h) g(t) z                    Euler-Maruyama
  s2  = score(x1, t')
  xt  = x - h c(t') x1 + h g(t')^2 s2 + sqrt(h) g(t') z                   the drift evaluated at (x1, t')
  x2  = (x1 + xt) / 2                                                    improved Euler
  d   = max(atol, rtol max(|x1|, |x1_prev|))
  E_b = sqrt(mean over the sample of ((x1 - x2) / d)^2)
  accepted (E_b <= 1):  x <- x2, x1_prev <- x1, t <- t'                  rejected: x, x1_prev, t unchanged
  h   <- min(t_new - eps, safety h E_b^-exponent)

A step with h >= t - eps lands on eps exactly; a sample at eps is finished (h = 0, its x frozen) and rides along until
every sample is.  A non-finite E_b is a rejection that halves the step (times `safety`).  The score of a rejected step is
evaluated again on the next attempt: re-using it is not implemented.

Per iteration the state is touched by three launches (include/stk_adaptive.h, csrc/adaptive.hip): ``stk_sde_stage_f32``
(x1), ``stk_sde_heun_error_f32`` (x2 and the partial sums of the error norm) and ``stk_sde_commit_f32`` (E_b, the decision,
the new t_b and h_b, and the per-sample select).  The coefficient rows are built on the device from ``sde_coefficients`` with
a few [B]-sized torch operations; the one value that reaches the host per iteration is the all-finished flag.

The network evaluations follow the engine's conventions as ``get_pc_sampler`` does: ``torch.no_grad``, weights prepared once
per run (``models.utils.frozen_weights``), ``precision`` ('fp16' applies to the network only: the three passes are always
fp32).  Everything runs on the device: host tensors raise the package's device error, there is no CPU path; a library
without include/stk_adaptive.h is refused when the sampler is built.  Sample quality (FID) at any tolerance is unmeasured.
"""
import math

import numpy as np
import torch

from . import sde_lib
from .engine import lib as stk_lib
from .models import utils as mutils

RTOL = 0.01
ATOL_CENTERED, ATOL_UNCENTERED = 0.0078, 0.0039          # 2 / 256 for data in [-1, 1], 1 / 256 for data in [0, 1]
H_INIT, SAFETY, EXPONENT = 0.01, 0.9, 0.9
MAX_ITERS = 10000


def _library():
  return mutils.require('has_adaptive', 'stk_adaptive.h', 'stk_sde_stage_f32, stk_sde_heun_error_f32 and stk_sde_commit_f32',
                        'the adaptive SDE sampler needs')


def default_atol(config):
  return ATOL_CENTERED if config.data.centered else ATOL_UNCENTERED


def sde_coefficients(sde, t):
  """(c(t), g(t)) of the forward SDE dx = c(t) x dt + g(t) dw at the times `t` [B], as [B] vectors of t's dtype on t's
  device: drift and diffusion of ``sde.sde`` on a tensor of ones.  float64 times give float64 coefficients.  VESDE's own
  ``sde`` rounds the constant sqrt(2 log(sigma_max / sigma_min)) to fp32 whatever the dtype of t, so its g is restated here
  from the SDE's own sigma(t)."""
  if isinstance(sde, sde_lib.VESDE):
    c, g = torch.zeros_like(t), sde._sigma(t) * math.sqrt(2. * sde._log_ratio())
  else:
    drift, g = sde.sde(torch.ones((t.shape[0], 1, 1, 1), dtype=t.dtype, device=t.device), t)
    c = drift.reshape(-1)
  g = g.reshape(-1)
  if c.dtype != t.dtype or g.dtype != t.dtype:
    raise TypeError(f'{type(sde).__name__}.sde does not carry {t.dtype} through ({c.dtype}, {g.dtype})')
  return c, g


def stage_rows(sde, t, h):
  """The [B, 4] coefficient rows of the Euler-Maruyama stage at (t, h): (1 - h c, 0, h g^2, sqrt(h) g)."""
  c, g = sde_coefficients(sde, t)
  return torch.stack([1. - h * c, torch.zeros_like(h), h * g * g, torch.sqrt(h) * g], dim=1).contiguous()


def heun_rows(sde, t_next, h):
  """The [B, 4] coefficient rows of the second stage, the drift at (x1, t'): (1, -h c', h g'^2, sqrt(h) g')."""
  c, g = sde_coefficients(sde, t_next)
  return torch.stack([torch.ones_like(h), -(h * c), h * g * g, torch.sqrt(h) * g], dim=1).contiguous()


def next_time(t, h, eps):
  """t' = t - h; a step that reaches t - eps lands on eps exactly (the rule of stk_sde_commit_f32, on the same fp32 values)."""
  return torch.where(h >= t - eps, torch.full_like(t, eps), t - h)


def _check_options(rtol, atol, h_init, safety, exponent, eps, T, max_iters):
  if not (rtol >= 0. and atol >= 0. and rtol + atol > 0.):
    raise ValueError(f'rtol and atol must be non-negative and not both zero, got rtol = {rtol!r}, atol = {atol!r}')
  if not h_init > 0.:
    raise ValueError(f'h_init must be positive, got {h_init!r}')
  if not safety > 0.:
    raise ValueError(f'safety must be positive, got {safety!r}')
  if not exponent >= 0.:
    raise ValueError(f'exponent must be non-negative, got {exponent!r}')
  if not 0. < eps < T:
    raise ValueError(f'the run goes from T down to eps with 0 < eps < T, got T = {T!r}, eps = {eps!r}')
  if int(max_iters) != max_iters or max_iters < 1:
    raise ValueError(f'max_iters must be a positive integer, got {max_iters!r}')


def adaptive_sample(score_fn, x, sde, rtol=RTOL, atol=ATOL_CENTERED, h_init=H_INIT, safety=SAFETY, exponent=EXPONENT, eps=1e-3,
                    max_iters=MAX_ITERS):
  """The loop: `x` (a contiguous fp32 device tensor drawn from the prior at ``sde.T``) is advanced IN PLACE to `eps`, every
  sample at its own pace.  Returns ``(x, iterations, info)``: `iterations` counts loop iterations (two evaluations of
  `score_fn` each), ``info['accepted']`` and ``info['rejected']`` are the per-sample step counts, [B] int64 on the device
  (their sum is below `iterations` for a sample that finished early), ``info['E']`` the error norms of the last iteration.
  RuntimeError when some sample has not reached `eps` after `max_iters` iterations."""
  lib = _library()
  mutils.check_inplace_state(x, lib)
  eps, T = float(np.float32(eps)), float(np.float32(sde.T))
  _check_options(rtol, atol, h_init, safety, exponent, eps, T, max_iters)
  B, dev = x.shape[0], x.device
  n = x.numel() // B
  ws_bytes = lib.sde_ws_bytes(B, n)
  if ws_bytes < 0:
    raise ValueError(f'a state of {B} samples of {n} elements is not supported by include/stk_adaptive.h (rc={ws_bytes})')
  ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
  t = torch.full((B,), T, dtype=torch.float32, device=dev)
  h = torch.minimum(torch.full_like(t, h_init), t - eps)
  t_new, h_new = torch.empty_like(t), torch.empty_like(h)
  E, accept = torch.empty_like(t), torch.empty(B, dtype=torch.int32, device=dev)
  accepted, rejected = (torch.zeros(B, dtype=torch.int64, device=dev) for _ in range(2))
  x1, x2, x1_prev = torch.empty_like(x), torch.empty_like(x), x.clone()
  stream = stk_lib.stream_ptr(dev)
  iterations = 0
  while not bool((t <= eps).all()):                     # the one value read back per iteration
    if iterations >= max_iters:
      raise RuntimeError(f'the adaptive sampler has not reached eps = {eps!r} after max_iters = {max_iters} iterations')
    z = torch.randn_like(x)
    s1 = mutils.checked_score(score_fn, x, t, lib)
    t_next = next_time(t, h, eps)
    with stk_lib.device_guard(dev):
      lib.sde_stage_f32(x.data_ptr(), None, s1.data_ptr(), z.data_ptr(), stage_rows(sde, t, h).data_ptr(), x1.data_ptr(), B, n,
                        stream)
    s2 = mutils.checked_score(score_fn, x1, t_next, lib)
    with stk_lib.device_guard(dev):
      lib.sde_heun_error_f32(x.data_ptr(), x1.data_ptr(), x1_prev.data_ptr(), s2.data_ptr(), z.data_ptr(),
                             heun_rows(sde, t_next, h).data_ptr(), atol, rtol, x2.data_ptr(), ws.data_ptr(), ws_bytes, B, n,
                             stream)
      lib.sde_commit_f32(x.data_ptr(), x1_prev.data_ptr(), x2.data_ptr(), x1.data_ptr(), t.data_ptr(), h.data_ptr(), eps,
                         safety, exponent, ws.data_ptr(), ws_bytes, t_new.data_ptr(), h_new.data_ptr(), E.data_ptr(),
                         accept.data_ptr(), B, n, stream)
    accepted += accept
    rejected += (t > eps) & (accept == 0)
    t, t_new, h, h_new = t_new, t, h_new, h
    iterations += 1
  return x, iterations, dict(accepted=accepted, rejected=rejected, E=E, t=t)


def get_adaptive_sampler(config, sde, shape, inverse_scaler, rtol=RTOL, atol=None, h_init=H_INIT, safety=SAFETY,
                         exponent=EXPONENT, denoise=True, eps=1e-3, device='cuda', precision='fp32', max_iters=MAX_ITERS):
  """``adaptive_sampler(model) -> (samples, nfe)`` with ``nfe = 2 iterations (+ 1 with denoise)``: the adaptive-step sampler
  from ``sde.T`` down to `eps`.  atol=None: 0.0078 for centered data, 0.0039 otherwise.  denoise: the noise-free last step of
  ``get_pc_sampler`` (one more evaluation).  precision='fp16': every network evaluation runs in the engine's fp16 mode
  (models.utils.precision)."""
  from . import sampling                 # sampling imports this module
  lib = _library()
  atol = default_atol(config) if atol is None else atol
  _check_options(rtol, atol, h_init, safety, exponent, float(np.float32(eps)), float(np.float32(sde.T)), max_iters)
  mutils.check_precision(precision)
  denoise_update_fn = sampling._denoiser(config, sde, probability_flow=True)

  def adaptive_sampler(model):
    with mutils.sampling_run(model, precision):
      score_fn, x = mutils.score_and_prior(config, sde, model, shape, device, lib)
      x, iterations, _ = adaptive_sample(score_fn, x, sde, rtol=rtol, atol=atol, h_init=h_init, safety=safety,
                                         exponent=exponent, eps=eps, max_iters=max_iters)
      if denoise:
        x = denoise_update_fn(model, x)
      return inverse_scaler(x), 2 * iterations + (1 if denoise else 0)

  return adaptive_sampler


def sampling_options(config):
  """(rtol, atol, h_init, safety, exponent) of ``config.sampling.adaptive_rtol / adaptive_atol / adaptive_h_init /
  adaptive_safety / adaptive_exponent``: the paper's 0.01, 0.0078 (centered data) or 0.0039, 0.01, 0.9 and 0.9 where a key is
  absent (the reference's configs have none)."""
  read = lambda key, default: mutils.config_option(config, 'sampling', key, default)
  return (read('adaptive_rtol', RTOL), read('adaptive_atol', default_atol(config)), read('adaptive_h_init', H_INIT),
          read('adaptive_safety', SAFETY), read('adaptive_exponent', EXPONENT))
