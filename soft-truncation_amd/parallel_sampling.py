"""A parallel-in-time sampler: Picard iteration over a sliding window of grid points (Shih et al., "Parallel Sampling of
Diffusion Models", 2023, ParaDiGMS).  Every other sampler here is sequential in time -- one network evaluation, a small update,
the next evaluation -- and at small batch most of the card idles through it.  Here a window of W consecutive grid points is
evaluated as ONE batch of W B samples, each slot at its own time; the W step increments are prefix-summed along time; and the
window slides forward past every slot that has stopped changing.  It computes the discretised trajectory of the sequential
loop, exactly so at tolerance 0, in fewer sequential evaluations of a larger batch.

The step map from grid point i to i + 1 is the generalised DDIM step, DDIM at eta = 0 and ancestral sampling at eta = 1, with
alpha, sigma of ``dpm_solver.dpm_schedule`` (float64, from times rounded to fp32 first):

  tau_i^2 = eta^2 sigma_{i+1}^2 (1 - (alpha_i sigma_{i+1})^2 / (alpha_{i+1} sigma_i)^2)
  a_i = alpha_{i+1} / alpha_i
  b_i = alpha_{i+1} sigma_i^2 / alpha_i - sigma_i sqrt(sigma_{i+1}^2 - tau_i^2)
  g_i = tau_i
  x_{i+1} = a_i x_i + b_i score(x_i, t_i) + g_i z_i

One iteration with the window at base i0 and p = min(W, N - i0) live slots, on the state X[W + 1, B, n] (slot-major, X[0]
committed) -- three launches of include/stk_parallel.h (csrc/parallel.hip) around one network evaluation:

  1. S = score_fn(X[:W] as [W B, C, H, W], t), t the slots' times, each repeated B times; slots j >= p are padding (evaluated
     at the last live time and ignored), so the batch is ALWAYS W B and the engine plans one extra program;
  2. ``stk_picard_scan_f32``: in fp32, in the order written, D_j = ((a_j - 1) X[j] + b_j S[j]) + g_j Z[(i0 + j) mod W],
     Y[0] = X[0], Y[j+1] = Y[j] + D_j strictly in sequence, err[b][j] = sum (Y[j] - X[j])^2 in float64, Y overwrites X[1..p];
  3. ``stk_picard_stride``: slot j is converged iff err[b][j] <= tol^2 sigma_{i0+j}^2 n for every b (a NaN is not);
     stride = 1 + the leading converged slots of j = 1 .. p - 1, so 1 <= stride <= p;
  4. ``stk_picard_slide_f32``: X[j] <- X[min(j + stride, p)]; the slots that enter start from the last point; i0 += stride.

The stride is the ONE host read of an iteration.  The tolerance scale sigma_i, the marginal std at the slot, is this
package's choice: the paper scales by the step's noise variance, which vanishes at eta = 0.  With window = 1 the loop IS the
sequential sampler, and at tol = 0 any window reproduces it bit for bit wherever the score function gives a sample the same
bits at either batch size (slots are accepted only when they have stopped changing in every bit).

The random draws: the prior, then the noise of step i as the (i + 1)-th ``torch.randn(B, C, H, W)`` on the device, drawn when
step i enters the window and kept in slot i mod W of a ring.  A run consumes the generator exactly as its window = 1 run does:
N draws for eta > 0, none for eta = 0.  The network evaluations follow the engine's conventions (``torch.no_grad``, weights
prepared once, 'fp16' applies to the network only).  Everything runs on the device; a library without include/stk_parallel.h
is refused when the sampler is built.  Beside the state of the sequential loop a run holds X, the ring and the window's
scores -- (3 W + 1) B n floats, (2 W + 1) at eta = 0 -- and the engine's arena of a batch of W B.

What this gains depends on how fast the iteration converges on a trained score, which is unmeasured: no checkpoint exists.
Sample quality at any tolerance is unmeasured too.  Not covered: correctors, second-order increments, per-sample strides.
"""
import math

import numpy as np
import torch

from . import dpm_solver
from .engine import lib as stk_lib
from .models import utils as mutils

MAX_WINDOW = 256                 # include/stk_parallel.h


def _library():
  mutils.require('has_solver', 'stk_solver.h', 'stk_dpm_update_f32', 'the parallel sampler needs')
  return mutils.require('has_parallel', 'stk_parallel.h', 'stk_picard_scan_f32, stk_picard_stride and stk_picard_slide_f32',
                        'the parallel sampler needs')


class PicardSchedule:
  """The host record of one run, float64 numpy throughout.  ``times`` [steps + 1] from T down to eps, every entry
  fp32-representable; ``alpha``, ``sigma`` there; ``coef`` [steps, 3], the rows (a_i - 1, b_i, g_i) of the module docstring
  (the difference formed in float64); ``thr_unit`` [steps], sigma_i^2: the threshold of slot i per unit of tol^2 n;
  ``final`` the row of ``dpm_solver.DpmSchedule`` that turns the evaluation at eps into the data prediction there."""

  def __init__(self, **fields):
    self.__dict__.update(fields)

  def __repr__(self):
    return (f'PicardSchedule({self.sde_name}, steps={self.steps}, eta={self.eta!r}, skip={self.skip!r}, '
            f'T={float(self.times[0])!r}, eps={float(self.times[-1])!r})')


def _check_eta(eta):
  try:
    value = float(eta)
  except (TypeError, ValueError):
    raise ValueError(f'parallel_eta must be a number in [0, 1], got {eta!r}') from None
  if not 0. <= value <= 1.:
    raise ValueError(f'parallel_eta must be a number in [0, 1], got {eta!r}')
  return value


def _check_steps(steps):
  try:
    ok = not isinstance(steps, bool) and int(steps) == steps and steps >= 1
  except (TypeError, ValueError, OverflowError):
    ok = False
  if not ok:
    raise ValueError(f'parallel_steps must be a positive integer, got {steps!r}')
  return int(steps)


def _check_window(window):
  if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or not 1 <= window <= MAX_WINDOW:
    raise ValueError(f'parallel_window must be an integer in [1, {MAX_WINDOW}], got {window!r}')
  return int(window)


def _check_tol(tol):
  try:
    value = float(tol)
  except (TypeError, ValueError):
    raise ValueError(f'parallel_tol must be a number >= 0, got {tol!r}') from None
  if not value >= 0.:                                  # NaN included
    raise ValueError(f'parallel_tol must be a number >= 0, got {tol!r}')
  return value


def picard_schedule(sde, steps, eta=0., skip='time', eps=None):
  """The time grid and the per-step coefficients (module docstring) for `sde`, as a :class:`PicardSchedule`.  The grid, alpha
  and sigma are ``dpm_solver.dpm_schedule``'s (VP, sub-VP, VE, reciprocal VE and EDM; `skip` and `eps` as there)."""
  steps, eta = _check_steps(steps), _check_eta(eta)
  dpm = dpm_solver.dpm_schedule(sde, steps, order=1, skip=skip, eps=eps)
  al, sg = dpm.alpha, dpm.sigma
  tau2 = eta ** 2 * sg[1:] ** 2 * (1. - (al[:-1] * sg[1:]) ** 2 / (al[1:] * sg[:-1]) ** 2)
  a = al[1:] / al[:-1]
  b = al[1:] * sg[:-1] ** 2 / al[:-1] - sg[:-1] * np.sqrt(sg[1:] ** 2 - tau2)
  g = np.sqrt(tau2)
  coef = np.stack([a - 1., b, g], axis=1)
  if not np.isfinite(coef).all():
    raise ValueError(f'{dpm.sde_name}: the step coefficients are not finite on this grid')
  return PicardSchedule(sde_name=dpm.sde_name, steps=steps, eta=eta, skip=skip, times=dpm.times, alpha=al, sigma=sg, coef=coef,
                        thr_unit=sg[:-1] ** 2, final=dpm.final)


def parallel_sample(score_fn, x, schedule, window, tol, denoise=False):
  """The loop: `x` (a contiguous fp32 device tensor [B, C, H, W] drawn from the prior at the schedule's T) is advanced IN
  PLACE to the schedule's eps -> ``(x, stats)`` with ``stats = dict(iterations, strides, evaluations)``: the number of
  iterations (sequential network evaluations of a batch of window B), the stride of each, and the sum of the live slots p
  over them (+ 1 with `denoise`): what a sequential loop would count as its evaluations.  denoise: one more evaluation at
  eps, at batch B, after which `x` holds the data prediction there (one ``stk_dpm_update_f32``)."""
  lib = _library()
  W, tol = _check_window(window), _check_tol(tol)
  mutils.check_inplace_state(x, lib)
  if x.dim() < 2:
    raise ValueError(f'x must be [B, ...], got shape {tuple(x.shape)}')
  B, n, N = x.shape[0], x.numel() // x.shape[0], schedule.steps
  device = x.device
  ws_bytes = int(lib.picard_ws_bytes(W, B, n))
  if ws_bytes < 0:
    raise ValueError(f'stk_picard_ws_bytes refuses a window of {W} slots of {B} rows of {n} (rc={ws_bytes})')
  ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
  X = x.unsqueeze(0).repeat(W + 1, *([1] * x.dim()))
  noisy = schedule.eta > 0.
  Z = torch.empty((W,) + tuple(x.shape), dtype=torch.float32, device=device) if noisy else None
  coef = torch.tensor(schedule.coef, dtype=torch.float32).to(device).contiguous()
  thr = torch.tensor(tol * tol * schedule.thr_unit * n, dtype=torch.float64).to(device)
  # slot j of the window at i0 is evaluated at times[i0 + min(j, p - 1)]: the padding repeats the last live time
  padded = np.concatenate([schedule.times[:N], np.full(W, schedule.times[N - 1])])
  t_all = torch.tensor(padded, dtype=torch.float32).to(device).repeat_interleave(B)
  stride_dev = torch.zeros(1, dtype=torch.int32, device=device)
  stream = stk_lib.stream_ptr(device)
  batch = (W * B,) + tuple(x.shape[1:])
  i0, entered, strides, evaluations = 0, 0, [], 0
  while i0 < N:
    p = min(W, N - i0)
    if noisy:
      for i in range(entered, i0 + p):                 # the steps that enter the window, in step order
        Z[i % W].copy_(torch.randn(tuple(x.shape), dtype=torch.float32, device=device))
      entered = i0 + p
    S = mutils.checked_score(score_fn, X[:W].view(batch), t_all[i0 * B:(i0 + W) * B], lib)
    with stk_lib.device_guard(device):
      lib.picard_scan_f32(X.data_ptr(), S.data_ptr(), mutils.optional_ptr(Z), coef.data_ptr(), i0, p, W, ws.data_ptr(), ws_bytes,
                          B, n, stream)
      lib.picard_stride(ws.data_ptr(), ws_bytes, thr.data_ptr(), i0, p, W, B, n, stride_dev.data_ptr(), None, stream)
      lib.picard_slide_f32(X.data_ptr(), stride_dev.data_ptr(), p, W, B, n, stream)
    stride = int(stride_dev.item())                    # the one host read of the iteration
    if not 1 <= stride <= p:
      raise RuntimeError(f'stk_picard_stride returned {stride} for a window of {p} live slots')
    strides.append(stride)
    evaluations += p
    i0 += stride
  x.copy_(X[0])
  if denoise:
    t = torch.full((B,), float(schedule.times[-1]), dtype=torch.float32, device=device)
    score = mutils.checked_score(score_fn, x, t, lib)
    dpm_solver._update(lib, x, score, None, schedule.final, (-math.inf, math.inf), x, None)
    evaluations += 1
  return x, dict(iterations=len(strides), strides=strides, evaluations=evaluations)


def get_parallel_sampler(config, sde, shape, inverse_scaler, steps=None, window=16, tol=0.01, eta=0., skip='time', denoise=True,
                         eps=1e-3, device='cuda', precision='fp32'):
  """``parallel_sampler(model) -> (samples, nfe)``: the loop above over `steps` steps (``sde.N`` where None) from ``sde.T``
  down to `eps`; ``nfe`` is the sum of the live slots over the iterations (+ 1 with `denoise`), and the sampler carries the
  ``stats`` of its last run as ``parallel_sampler.last_stats``.  Classes, guidance and augmentation labels in force around the
  call are repeated for the window's batch (``models.utils.tiled_conditions``); under guidance a window is one evaluation at
  batch 2 window B.  precision='fp16': every network evaluation runs in the engine's fp16 mode; the scan is always fp32."""
  lib = _library()
  window, tol = _check_window(window), _check_tol(tol)
  schedule = picard_schedule(sde, sde.N if steps is None else steps, eta=eta, skip=skip, eps=eps)
  mutils.check_precision(precision)

  def parallel_sampler(model):
    with mutils.sampling_run(model, precision):
      score_fn, x = mutils.score_and_prior(config, sde, model, shape, device, lib)

      def windowed(xw, t):
        if xw.shape[0] == x.shape[0]:                  # window = 1, and the evaluation of `denoise`
          return score_fn(xw, t)
        with mutils.tiled_conditions(model, window):
          return score_fn(xw, t)

      x, stats = parallel_sample(windowed, x, schedule, window, tol, denoise=denoise)
      parallel_sampler.last_stats = stats
      return inverse_scaler(x), stats['evaluations']

  parallel_sampler.last_stats = None
  return parallel_sampler


def sampling_options(config):
  """(steps, window, tol, eta, skip) of ``config.sampling.parallel_steps / parallel_window / parallel_tol / parallel_eta /
  parallel_skip``: None (``sde.N``), 16, 0.01, 0 and 'time' where a key is absent (the reference's configs have none).  The
  default tolerance is where a float64 model of the loop on a Gaussian data law stays within 8e-4 of max |x| of the sequential
  run; sample quality there is unmeasured."""
  read = lambda key, default: mutils.config_option(config, 'sampling', key, default)
  return (read('parallel_steps', None), read('parallel_window', 16), read('parallel_tol', 0.01), read('parallel_eta', 0.),
          read('parallel_skip', 'time'))
