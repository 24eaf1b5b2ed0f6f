"""Diffusion posterior sampling (Chung et al., "Diffusion Posterior Sampling for General Noisy Inverse Problems", 2023):
conditional sampling given a measurement ``y = A(x) (+ noise)`` for ANY differentiable operator ``A``, where the samplers of
``controllable_generation.py`` need an orthogonal projection.

A guided predictor step at ``(x, t)`` is, in this order (``dps_update``):

  1. ONE evaluation of the score network at ``(x, t)`` with the input gradient kept (the engine's forward under grad mode);
  2. ``stk_tweedie_f32``: the data prediction ``x0 = clamp((x + s^2 score) / a, lo, hi)``, ``(a, s)`` from ``sde.marginal_prob``;
  3. the operator, ``m = A(x0)``, under autograd;
  4. ``stk_residual_f32``: ``r = y - m`` and the float64 partial sums of its squares, per sample;
  5. ``v = autograd.grad(m, x0, r)``, that is ``A^T r``;
  6. ``stk_guide_seed_f32``: ``|r|`` per sample and the seed ``(s^2 / a) v`` of the network's backward (0 where x0 is clamped);
  7. ``gnet = autograd.grad(score, x, seed)``: the engine's input-only backward (no parameter gradients);
  8. the unconditional predictor update ``x -> (xp, xpm)``, built on a score function that hands back the score of step 1: a
     guided step costs one forward and one input-only backward.  A predictor that asks for the score anywhere else raises;
  9. ``stk_guide_update_f32``: ``x = xp + (zeta / |r|) g``, ``x_mean = xpm + (zeta / |r|) g`` with ``g = v / a + gnet``
     (``g = gnet`` where x0 is clamped).

``g`` is ``-|r|`` times the gradient of ``|y - A(x0(x))|`` with respect to ``x``: the step descends the residual norm by ``zeta``.
The clamp has derivative 1 strictly inside ``(lo, hi)`` and 0 at a bound.  The guidance draws no noise: the only draws of a
step are the predictor's own.  The four launches are include/stk_posterior.h (csrc/posterior.hip); ``|r|`` is summed in
float64 in a fixed order and is bit-identical from run to run.

The network evaluations follow ``likelihood.py``: ``torch.no_grad`` and ``models.utils.frozen_weights`` around the loop, grad
mode only around the score and the operator.  fp32 only: ``config.sampling.precision = 'fp16'`` raises ValueError when the
sampler is built (the forward-only fp16 mode has no backward).  Everything runs on the device: host tensors raise the
package's device error; a library without include/stk_posterior.h is refused when the sampler is built.  Sample quality is
unmeasured.
"""
import math

import torch

from . import controllable_generation as cg
from .engine import lib as stk_lib
from .models import utils as mutils
from .op import _backend
from .op.upfirdn2d import upfirdn2d
from .sampling import NonePredictor, pc_updates, tqdm


def _library():
  return mutils.require('has_posterior', 'stk_posterior.h',
                        'stk_tweedie_f32, stk_residual_f32, stk_guide_seed_f32 and stk_guide_update_f32',
                        'the posterior sampler needs')


# ---- measurement operators: callables A(x0) -> m on fp32 device tensors, differentiable by autograd ------------------------
class GaussianBlur:
  """``size`` x ``size`` Gaussian blur of standard deviation ``std`` (pixels) with 'same' zero padding: ``op.upfirdn2d`` with
  the normalised taps, computed in float64 and rounded once (up to 8 x 8 taps run on the op's tiled kernels, more on its
  general one).  Its adjoint is upfirdn2d's own backward."""

  def __init__(self, size, std):
    if isinstance(size, bool) or not isinstance(size, int) or size < 1:        # what stk_upfirdn2d_f32 refuses, said here
      raise ValueError(f'size must be a positive int (the taps per side), got {size!r}')
    std = float(std)
    if not (std > 0. and math.isfinite(std)):
      raise ValueError(f'std must be positive and finite, got {std!r}')
    self.size, self.std = size, std
    self.taps = self.taps64(size, std).to(torch.float32)
    self.pad = (size // 2, (size - 1) // 2)

  @staticmethod
  def taps64(size, std):
    """The [size, size] float64 taps: the outer product of the sampled Gaussian with itself, normalised to sum 1."""
    i = torch.arange(size, dtype=torch.float64) - (size - 1) / 2.
    g = torch.exp(-0.5 * (i / std) ** 2)
    k = torch.outer(g, g)
    return k / k.sum()

  def __call__(self, x0):
    return upfirdn2d(x0, self.taps, pad=self.pad)


class Masking:
  """``m = mask * x0``: a float32 mask of the state's spatial size that broadcasts over batch and channels
  (``controllable_generation.mask_form``).  Unlike the inpainter, the measurement may be noisy."""

  def __init__(self, mask):
    if not torch.is_tensor(mask) or mask.dtype != torch.float32 or not 2 <= mask.dim() <= 4:
      raise ValueError('mask must be a float32 tensor [H,W], [C,H,W] or [N,C,H,W]')
    self.mask = mask

  def __call__(self, x0):
    cg.mask_form(self.mask, x0)
    _backend.check(self.mask, _backend.get())
    return x0 * self.mask.reshape((1,) * (4 - self.mask.dim()) + tuple(self.mask.shape))


class _BlockMean(torch.autograd.Function):
  """forward: ``controllable_generation.block_mean``.  backward: its adjoint, every pixel of a block receiving 1 / r^2 of the
  block's gradient -- ONE stk_superres_f32 launch on a zero state with a = 1 / r^2 (exact: r is a power of two)."""

  @staticmethod
  def forward(ctx, x0, r):
    ctx.r = r
    return cg.block_mean(x0, r)

  @staticmethod
  def backward(ctx, gm):
    r = ctx.r
    lib = cg._superres_library()
    gm = gm.contiguous()
    N, C, h, w = gm.shape
    zero = torch.zeros((N, C, h * r, w * r), dtype=torch.float32, device=gm.device)
    a = torch.full((N,), 1. / (r * r), dtype=torch.float32, device=gm.device)
    return cg._superres(lib, zero, gm, None, a, a, r, torch.empty_like(zero), None), None


class BlockAveraging:
  """``m`` = the ``factor`` x ``factor`` block means of x0, ``factor`` in ``controllable_generation.FACTORS``: noisy
  super-resolution."""

  def __init__(self, factor):
    self.factor = cg._check_factor(factor)

  def __call__(self, x0):
    return _BlockMean.apply(x0, self.factor)


# ---- argument checks ---------------------------------------------------------------------------------------------------
def _check_zeta(zeta):
  zeta = float(zeta)
  if not zeta >= 0.:                 # a NaN fails the comparison
    raise ValueError(f'zeta must be non-negative, got {zeta!r}')
  return zeta


def _check_clip(clip):
  """(lo, hi) as floats; None is no clamp."""
  if clip is None:
    return -math.inf, math.inf
  try:
    lo, hi = (float(v) for v in clip)
  except (TypeError, ValueError):
    raise ValueError(f'clip must be None or a (lo, hi) pair with lo < hi, got {clip!r}') from None
  if not lo < hi:
    raise ValueError(f'clip must be None or a (lo, hi) pair with lo < hi, got {clip!r}')
  return lo, hi


def _check_fp32(config):
  if mutils.sampling_precision(config) != 'fp32':
    raise ValueError("posterior sampling runs in fp32 only: config.sampling.precision='fp16' is refused (the guidance "
                     "differentiates the network, and the forward-only fp16 mode has no backward)")


def _vec_t(x, t):
  if torch.is_tensor(t) and t.dim() == 1:
    return t
  return torch.ones(x.shape[0], device=x.device) * t


# ---- the launches --------------------------------------------------------------------------------------------------------
def _ptr(t):
  return t.data_ptr() if t is not None else None


def _gradient_parts(lib, score_fn, sde, operator, y, x, vec_t, lo, hi):
  """Steps 1-7 of the module docstring on a checked, contiguous state -> (score, v, gnet, x0, a, rnorm): the detached score at
  (x, vec_t), A^T r, the network's vjp of the seed, the data prediction, the mean coefficient [N] and |r| [N]."""
  N, n = x.shape[0], x[0].numel()
  dev, stream = x.device, stk_lib.stream_ptr(x.device)
  a, s = cg._coefficients(sde, x, vec_t)
  with torch.enable_grad():
    xg = x.detach().requires_grad_(True)
    score_g = score_fn(xg, vec_t)
  _backend.check(score_g, lib)
  if score_g.shape != x.shape or score_g.dtype != torch.float32:
    raise ValueError(f'score_fn returned {score_g.dtype} {tuple(score_g.shape)} for a float32 state {tuple(x.shape)}')
  score = score_g.detach().contiguous()
  x0 = torch.empty_like(x)
  with stk_lib.device_guard(dev):
    lib.tweedie_f32(x.data_ptr(), score.data_ptr(), a.data_ptr(), s.data_ptr(), lo, hi, x0.data_ptr(), N, n, stream)
  with torch.enable_grad():
    x0g = x0.requires_grad_(True)
    m_g = operator(x0g)
  if not torch.is_tensor(m_g) or m_g.dtype != torch.float32 or m_g.dim() < 1 or m_g.shape[0] != N or m_g.numel() == 0:
    raise ValueError(f'the operator must return a non-empty float32 tensor [N, ...] with N = {N}, got '
                     f'{getattr(m_g, "dtype", type(m_g))} {tuple(getattr(m_g, "shape", ()))}')
  _backend.check(m_g, lib)
  if tuple(y.shape) != tuple(m_g.shape):
    raise ValueError(f'y {tuple(y.shape)} does not match the operator\'s output {tuple(m_g.shape)}')
  if not m_g.requires_grad:
    raise ValueError('the operator\'s output does not depend on its input through autograd')
  m = m_g.detach().contiguous()
  k = m.numel() // N
  r = torch.empty_like(m)
  ws_bytes = lib.posterior_ws_bytes(N, k)
  if ws_bytes <= 0:
    raise stk_lib.StkError(f'stk_posterior_ws_bytes({N}, {k}) = {ws_bytes}')
  ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
  with stk_lib.device_guard(dev):
    lib.residual_f32(y.data_ptr(), m.data_ptr(), r.data_ptr(), ws.data_ptr(), ws_bytes, N, k, stream)
  v = torch.autograd.grad(m_g, x0g, r)[0].contiguous()
  x0 = x0g.detach()
  seed, rnorm = torch.empty_like(x), torch.empty(N, dtype=torch.float32, device=dev)
  with stk_lib.device_guard(dev):
    lib.guide_seed_f32(v.data_ptr(), x0.data_ptr(), a.data_ptr(), s.data_ptr(), lo, hi, ws.data_ptr(), ws_bytes, k,
                       seed.data_ptr(), rnorm.data_ptr(), N, n, stream)
  gnet = torch.autograd.grad(score_g, xg, seed)[0].contiguous()
  return score, v, gnet, x0, a, rnorm


def _guide_update(lib, xp, xpm, v, gnet, x0, a, rnorm, zeta, lo, hi, x_out, xmean_out):
  N, n = xp.shape[0], xp[0].numel()
  with stk_lib.device_guard(xp.device):
    lib.guide_update_f32(xp.data_ptr(), _ptr(xpm), v.data_ptr(), gnet.data_ptr(), x0.data_ptr(), a.data_ptr(),
                         rnorm.data_ptr(), zeta, lo, hi, x_out.data_ptr(), _ptr(xmean_out), N, n,
                         stk_lib.stream_ptr(xp.device))


def _check_inputs(lib, x, y):
  for v in (x, y):
    _backend.check(v, lib)
  cg._check_state(x, 'x')
  if y.dtype != torch.float32 or y.dim() < 1 or y.shape[0] != x.shape[0]:
    raise ValueError(f'y must be a float32 tensor [N, ...] with N = {x.shape[0]}, got {y.dtype} {tuple(y.shape)}')


def measurement_gradient(score_fn, sde, operator, y, x, t, clip=None):
  """``(g, rnorm, x0)`` at ``(x, t)``: ``g = v / a + gnet`` [N,C,H,W] (module docstring; ``-|r|`` times the gradient of
  ``|y - A(x0(x))|``), ``rnorm = |y - A(x0)|`` [N], and the data prediction x0.  One score evaluation and one input-only
  backward.  `x` is not written."""
  lib = _library()
  _check_inputs(lib, x, y)
  lo, hi = _check_clip(clip)
  with torch.no_grad():
    xc = x.contiguous()
    _, v, gnet, x0, a, rnorm = _gradient_parts(lib, score_fn, sde, operator, y.contiguous(), xc, _vec_t(xc, t), lo, hi)
    # g through the update itself: 0 + (1 / 1) g
    g, one = torch.empty_like(xc), torch.ones_like(rnorm)
    _guide_update(lib, torch.zeros_like(xc), None, v, gnet, x0, a, one, 1., lo, hi, g, None)
  return g, rnorm, x0


def _dps_step(lib, config, sde, score_fn, predictor, operator, y, x, vec_t, zeta, probability_flow, lo, hi):
  """One guided predictor step on checked, contiguous tensors (steps 1-9 of the module docstring)."""
  score, v, gnet, x0, a, rnorm = _gradient_parts(lib, score_fn, sde, operator, y, x, vec_t, lo, hi)

  def known_score(xq, tq, *args, **kwargs):
    same_x = xq is x or (xq.data_ptr() == x.data_ptr() and xq.shape == x.shape and xq.stride() == x.stride())
    if not same_x or not (tq is vec_t or (tq.shape == vec_t.shape and torch.equal(tq, vec_t))):
      raise RuntimeError('the predictor of a guided step asked for the score at another point than (x, t): dps_update '
                         'evaluates the network once per step, use a predictor that takes its score at the current state')
    return score

  obj = NonePredictor(sde, known_score, probability_flow) if predictor is None \
      else predictor(config, sde, known_score, probability_flow)
  xp, xpm = obj.update_fn(x, vec_t)
  xp, xpm = xp.contiguous(), xpm.contiguous()
  # the update's own outputs are overwritten in place, unless they are the caller's tensor or one another (the identity
  # predictor returns x itself, twice)
  if len({x.data_ptr(), xp.data_ptr(), xpm.data_ptr()}) == 3:
    out, mean = xp, xpm
  else:
    out, mean = torch.empty_like(xp), torch.empty_like(xpm)
  _guide_update(lib, xp, xpm, v, gnet, x0, a, rnorm, zeta, lo, hi, out, mean)
  return out, mean, rnorm


def dps_update(config, sde, score_fn, predictor, operator, y, x, t, zeta, probability_flow=False, clip=None):
  """One guided predictor step at time t -> ``(x, x_mean, rnorm)``: the update of ``predictor`` (a class of
  ``sampling.get_predictor``, or None for the identity) moved by ``(zeta / |r|) g``.  One forward and one input-only backward
  of the network; the only draws are the predictor's own.  `x` is not written."""
  lib = _library()
  _check_inputs(lib, x, y)
  zeta = _check_zeta(zeta)
  lo, hi = _check_clip(clip)
  with torch.no_grad():
    xc = x.contiguous()
    return _dps_step(lib, config, sde, score_fn, predictor, operator, y.contiguous(), xc, _vec_t(xc, t), zeta,
                     probability_flow, lo, hi)


def get_dps_sampler(config, sde, operator, predictor, corrector, inverse_scaler, snr, n_steps=1, probability_flow=False,
                    continuous=False, denoise=True, eps=1e-5, zeta=1.0, clip=None):
  """``dps_sampler(model, y)`` -> [N,C,H,W]: PC sampling from the prior given the measurement ``y = operator(image)`` [N, ...]
  (float32, in the model's data scale).  ``controllable_generation``'s loop: at each of ``linspace(sde.T, eps, sde.N)`` the
  unguided corrector (``sampling.shared_corrector_update_fn``), then the guided predictor (``dps_update``)."""
  lib = _library()
  _check_fp32(config)
  zeta = _check_zeta(zeta)
  lo, hi = _check_clip(clip)
  if not callable(operator):
    raise ValueError(f'operator must be a callable A(x0) -> m, got {operator!r}')
  _, correct = pc_updates(config, sde, predictor, corrector, snr, n_steps, probability_flow, continuous)
  size, channels = config.data.image_size, config.data.num_channels

  def dps_sampler(model, y):
    _backend.check(y, lib)
    if y.dtype != torch.float32 or y.dim() < 1 or y.shape[0] < 1:
      raise ValueError(f'y must be a non-empty float32 tensor [N, ...], got {y.dtype} {tuple(y.shape)}')
    y = y.contiguous()
    N = y.shape[0]
    with mutils.sampling_run(model):
      score_fn = mutils.get_score_fn(config, sde, model, train=False, continuous=continuous)
      x = x_mean = sde.prior_sampling((N, channels, size, size)).to(y.device).contiguous()
      timesteps = torch.linspace(sde.T, eps, sde.N)
      for i in tqdm(range(sde.N)):
        vec_t = torch.ones(N, device=y.device) * timesteps[i]
        x, x_mean = correct(x, vec_t, model=model)
        x, x_mean, _ = _dps_step(lib, config, sde, score_fn, predictor, operator, y, x.contiguous(), vec_t, zeta,
                                 probability_flow, lo, hi)
      return inverse_scaler(x_mean if denoise else x)

  return dps_sampler
