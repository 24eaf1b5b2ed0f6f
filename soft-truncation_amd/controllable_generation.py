"""Conditional predictor-corrector samplers: inpainting and colourisation (score_sde's controllable_generation.py, which
the reference dropped from its fork), and super-resolution, the member of that family upstream does not spell out.

``get_pc_inpainter`` / ``get_pc_colorizer`` keep upstream's names, update rules and loop; like ``sampling.get_pc_sampler``
of this package they take ``config`` first.  At each of the N times of ``linspace(sde.T, eps, sde.N)`` the corrector
half-step runs first, then the predictor half-step.  A half-step is, in this order:

  1. the unconditional update (``sampling.shared_corrector_update_fn`` / ``shared_predictor_update_fn``): the network on the
     HIP engine, with whatever noise the update draws;
  2. ``sde.marginal_prob`` at this time, per image: the mean coefficient ``a`` and the std ``s`` of the perturbed data;
  3. ONE ``torch.randn_like(x)``;
  4. ONE launch of ``stk_impute_f32`` (include/stk_impute.h, csrc/impute.hip): the known part of the state becomes
     ``a data + s z`` under the mask, and ``x_mean`` its noise-free counterpart -- blended from the NEW x, as upstream does.

That draw order is part of the interface.  For colourisation the blend happens in the decoupled colour space (upstream's
orthogonal matrix ``M``, applied per pixel as ``einsum('bihw,ij->bjhw')``) with the mask selecting its first channel; the two
3x3 products are part of the same launch.  ``z`` lives in that space.

The network evaluations follow the engine's conventions exactly as ``get_pc_sampler`` does: ``torch.no_grad``, weights
prepared once per run (``models.utils.frozen_weights``), ``config.sampling.precision`` ('fp16' applies to the network only:
the imputation is always fp32).  Everything runs on the device: host tensors raise the package's device error, there is
no CPU path; a library without include/stk_impute.h is refused when the sampler is built.

``get_pc_superresolver`` samples a full-resolution image given its r x r block means ``low`` [N,C,H/r,W/r] (``block_mean`` makes
one from an image), r = ``factor`` in {2, 4, 8, 16}.  It is the colouriser's construction with the orthonormal transform
acting on the r^2 pixels of a block instead of the 3 channels of a pixel, the kept coefficient being the block's DC term:
r times the block mean, so noise of std ``s`` on the data is ``s / r`` on the mean.  The loop and the conventions are those
above.  A half-step (``superres_update``) is, in this order: the unconditional update; ``sde.marginal_prob`` per image;
ONE ``torch.randn`` of ``low``'s shape (fp32, on x's device); ONE launch of ``stk_superres_f32`` (include/stk_superres.h,
csrc/superres.hip), which shifts every pixel of a block by ``(a low + (s / r) z) - blockmean(x)``, and by
``a low - blockmean(x)`` for ``x_mean``.  That draw order, too, is part of the interface.  A library without
include/stk_superres.h is refused when the sampler is built.  Sample quality is unmeasured.
"""
import ctypes

import numpy as np
import torch

from .engine import lib as stk_lib
from .models import utils as mutils
from .op import _backend
from .sampling import pc_updates, tqdm

# upstream's decoupling matrix: orthogonal, its first column the gray axis (1, 1, 1) / sqrt(3)
M = torch.tensor([[5.7735014e-01, -8.1649649e-01, 4.7008697e-08],
                  [5.7735026e-01, 4.0824834e-01, 7.0710671e-01],
                  [5.7735026e-01, 4.0824822e-01, -7.0710683e-01]], dtype=torch.float32)
# its inverse, computed once in float64 and rounded
INV_M = torch.from_numpy(np.linalg.inv(M.numpy().astype(np.float64))).to(torch.float32)
_IDENTITY = torch.eye(3, dtype=torch.float32)


def _host9(m):
  return (ctypes.c_float * 9)(*m.reshape(-1).tolist())


# host arrays the entry copies into its launches; (mix, unmix) pairs
_C_M, _C_INV_M, _C_I = _host9(M), _host9(INV_M), _host9(_IDENTITY)
_MIX_BLEND = (_C_M, _C_INV_M)       # blend in the decoupled space, return to RGB
_MIX_DECOUPLE = (_C_M, _C_I)
_MIX_COUPLE = (_C_INV_M, _C_I)


def _library():
  return mutils.require('has_impute', 'stk_impute.h', 'stk_impute_f32', 'the inpainting and colourisation samplers need')


def mask_form(mask, data):
  """(mask_n, mask_c) of a mask for `data` [N,C,H,W]: the mask is fp32, of `data`'s spatial size, with a batch and a channel
  extent of 1 or of `data`'s (missing leading axes count as 1).  Host-only: reads shapes and dtypes, so meta tensors do."""
  if data.dim() != 4:
    raise ValueError(f'data must be [N,C,H,W], got {tuple(data.shape)}')
  if mask.dtype != torch.float32:
    raise ValueError(f'mask must be float32, got {mask.dtype}')
  if not 2 <= mask.dim() <= 4:
    raise ValueError(f'mask must be [H,W], [C,H,W] or [N,C,H,W] (extents 1 broadcast), got {tuple(mask.shape)}')
  shape = (1,) * (4 - mask.dim()) + tuple(mask.shape)
  N, C, H, W = data.shape
  if shape[2:] != (H, W) or shape[0] not in (1, N) or shape[1] not in (1, C):
    raise ValueError(f'mask {tuple(mask.shape)} does not broadcast to data {tuple(data.shape)} over batch and channels')
  return shape[0], shape[1]


def _check_state(x, what):
  if x.dim() != 4 or x.dtype != torch.float32:
    raise ValueError(f'{what} must be a float32 [N,C,H,W] tensor, got {x.dtype} {tuple(x.shape)}')


def _check_mask(lib, mask, data):
  """The whole mask check of one call: device, form, and values in [0, 1] (one reduction, one read-back)."""
  _backend.check(mask, lib)
  form = mask_form(mask, data)
  lo, hi = (float(v) for v in torch.aminmax(mask))
  if not (lo >= 0. and hi <= 1.):       # a NaN fails both comparisons
    raise ValueError(f'mask values must lie in [0, 1], got [{lo}, {hi}]')
  return form


def _same_shape(data, x, what):
  if tuple(data.shape) != tuple(x.shape):
    raise ValueError(f'{what} {tuple(data.shape)} does not match the state {tuple(x.shape)}')


def _impute(lib, x, data, z, mask, form, a, s, x_out, x_mean, mix=None):
  """One launch of stk_impute_f32 on contiguous fp32 device tensors.  mix: a (mix, unmix) pair of host arrays, or None."""
  N, C, H, W = x.shape
  with stk_lib.device_guard(x.device):
    lib.impute_f32(x.data_ptr(), data.data_ptr(), z.data_ptr() if z is not None else None, mask.data_ptr(), a.data_ptr(),
                   s.data_ptr(), ctypes.addressof(mix[0]) if mix else None, ctypes.addressof(mix[1]) if mix else None,
                   x_out.data_ptr(), x_mean.data_ptr() if x_mean is not None else None, N, C, H * W, form[0], form[1],
                   stk_lib.stream_ptr(x.device))
  return x_out


def _ones(x):
  return torch.ones(x.shape[0], dtype=torch.float32, device=x.device)


def _remix(inputs, mix):
  """inputs M per pixel through the kernel: an all-zero mask leaves x M untouched by the blend."""
  lib = _library()
  _backend.check(inputs, lib)
  _check_state(inputs, 'inputs')
  if inputs.shape[1] != 3:
    raise ValueError(f'the colour transform needs 3 channels, got {inputs.shape[1]}')
  x = inputs.contiguous()
  one = _ones(x)
  zero = torch.zeros((1, 1) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
  return _impute(lib, x, x, None, zero, (1, 1), one, one, torch.empty_like(x), None, mix)


def decouple(inputs):
  """RGB -> the decoupled space: ``einsum('bihw,ij->bjhw', inputs, M)``; channel 0 is sqrt(3) times the gray value."""
  return _remix(inputs, _MIX_DECOUPLE)


def couple(inputs):
  """The decoupled space -> RGB: ``einsum('bihw,ij->bjhw', inputs, inv(M))``."""
  return _remix(inputs, _MIX_COUPLE)


def get_mask(image):
  """Ones on channel 0, zeros elsewhere, shaped like `image`: the known part of a gray image in the decoupled space."""
  mask = torch.zeros_like(image)
  mask[:, :1] = 1.
  return mask


def _coefficients(sde, x, vec_t):
  """(a, s) [N] of ``sde.marginal_prob`` at vec_t: the mean is a * data for every SDE of sde_lib, so the coefficient is the
  mean of a tensor of ones -- exactly the SDE's own fp32 value (1 for the VE family), no division of tensors."""
  one = torch.ones((x.shape[0], 1, 1, 1), dtype=torch.float32, device=x.device)
  coeff, std = sde.marginal_prob(one, vec_t)
  return coeff.reshape(-1).to(torch.float32).contiguous(), std.to(torch.float32).contiguous()


def _half_step(lib, update_fn, sde, model, data, mask, form, x, t, mix):
  """update, marginal_prob, one randn_like, one launch (module docstring).  data, mask: contiguous and checked."""
  vec_t = torch.ones(data.shape[0], device=data.device) * t
  xu, _ = update_fn(x, vec_t, model=model)
  a, s = _coefficients(sde, data, vec_t)
  z = torch.randn_like(xu)
  xu = xu.contiguous()
  # the update's own output is overwritten in place, unless it is the caller's tensor (the identity updates return x itself)
  out = xu if xu.data_ptr() != x.data_ptr() else torch.empty_like(xu)
  x_mean = torch.empty_like(xu)
  _impute(lib, xu, data, z, mask, form, a, s, out, x_mean, mix)
  return out, x_mean


def inpaint_update(update_fn, sde, model, data, mask, x, t):
  """One inpainting half-step at time t around ``update_fn(x, vec_t, model=model)`` -> (x, x_mean): where the mask is 1 the
  state becomes the data perturbed to time t, elsewhere it stays what the update gave (upstream's inpaint_update_fn)."""
  lib = _library()
  for v in (x, data):
    _backend.check(v, lib)
  _check_state(x, 'x')
  _same_shape(data, x, 'data')
  _check_state(data, 'data')
  form = _check_mask(lib, mask, data)
  with torch.no_grad():
    return _half_step(lib, update_fn, sde, model, data.contiguous(), mask.contiguous(), form, x, t, None)


def _check_gray(lib, gray, x=None):
  _backend.check(gray, lib)
  _check_state(gray, 'gray_scale_img')
  if gray.shape[1] != 3:
    raise ValueError(f'gray_scale_img must have 3 channels, got {gray.shape[1]}')
  if x is not None:
    _backend.check(x, lib)
    _check_state(x, 'x')
    _same_shape(gray, x, 'gray_scale_img')


def colorize_update(update_fn, sde, model, gray, x, t):
  """One colourisation half-step at time t -> (x, x_mean): the inpainting half-step in the decoupled colour space, the
  mask being its channel 0 (upstream's colorization_update_fn)."""
  lib = _library()
  _check_gray(lib, gray, x)
  with torch.no_grad():
    return _half_step(lib, update_fn, sde, model, gray.contiguous(), get_mask(gray[:1]), (1, 3), x, t, _MIX_BLEND)


def _run(config, sde, lib, model, data, mask, form, mix, updates, inverse_scaler, denoise, eps):
  """The loop both samplers share.  The first launch is the initialisation: a = 1 and no noise give
  data mask + prior (1 - mask), in the decoupled space when `mix` is given."""
  predict, correct = updates
  with mutils.sampling_run(model, mutils.sampling_precision(config)):
    prior = sde.prior_sampling(data.shape).to(data.device).contiguous()
    one = _ones(data)
    x = x_mean = _impute(lib, prior, data, None, mask, form, one, one, prior, None, mix)
    timesteps = torch.linspace(sde.T, eps, sde.N)
    for i in tqdm(range(sde.N)):
      t = timesteps[i]
      x, x_mean = _half_step(lib, correct, sde, model, data, mask, form, x, t, mix)
      x, x_mean = _half_step(lib, predict, sde, model, data, mask, form, x, t, mix)
    return inverse_scaler(x_mean if denoise else x)


def get_pc_inpainter(config, sde, predictor, corrector, inverse_scaler, snr, n_steps=1, probability_flow=False,
                     continuous=False, denoise=True, eps=1e-5):
  """``pc_inpainter(model, data, mask)``: PC sampling of the part of `data` [N,C,H,W] where `mask` is 0, given the part where
  it is 1 (a float32 mask in [0, 1] that broadcasts over batch and channels; fractional values blend)."""
  lib = _library()
  updates = pc_updates(config, sde, predictor, corrector, snr, n_steps, probability_flow, continuous)
  mutils.sampling_precision(config)            # a bad config.sampling.precision fails here, not in the loop

  def pc_inpainter(model, data, mask):
    _backend.check(data, lib)
    _check_state(data, 'data')
    form = _check_mask(lib, mask, data)
    return _run(config, sde, lib, model, data.contiguous(), mask.contiguous(), form, None, updates, inverse_scaler, denoise,
                eps)

  return pc_inpainter


def get_pc_colorizer(config, sde, predictor, corrector, inverse_scaler, snr, n_steps=1, probability_flow=False,
                     continuous=False, denoise=True, eps=1e-5):
  """``pc_colorizer(model, gray_scale_img)``: PC sampling of the colour of a gray image given as [N,3,H,W]."""
  lib = _library()
  updates = pc_updates(config, sde, predictor, corrector, snr, n_steps, probability_flow, continuous)
  mutils.sampling_precision(config)

  def pc_colorizer(model, gray_scale_img):
    _check_gray(lib, gray_scale_img)
    gray = gray_scale_img.contiguous()
    return _run(config, sde, lib, model, gray, get_mask(gray[:1]), (1, 3), _MIX_BLEND, updates, inverse_scaler, denoise, eps)

  return pc_colorizer


FACTORS = (2, 4, 8, 16)      # the block sizes of include/stk_superres.h


def _superres_library():
  return mutils.require('has_superres', 'stk_superres.h', 'stk_superres_f32 and stk_block_mean_f32',
                        'the super-resolution sampler needs')


def _check_factor(factor):
  if isinstance(factor, bool) or not isinstance(factor, int) or factor not in FACTORS:
    raise ValueError(f'factor must be one of {FACTORS}, got {factor!r}')
  return factor


def superres_shape(low, factor):
  """The [N,C,H,W] shape of the image a measurement `low` [N,C,H/r,W/r] (float32) of block size r = `factor` belongs to.
  Host-only: reads shapes and dtypes, so meta tensors do."""
  r = _check_factor(factor)
  if low.dim() != 4 or low.dtype != torch.float32:
    raise ValueError(f'low must be a float32 [N,C,H/{r},W/{r}] tensor, got {low.dtype} {tuple(low.shape)}')
  N, C, h, w = low.shape
  if min(N, C, h, w) < 1:
    raise ValueError(f'low must not be empty, got {tuple(low.shape)}')
  return N, C, h * r, w * r


def _check_low(low, factor, shape, what):
  """`low` is the measurement of an [N,C,H,W] = `shape` image at this factor."""
  full = superres_shape(low, factor)
  if full != tuple(shape):
    raise ValueError(f'low {tuple(low.shape)} at factor {factor} stands for an image of {full}, not for {what} {tuple(shape)}')


def _superres(lib, x, low, z, a, s, r, x_out, x_mean):
  """One launch of stk_superres_f32 on contiguous fp32 device tensors."""
  N, C, H, W = x.shape
  with stk_lib.device_guard(x.device):
    lib.superres_f32(x.data_ptr(), low.data_ptr(), z.data_ptr() if z is not None else None, a.data_ptr(), s.data_ptr(),
                     x_out.data_ptr(), x_mean.data_ptr() if x_mean is not None else None, N, C, H, W, r,
                     stk_lib.stream_ptr(x.device))
  return x_out


def block_mean(images, factor):
  """The r x r block means of `images` [N,C,H,W] -> [N,C,H/r,W/r], r = `factor`: the measurement the super-resolution
  sampler takes (one launch of stk_block_mean_f32, the sum the data-consistency step itself takes)."""
  lib = _superres_library()
  _backend.check(images, lib)
  _check_state(images, 'images')
  r = _check_factor(factor)
  N, C, H, W = images.shape
  if N * C == 0 or H == 0 or W == 0 or H % r or W % r:
    raise ValueError(f'images {tuple(images.shape)} do not divide into {r} x {r} blocks')
  x = images.contiguous()
  out = torch.empty((N, C, H // r, W // r), dtype=torch.float32, device=x.device)
  with stk_lib.device_guard(x.device):
    lib.block_mean_f32(x.data_ptr(), out.data_ptr(), N * C, H, W, r, stk_lib.stream_ptr(x.device))
  return out


def _superres_half_step(lib, update_fn, sde, model, low, r, x, t):
  """update, marginal_prob, one randn of low's shape, one launch (module docstring).  low: contiguous and checked."""
  vec_t = torch.ones(low.shape[0], device=low.device) * t
  xu, _ = update_fn(x, vec_t, model=model)
  a, s = _coefficients(sde, low, vec_t)
  z = torch.randn(low.shape, dtype=torch.float32, device=xu.device)
  xu = xu.contiguous()
  # as in _half_step: overwrite the update's own output, never the caller's tensor
  out = xu if xu.data_ptr() != x.data_ptr() else torch.empty_like(xu)
  x_mean = torch.empty_like(xu)
  _superres(lib, xu, low, z, a, s, r, out, x_mean)
  return out, x_mean


def superres_update(update_fn, sde, model, low, factor, x, t):
  """One super-resolution half-step at time t around ``update_fn(x, vec_t, model=model)`` -> (x, x_mean): the r x r block
  means of the state become ``a low + (s / r) z`` (``a low`` for x_mean), what the update gave is kept otherwise.  Draw
  order: the update's own noise, then ONE ``torch.randn`` of low's shape on x's device.  `x` is not written."""
  lib = _superres_library()
  for v in (x, low):
    _backend.check(v, lib)
  _check_state(x, 'x')
  _check_low(low, factor, x.shape, 'the state')
  with torch.no_grad():
    return _superres_half_step(lib, update_fn, sde, model, low.contiguous(), factor, x, t)


def get_pc_superresolver(config, sde, predictor, corrector, inverse_scaler, snr, n_steps=1, probability_flow=False,
                         continuous=False, denoise=True, eps=1e-5, factor=4):
  """``pc_superresolver(model, low)`` -> [N,C,H,W]: PC sampling of an image whose `factor` x `factor` block means are `low`
  [N,C,H/factor,W/factor], float32 in the model's data scale; H = W = ``config.data.image_size``."""
  lib = _superres_library()
  r = _check_factor(factor)
  updates = pc_updates(config, sde, predictor, corrector, snr, n_steps, probability_flow, continuous)
  precision = mutils.sampling_precision(config)      # a bad config.sampling.precision fails here, not in the loop
  size, channels = config.data.image_size, config.data.num_channels
  if size % r:
    raise ValueError(f'config.data.image_size = {size} does not divide into {r} x {r} blocks')

  def pc_superresolver(model, low):
    _backend.check(low, lib)
    shape = (superres_shape(low, r)[0], channels, size, size)
    _check_low(low, r, shape, 'the model\'s input')
    low = low.contiguous()
    predict, correct = updates
    with mutils.sampling_run(model, precision):
      # the initial state: the prior with its block means replaced by low's (a = 1, no noise)
      prior = sde.prior_sampling(shape).to(low.device).contiguous()
      one = _ones(low)
      x = x_mean = _superres(lib, prior, low, None, one, one, r, prior, None)
      timesteps = torch.linspace(sde.T, eps, sde.N)
      for i in tqdm(range(sde.N)):
        t = timesteps[i]
        x, x_mean = _superres_half_step(lib, correct, sde, model, low, r, x, t)
        x, x_mean = _superres_half_step(lib, predict, sde, model, low, r, x, t)
      return inverse_scaler(x_mean if denoise else x)

  return pc_superresolver
