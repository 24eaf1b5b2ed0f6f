"""Model registry and the score-function wrappers (reference: models/utils.py).

Kept verbatim at the interface level so a ``run_lib.py``-style driver works unchanged:
``register_model`` / ``get_model`` (:25-48), ``get_sigmas`` (:51-62), ``get_ddpm_params`` (:65-86),
``create_model`` (:89-95), ``get_model_fn`` (:97-126), ``get_score_fn`` (:128-190) and the
flatten helpers (:193-200).

MI355X-specific difference, by design: the reference wraps the model in
``torch.nn.DataParallel`` (one process, threads, per-forward broadcast of all 247 MB of
parameters).  Here every GPU runs its own process; :class:`DataParallel` below only keeps the
``module.`` key prefix of the reference's checkpoints and, when ``torch.distributed`` is
initialised, averages gradients with one bucketed RCCL all-reduce per step
(see ``engine/ddp.py``).
"""
import contextlib
import math

import numpy as np
import torch

from .. import sde_lib
from ..op import _backend

_MODELS = {}


def register_model(cls=None, *, name=None):
  """Decorator registering a model class under ``name`` (default: the class name)."""

  def add(model_cls):
    key = name if name is not None else model_cls.__name__
    if key in _MODELS:
      raise ValueError(f'Already registered model with name: {key}')
    _MODELS[key] = model_cls
    return model_cls

  return add if cls is None else add(cls)


def get_model(name):
  return _MODELS[name]


def get_sigmas(config):
  """Geometric ladder of SMLD noise levels, sigma_max -> sigma_min (models/utils.py:51-62)."""
  return np.exp(np.linspace(np.log(config.model.sigma_max), np.log(config.model.sigma_min),
                            config.model.num_scales))


def get_ddpm_params(config):
  """DDPM beta/alpha tables over 1000 steps (models/utils.py:65-86)."""
  steps, m = 1000, config.model
  lo, hi = m.beta_min / m.num_scales, m.beta_max / m.num_scales
  betas = np.linspace(lo, hi, steps, dtype=np.float64)
  alphas = 1. - betas
  cum = np.cumprod(alphas, axis=0)
  return dict(betas=betas, alphas=alphas, alphas_cumprod=cum, sqrt_alphas_cumprod=np.sqrt(cum),
              sqrt_1m_alphas_cumprod=np.sqrt(1. - cum), beta_min=lo * (steps - 1), beta_max=hi * (steps - 1),
              num_diffusion_timesteps=steps)


class DataParallel(torch.nn.Module):
  """Single-device stand-in for ``torch.nn.DataParallel`` (models/utils.py:94).

  state_dict keys keep the ``module.`` prefix of the reference's checkpoints.  Data
  parallelism is one process per GPU: gradient exchange happens in ``losses.optimize_fn`` via
  ``engine.ddp`` when a process group exists, never by replicating the module across threads.
  """

  def __init__(self, module):
    super().__init__()
    self.module = module

  def forward(self, *args, **kwargs):
    return self.module(*args, **kwargs)


def create_model(config, sde):
  """Instantiate ``config.model.name`` on ``config.device`` (models/utils.py:89-95)."""
  score_model = get_model(config.model.name)(config, sde)
  score_model = score_model.to(config.device)
  if hasattr(score_model, 'engine'):
    # bind the parameters to the flat HBM buffers now, so the optimizer and the EMA created right after
    # (utils.load_model) see the final storage.  Loads libstk.so: raises if the HIP library is missing.
    score_model.engine().ensure_flat()
  return DataParallel(score_model)


def frozen_weights(model):
  """Context manager for loops that evaluate `model` many times on fixed parameters (samplers, likelihood ODEs): the
  engine prepares the convolution weights once instead of once per evaluation.  A no-op for models without an engine."""
  inner = getattr(model, 'module', model)
  engine = getattr(inner, 'engine', None)
  return engine().frozen_weights() if callable(engine) else contextlib.nullcontext()


PRECISIONS = ('fp32', 'fp16')


def check_precision(value, what='precision'):
  if value not in PRECISIONS:
    raise ValueError(f'{what} must be one of {PRECISIONS}, got {value!r}')
  return value


def precision(model, precision):
  """Context manager: the network evaluations of `model` inside it run in `precision` -- 'fp32' (the default path) or
  'fp16' (one fp16 product per multiply-add in the split convolutions, include/stk_fp16.h; forward-only: a forward that
  a backward may follow raises ValueError inside the block).  For a user's own loop around get_score_fn.  A no-op for
  models without an engine (the value is still checked)."""
  check_precision(precision)
  inner = getattr(model, 'module', model)
  engine = getattr(inner, 'engine', None)
  return engine().precision(precision) if callable(engine) else contextlib.nullcontext()


def training_precision(model, precision):
  """Context manager: the network evaluations of `model` inside it that a backward may follow (grad mode, an input
  gradient) run in `precision`, forward and backward -- 'fp32' (the default path) or 'fp16' (one fp16 product per
  multiply-add in every split convolution, include/stk_fp16.h and include/stk_fp16_train.h).  Forward-only evaluations
  inside it keep following precision(), fp32 by default.  For a user's own training loop; get_step_fn applies it from
  config.training.precision.  A no-op for models without an engine (the value is still checked)."""
  check_precision(precision)
  inner = getattr(model, 'module', model)
  engine = getattr(inner, 'engine', None)
  return engine().training_precision(precision) if callable(engine) else contextlib.nullcontext()


def current_training_precision(model):
  """The training precision in force for `model` ('fp32' for a model without an engine)."""
  inner = getattr(model, 'module', model)
  engine = getattr(inner, 'engine', None)
  return engine().train_mode if callable(engine) else 'fp32'


def config_option(config, section, key, default):
  """``config.<section>.<key>``, or `default` where the key is absent (the reference's configs have none of the keys this
  package adds)."""
  try:
    return getattr(getattr(config, section), key)
  except (AttributeError, KeyError):
    return default


def config_training_precision(config):
  """config.training.precision: 'fp32' when the key is absent, else checked."""
  return check_precision(config_option(config, 'training', 'precision', 'fp32'), 'config.training.precision')


def sampling_precision(config):
  """config.sampling.precision: 'fp32' when the key is absent, else checked."""
  return check_precision(config_option(config, 'sampling', 'precision', 'fp32'), 'config.sampling.precision')


# ---- class conditioning and classifier-free guidance (include/stk_cond.h) ----------------------------------------------------
def num_classes(model):
  """C of a class-conditional network (config.model.num_classes), 0 for any other model; sees through DataParallel."""
  return int(getattr(getattr(model, 'module', model), 'num_classes', 0) or 0)


def as_class_tensor(classes, C, read_values=True):
  """`classes` -- a 1-D integer tensor, or a sequence of integers and None -- as an int64 tensor with None replaced by the
  null class C.  ValueError for another shape or dtype, for an empty batch, and (read_values: ONE host read of a device
  tensor) for a value outside [0, C]."""
  if torch.is_tensor(classes):
    if classes.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
      raise ValueError(f'classes must be an integer tensor, got {classes.dtype}')
    t = classes.to(torch.int64)
  else:
    try:
      items = list(classes)
    except TypeError:
      raise ValueError(f'classes must be a [B] integer tensor or a sequence, got {type(classes).__name__}') from None
    for v in items:
      if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
        raise ValueError(f'classes must hold integers or None, got {v!r}')
    t = torch.tensor([C if v is None else int(v) for v in items], dtype=torch.int64)
  if t.dim() != 1 or t.numel() == 0:
    raise ValueError(f'classes must have shape [B] with B > 0, got {tuple(t.shape)}')
  if read_values:
    lo, hi = torch.stack(torch.aminmax(t)).tolist()
    if lo < 0 or hi > C:
      raise ValueError(f'classes must lie in [0, {C}] ({C} is the null class), got values from {lo} to {hi}')
  return t


@contextlib.contextmanager
def classes_in_force(model, cls):
  """The unchecked core of :func:`class_condition` without guidance, for callers that have checked already (get_step_fn):
  `cls` is a [B] float32 tensor of class indices on the model's device."""
  inner = getattr(model, 'module', model)
  saved, inner._class_ctx = inner._class_ctx, (cls, 0.0, None)
  saved_rescale, inner._cfg_rescale = getattr(inner, '_cfg_rescale', 0.0), 0.0
  try:
    yield
  finally:
    inner._class_ctx, inner._cfg_rescale = saved, saved_rescale


@contextlib.contextmanager
def class_condition(model, classes, guidance=0.0, rescale=0.0):
  """Context manager: every network evaluation of the class-conditional `model` inside it is conditioned on `classes` -- a
  [B] integer tensor or sequence, the value C (= config.model.num_classes) or None for the null class -- with
  classifier-free guidance of weight `guidance`: out = c + guidance (c - u), c the evaluation with the classes, u the one
  with the null class.  guidance = 0 is the plain conditional evaluation, one pass at batch B, bit for bit; any other
  weight costs ONE pass at batch 2 B ([x; x] with classes [y; null]) and one launch of stk_cfg_combine_f32 (torch
  operators under grad mode, where autograd has to see the combination), and the engine's arena of a batch of 2 B.

  rescale = phi in [0, 1] (Lin et al. 2024, "Common Diffusion Noise Schedules and Sample Steps Are Flawed", section 3.4)
  pulls each sample's guided output g back towards the standard deviation of its conditional output c:
  out = (phi std(c) / std(g) + 1 - phi) g, the standard deviations per sample over C H W in population form.  0 is the
  path above, bit for bit; any other value replaces the combination by the two launches of stk_cfg_rescale_f32
  (include/stk_guided.h; the same formula by torch operators under grad mode, so the DPS sampler and the likelihood
  differentiate through it); with guidance = 0 it is accepted and does nothing (c is its own target).  Sample quality under
  it is unmeasured.  A model whose library lacks include/stk_guided.h raises NotImplementedError at its first guided evaluation.

  Every sampler takes classes through it unchanged: ``with class_condition(model, y, 1.5): sampling_fn(model)``.
  Checked once, on entry, with one host read: ValueError for a model that is not class-conditional, a wrong shape or
  dtype, a value outside [0, C], a guidance weight that is not finite, a rescale outside [0, 1]; an evaluation of a batch of
  another size inside it raises ValueError too.  Contexts nest and restore; `model` may be the DataParallel wrapper."""
  inner = getattr(model, 'module', model)
  C = num_classes(model)
  if C <= 0:
    raise ValueError(f'{type(inner).__name__} is not class-conditional (config.model.num_classes is absent or 0)')
  try:
    w = float(guidance)
  except (TypeError, ValueError):
    raise ValueError(f'guidance must be a finite number, got {guidance!r}') from None
  if not math.isfinite(w):
    raise ValueError(f'guidance must be a finite number, got {guidance!r}')
  try:
    phi = float(rescale)
  except (TypeError, ValueError):
    raise ValueError(f'rescale must be a number in [0, 1], got {rescale!r}') from None
  if not 0.0 <= phi <= 1.0:
    raise ValueError(f'rescale must be a number in [0, 1], got {rescale!r}')
  device = next(inner.parameters()).device
  cls = as_class_tensor(classes, C).to(device=device, dtype=torch.float32)
  both = torch.cat([cls, inner.null_classes(cls.shape[0], device)]) if w != 0.0 else None
  saved, inner._class_ctx = inner._class_ctx, (cls, w, both)
  saved_rescale, inner._cfg_rescale = getattr(inner, '_cfg_rescale', 0.0), phi
  try:
    yield
  finally:
    inner._class_ctx, inner._cfg_rescale = saved, saved_rescale


# ---- augmentation labels (include/stk_augment.h, augment.py) ---------------------------------------------------------------
def augment_dim(model):
  """K of a network with an augmentation embedding (config.model.augment_dim), 0 for any other; sees through DataParallel."""
  return int(getattr(getattr(model, 'module', model), 'augment_dim', 0) or 0)


@contextlib.contextmanager
def augment_in_force(model, labels):
  """The unchecked core of :func:`augment_condition`, for callers that have checked already (get_step_fn): `labels` is a
  [B, K] float32 tensor on the model's device."""
  inner = getattr(model, 'module', model)
  saved, inner._aug_ctx = inner._aug_ctx, labels
  try:
    yield
  finally:
    inner._aug_ctx = saved


@contextlib.contextmanager
def augment_condition(model, labels):
  """Context manager: every network evaluation of `model` inside it is told the augmentation `labels` -- a [B, K] float
  tensor, K = config.model.augment_dim -- of the images it sees (losses.get_step_fn under config.training.augment).  With no
  context in force the labels are zeros: a clean image, which is what sampling, the likelihood and DPS evaluate.  Under
  classifier-free guidance (class_condition with a weight) the labels are repeated for the [x; x] batch.  ValueError: a
  model without the embedding, labels of another shape; an evaluation of a batch of another size inside it raises ValueError
  too.  Contexts nest and restore; `model` may be the DataParallel wrapper."""
  inner = getattr(model, 'module', model)
  K = augment_dim(model)
  if K <= 0:
    raise ValueError(f'{type(inner).__name__} has no augmentation embedding (config.model.augment_dim is absent or 0)')
  if not torch.is_tensor(labels) or labels.dim() != 2 or labels.shape[1] != K or labels.shape[0] == 0 or \
      not labels.dtype.is_floating_point:
    raise ValueError(f'augmentation labels must be a [B, {K}] float tensor (config.model.augment_dim = {K}), got '
                     f'{tuple(labels.shape) if torch.is_tensor(labels) else type(labels).__name__}')
  device = next(inner.parameters()).device
  saved, inner._aug_ctx = inner._aug_ctx, labels.detach().to(device=device, dtype=torch.float32).contiguous()
  try:
    yield
  finally:
    inner._aug_ctx = saved


@contextlib.contextmanager
def tiled_conditions(model, reps):
  """Context manager: the class context in force (models.utils.class_condition: the classes, and [classes; null] under
  guidance) and the augmentation labels in force (augment_condition) are repeated `reps` times, slot-major -- the conditions of
  a batch [reps, B] that stacks `reps` copies of the batch they were given for (the window of parallel_sampling.py).  With
  no context in force it does nothing.  Contexts nest and restore; `model` may be the DataParallel wrapper."""
  try:
    ok = not isinstance(reps, bool) and int(reps) == reps and reps >= 1
  except (TypeError, ValueError, OverflowError):
    ok = False
  if not ok:
    raise ValueError(f'reps must be a positive integer, got {reps!r}')
  reps = int(reps)
  inner = getattr(model, 'module', model)
  ctx, aug = getattr(inner, '_class_ctx', None), getattr(inner, '_aug_ctx', None)
  if reps == 1 or (ctx is None and aug is None):
    yield
    return
  if ctx is not None:
    cls, w, both = ctx
    tiled = cls.repeat(reps)
    inner._class_ctx = (tiled, w, None if both is None else torch.cat([tiled, both[cls.shape[0]:].repeat(reps)]))
  if aug is not None:
    inner._aug_ctx = aug.repeat(reps, 1)
  try:
    yield
  finally:
    if ctx is not None:
      inner._class_ctx = ctx
    if aug is not None:
      inner._aug_ctx = aug


# ---- what the samplers share (sampling.py, controllable_generation.py, dpm_solver.py, adaptive_sde.py) --------------------
def require(has, header, entries, user):
  """The bound library, which must implement the optional header `header` (``has``: its StkLib attribute, engine/lib.py
  OPTIONAL_HEADERS); NotImplementedError otherwise.  user: who needs `entries`, e.g. 'the DPM-Solver++ sampler needs'."""
  lib = _backend.get()
  if not getattr(lib, has):
    raise NotImplementedError(f'{lib.path} ({lib.backend}) does not implement include/{header}: {user} {entries} '
                              f'(there is no other path)')
  return lib


@contextlib.contextmanager
def sampling_run(model, mode=None):
  """Context of one sampling run on fixed weights: ``torch.no_grad``, the convolution weights prepared once
  (:func:`frozen_weights`) and, unless `mode` is None, the network evaluations in precision `mode` (:func:`precision`).
  Inside it a sampler builds its score function, draws the prior and loops, in that order."""
  with torch.no_grad(), frozen_weights(model), contextlib.nullcontext() if mode is None else precision(model, mode):
    yield


def score_and_prior(config, sde, model, shape, device, lib):
  """(score_fn, x): the score function of `model` and ONE ``sde.prior_sampling(shape)`` as a contiguous tensor on `device`,
  which must be the library's."""
  score_fn = get_score_fn(config, sde, model, train=False, continuous=config.training.continuous)
  x = sde.prior_sampling(shape).to(device).contiguous()
  _backend.check(x, lib)
  return score_fn, x


def check_inplace_state(x, lib, why='it is updated in place'):
  """The state a loop advances in place (or an operand the kernels take as it lies): on the library's device, contiguous,
  float32."""
  _backend.check(x, lib)
  if x.dtype != torch.float32 or not x.is_contiguous():
    raise ValueError(f'x must be a contiguous float32 tensor ({why}), got {x.dtype}, strides {x.stride()}')


def checked_score(score_fn, x, t, lib):
  """``score_fn(x, t)``, which must be a float32 tensor of x's shape on the library's device, made contiguous."""
  score = score_fn(x, t)
  _backend.check(score, lib)
  if score.shape != x.shape or score.dtype != torch.float32:
    raise ValueError(f'score_fn returned {score.dtype} {tuple(score.shape)} for a float32 state {tuple(x.shape)}')
  return score.contiguous()


def fp32_levels(v):
  """`v` rounded to fp32 and held as float64 numpy: the levels a schedule computes its float64 coefficients at."""
  return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def optional_ptr(t):
  """The device pointer of an optional operand: None (null) where it is absent."""
  return None if t is None else t.data_ptr()


def level_conditioning(levels, B, device):
  """[len(levels), B] fp32 on `device`: row j conditions evaluation j of a run on a batch of B, one host-to-device copy."""
  return torch.tensor(levels, dtype=torch.float32).to(device)[:, None].expand(-1, B).contiguous()


def get_model_fn(model, train=False):
  """Callable running the model in train or eval mode, re-asserted on every call (models/utils.py:97-126)."""

  def model_fn(x, labels):
    model.train() if train else model.eval()
    return model(x, labels)

  return model_fn


def _vp_time_labels(config, sde, t):
  """Conditioning of a continuously-trained VP network: 999 t, or the unbounded parametrisation that rescales the
  antiderivative of g^2/sigma^2 onto [0, 999] (models/utils.py:149-154)."""
  tr = config.training
  if not tr.unbounded_parametrization:
    return t * 999
  sc = tr.stabilizing_constant
  a0 = sde.antiderivative(1e-5, stabilizing_constant=sc)
  return (sde.antiderivative(t, stabilizing_constant=sc) - a0) / (sde.antiderivative(sde.T, stabilizing_constant=sc) - a0) * 999.


def _vp_score_fn(config, sde, model_fn, continuous):
  sub = isinstance(sde, sde_lib.subVPSDE)

  def score_fn(x, t, logsnr_model=None, logsnr=None):
    if continuous or sub:
      labels = _vp_time_labels(config, sde, t)
      std = sde.marginal_prob(torch.zeros_like(x), t)[1]
      out = model_fn(x, labels)
    else:                                           # discrete DDPM ladder
      labels = t * (sde.N - 1)
      out = model_fn(x, labels)
      std = sde.sqrt_1m_alphas_cumprod.to(labels.device)[labels.long()]
    return - out / std[:, None, None, None] if config.training.ddpm_score else out

  return score_fn


def _ve_score_fn(sde, model_fn, continuous):
  def score_fn(x, t):
    if continuous:
      labels = sde.marginal_prob(torch.zeros_like(x), t)[1]          # sigma(t)
    else:
      labels = sde.T - t
      labels *= sde.N - 1
      labels = torch.round(labels).long()
    return model_fn(x, labels)

  return score_fn


# ---- the EDM formulation (sde_lib.EDM, include/stk_edm.h) ---------------------------------------------------------------------
EDM_TRAINING_REFUSED = ('mixed', 'importance_sampling', 'likelihood_weighting', 'reconstruction_loss')


def check_edm_config(config, training=False):
  """What sde_lib.EDM asks of a config, checked when a score function, a loss, a step function or a sampler is built on it;
  ValueError naming the key.  ``data.centered`` must be true (the network recentres uncentred data itself, which it would
  apply to c_in x), ``model.scale_by_sigma`` false (the denoiser's c_out is the output scale) and ``training.continuous``
  true; training: ``training.mixed / importance_sampling / likelihood_weighting / reconstruction_loss`` must all be off
  (they belong to the Soft-Truncation objective)."""
  if not config_option(config, 'data', 'centered', False):
    raise ValueError('the EDM formulation needs config.data.centered = True: the network would recentre c_in x itself')
  if config_option(config, 'model', 'scale_by_sigma', False):
    raise ValueError('the EDM formulation needs config.model.scale_by_sigma = False: c_out is the output scale of the denoiser')
  if not config_option(config, 'training', 'continuous', True):
    raise ValueError('the EDM formulation needs config.training.continuous = True: the noise level is a continuous time')
  if training:
    for key in EDM_TRAINING_REFUSED:
      if config_option(config, 'training', key, False):
        raise ValueError(f'the EDM loss does not take config.training.{key}: it belongs to the Soft-Truncation objective')


def edm_coefficients(sigma, sigma_data):
  """The six rows of include/stk_edm.h -- c_in, c_in sigma, c_skip, c_out, lambda = 1 / c_out^2, c_noise = ln(sigma) / 4 -- of
  the [B] tensor `sigma`, in float64 in the header's operation order; the caller rounds them."""
  S, d = sigma.double(), float(sigma_data)
  v = S * S + d * d
  q = torch.sqrt(v)
  p = S * d
  return 1. / q, S / q, (d * d) / v, p / q, v / (p * p), torch.log(S) / 4.


def get_edm_model_fn(config, model, train=False):
  """``F(x_in, c_noise)``: the raw network under the EDM conditioning c_noise = ln(sigma) / 4 ([B] fp32) -- handed over as it
  is for ``embedding_type = 'positional'``, as exp(c_noise) for 'fourier', whose forward takes the log itself."""
  model_fn = get_model_fn(model, train=train)
  if config.model.embedding_type.lower() == 'fourier':
    return lambda x_in, c_noise: model_fn(x_in, torch.exp(c_noise))
  return model_fn


def ct_coefficients(sigma, sigma_data, sigma_min):
  """The five rows of one level of include/stk_consistency.h -- c_in, c_in sigma, c_skip, c_out, c_noise = ln(sigma) / 4 of the
  consistency function, whose c_skip = 1 and c_out = 0 at sigma = sigma_min -- of the [B] tensor `sigma`, in float64 in the
  header's operation order; the caller rounds them."""
  S, d, e = sigma.double(), float(sigma_data), float(sigma_min)
  v = S * S + d * d
  q = torch.sqrt(v)
  g = S - e
  w = g * g + d * d
  return 1. / q, S / q, (d * d) / w, (d * g) / q, torch.log(S) / 4.


def ct_sigma_min(sde):
  """sigma_min as the kernels and the levels carry it: rounded to fp32, so that the lowest level meets it exactly."""
  return float(np.float32(sde.sigma_min))


def get_consistency_fn(config, sde, model, train=False):
  """``f(x, sigma) = c_skip x + c_out F(c_in x; c_noise)``: the consistency function around the raw network (consistency.py,
  include/stk_consistency.h) at the [B] levels `sigma`, by torch operators -- autograd sees it -- for users' own loops.  The
  network is conditioned exactly as :func:`get_edm_model_fn` does; f(x, sigma_min) = x."""
  if not isinstance(sde, sde_lib.EDM):
    raise ValueError(f'the consistency function needs sde_lib.EDM (config.training.sde = \'edm\'), got {type(sde).__name__}')
  check_edm_config(config)
  F = get_edm_model_fn(config, model, train)
  s, e = float(sde.sigma_data), ct_sigma_min(sde)

  def consistency_fn(x, sigma):
    c_in, _, c_skip, c_out, c_noise = (v.to(torch.float32) for v in ct_coefficients(sigma, s, e))
    out = F(c_in[:, None, None, None] * x, c_noise)
    return c_skip[:, None, None, None] * x + c_out[:, None, None, None] * out

  return consistency_fn


def _edm_score_fn(config, sde, model, train):
  """score(x, sigma) = (D(x; sigma) - x) / sigma^2 = -c_in^2 x + (s c_in / sigma) F(c_in x; c_noise), by torch operators
  (autograd sees it: the likelihood, DPS and class_condition work as for the other families).  Classifier-free guidance acts
  on F inside the model; D is affine in it."""
  check_edm_config(config)
  F = get_edm_model_fn(config, model, train)
  s = float(sde.sigma_data)

  def score_fn(x, t):
    sigma = t.to(x.dtype)
    c_in = 1. / torch.sqrt(sigma * sigma + s * s)
    out = F(c_in[:, None, None, None] * x, (torch.log(sigma) / 4.).to(torch.float32))
    return -(c_in * c_in)[:, None, None, None] * x + (s * c_in / sigma)[:, None, None, None] * out

  return score_fn


# ---- rectified flow (sde_lib.RectifiedFlow, include/stk_flow.h) ------------------------------------------------------------------
def check_flow_config(config, training=False):
  """What sde_lib.RectifiedFlow asks of a config, checked when a velocity or score function, a loss, a step function or a
  sampler is built on it; ValueError naming the key.  ``model.scale_by_sigma`` must be false (the velocity is the network's
  output as it is) and ``training.continuous`` true; training: ``training.mixed / importance_sampling / likelihood_weighting
  / reconstruction_loss`` must all be off (they belong to the Soft-Truncation objective).  Centred and uncentred data are both
  allowed: the network recentres x_t as it does for VP."""
  if config_option(config, 'model', 'scale_by_sigma', False):
    raise ValueError('rectified flow needs config.model.scale_by_sigma = False: the velocity is the output of the network')
  if not config_option(config, 'training', 'continuous', True):
    raise ValueError('rectified flow needs config.training.continuous = True: the time of the interpolant is continuous')
  if training:
    for key in EDM_TRAINING_REFUSED:
      if config_option(config, 'training', key, False):
        raise ValueError(f'the flow loss does not take config.training.{key}: it belongs to the Soft-Truncation objective')


def get_flow_model_fn(config, model, train=False):
  """``v(x, t)``: the raw network as the velocity of the interpolant at the [B] times `t` -- conditioned on 999 t for
  ``embedding_type = 'positional'`` (the range of the VP labels), on t itself for 'fourier', whose forward takes the log.
  Classifier-free guidance, guidance rescale and augmentation labels act inside the model.  ValueError for a config the family
  refuses (:func:`check_flow_config`)."""
  check_flow_config(config)
  model_fn = get_model_fn(model, train=train)
  if config.model.embedding_type.lower() == 'fourier':
    return model_fn
  return lambda x, t: model_fn(x, t * 999)


get_velocity_fn = get_flow_model_fn


def _flow_score_fn(config, model, train):
  """score(x, t) = -(x + (1 - t) v(x, t)) / t of the Gaussian bridge x_t = (1 - t) x_0 + t z, by torch operators (autograd
  sees it).  Valid for 0 < t <= 1."""
  v = get_flow_model_fn(config, model, train)

  def score_fn(x, t):
    tt = t.to(x.dtype)[:, None, None, None]
    return -(x + (1. - tt) * v(x, t)) / tt

  return score_fn


def get_raw_fn(config, sde, model, train=False, continuous=False):
  """The pieces of :func:`get_score_fn` for callers that fuse what follows the network (losses.py's fused loss path):
  ``raw_fn(x, t) -> network output`` with exactly the conditioning labels `get_score_fn` computes, and ``neg_over_std``:
  whether the score is ``-output / std(t)`` (VP family with ``training.ddpm_score``) or the output itself.  Returns
  ``(None, None)`` for the combinations it does not cover (discrete ladders).  sde_lib.EDM: ``raw_fn(x_in, sigma) = F``, the
  network on an input the caller has scaled by c_in already (the score is :func:`get_score_fn`'s, not the output);
  sde_lib.RectifiedFlow: ``raw_fn(x, t) = v``, the velocity (likewise)."""
  model_fn = get_model_fn(model, train=train)
  if isinstance(sde, sde_lib.RectifiedFlow):
    return get_flow_model_fn(config, model, train), False
  if isinstance(sde, sde_lib.EDM):
    check_edm_config(config)
    F = get_edm_model_fn(config, model, train)
    return (lambda x_in, t: F(x_in, (torch.log(t) / 4.).to(torch.float32))), False
  if isinstance(sde, (sde_lib.VPSDE, sde_lib.subVPSDE)):
    if not (continuous or isinstance(sde, sde_lib.subVPSDE)):
      return None, None
    return (lambda x, t: model_fn(x, _vp_time_labels(config, sde, t))), bool(config.training.ddpm_score)
  if isinstance(sde, (sde_lib.VESDE, sde_lib.reciprocal_VESDE)) and continuous:
    tiny = lambda x: torch.zeros((x.shape[0], 1, 1, 1), dtype=x.dtype, device=x.device)
    return (lambda x, t: model_fn(x, sde.marginal_prob(tiny(x), t)[1])), False      # labels = sigma(t)
  return None, None


def get_score_fn(config, sde, model, train=False, continuous=False):
  """Turn the raw network into a score function s(x, t) (models/utils.py:128-190).

  VP / subVP: labels = 999 t (continuous), score = -net/std when ``training.ddpm_score``;
  VE / RVE:   labels = sigma(t) (continuous), the network output is already the score;
  EDM:        t = sigma, score = (D(x; sigma) - x) / sigma^2 of the preconditioned denoiser D;
  RectifiedFlow: score = -(x + (1 - t) v(x, t)) / t of the velocity v, for 0 < t <= 1."""
  if isinstance(sde, sde_lib.EDM):
    return _edm_score_fn(config, sde, model, train)
  if isinstance(sde, sde_lib.RectifiedFlow):
    return _flow_score_fn(config, model, train)
  model_fn = get_model_fn(model, train=train)
  if isinstance(sde, (sde_lib.VPSDE, sde_lib.subVPSDE)):
    return _vp_score_fn(config, sde, model_fn, continuous)
  if isinstance(sde, (sde_lib.VESDE, sde_lib.reciprocal_VESDE)):
    return _ve_score_fn(sde, model_fn, continuous)
  raise NotImplementedError(f"SDE class {sde.__class__.__name__} not yet supported.")


def to_flattened_numpy(x):
  return x.detach().cpu().numpy().reshape((-1,))


def from_flattened_numpy(x, shape):
  return torch.from_numpy(x.reshape(shape))
