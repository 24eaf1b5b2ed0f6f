"""Training objective and the one-step training function (reference: losses.py).

Interface kept verbatim: ``get_optimizer(config, params)`` (:29-41), ``optimization_manager(config)``
-> ``optimize_fn(optimizer, params, step, lr, warmup, grad_clip)`` (:44-58),
``get_sde_loss_fn`` (:61-168), ``get_smld_loss_fn`` (:171-192), ``get_ddpm_loss_fn`` (:195-215),
``get_step_fn(config, sde, train, optimize_fn=None)`` -> ``step_fn(state, batch)`` returning the
per-sample losses as a CPU tensor and mutating ``state`` in place (:218-325).

What changes underneath: the score network is one planned HIP graph instead of
37.7k eager ops; ``optimizer`` is ``engine.optim.FusedAdam`` (clip + Adam in two launches, norm
kept on the device); the EMA update is one launch; and with ``torch.distributed`` initialised the
gradients are averaged by a bucketed RCCL all-reduce inside ``optimize_fn``.

The soft-truncation loss itself (time sampling, perturbation, weighting) is per-sample scalar
math plus a few element-wise passes over the [B,3,H,W] batch; it is written with the same torch
expression order as the reference so results are bit-identical on identical inputs.
"""
import contextlib
import os

import numpy as np
import torch
import torch.optim as optim

from . import _decoder
from .engine import ddp
from .engine.flat import flat_of
from .engine.optim import FusedAdam
from .models import utils as mutils
from .sde_lib import EDM, VESDE, VPSDE, RectifiedFlow, reciprocal_VESDE


def _wide(v):
  return v[:, None, None, None]


def _per_sample_reducer(config):
  """mean over CHW when ``training.reduce_mean`` else half the sum (losses.py:77)."""
  if config.training.reduce_mean:
    return torch.mean
  return lambda *args, **kwargs: 0.5 * torch.sum(*args, **kwargs)


# optimizer name -> (second Adam beta, decoupled weight decay); losses.py:31-39
_OPTIMIZERS = {'Adam': (0.999, False), 'AdamW': (0.99, True)}


def get_optimizer(config, params):
  """Adam / AdamW per ``config.optim`` (losses.py:29-41).  Flat-backed parameters (the score network) get the fused
  HIP optimizer; other parameter lists get torch's."""
  params, o = list(params), config.optim
  if o.optimizer not in _OPTIMIZERS:
    raise NotImplementedError(f'Optimizer {o.optimizer} not supported yet!')
  beta2, decoupled = _OPTIMIZERS[o.optimizer]
  common = dict(lr=o.lr, betas=(o.beta1, beta2), eps=o.eps, weight_decay=o.weight_decay)
  if flat_of(params) is not None:
    return FusedAdam(params, adamw=True, **common) if decoupled else FusedAdam(params, amsgrad=o.amsgrad, **common)
  return optim.AdamW(params, **common) if decoupled else optim.Adam(params, amsgrad=o.amsgrad, **common)


def optimization_manager(config):
  """optimize_fn: lr warm-up, gradient exchange (multi-GPU), clipping, optimizer step (losses.py:44-58)."""

  def optimize_fn(optimizer, params, step, lr=config.optim.lr, warmup=config.optim.warmup,
                  grad_clip=config.optim.grad_clip):
    fused = hasattr(optimizer, 'clip_grad_norm')
    # a generator would be exhausted by the first consumer below; the fused optimizer works on its flat buffers and needs
    # no list at all (walking the module tree of the 61.8 M-parameter net is ~0.9 ms of host time)
    params = None if fused else list(params)
    if warmup > 0:
      warm_lr = lr * np.minimum(step / warmup, 1.0)
      for group in optimizer.param_groups:
        group['lr'] = warm_lr
    ddp.sync_gradients(optimizer, None if fused else params)
    if grad_clip >= 0:
      if fused:
        optimizer.clip_grad_norm(grad_clip)      # norm stays on the device, folded into the Adam launch
      else:
        torch.nn.utils.clip_grad_norm_(params, max_norm=grad_clip)
    optimizer.step()

  return optimize_fn


# STK_FUSED_LOSS=0: the loss arithmetic around the network as the reference's torch expressions (~35 small launches per
# evaluation and as many in its backward) instead of three kernels (A/B switch; results agree to the last bits)
FUSED_LOSS = os.environ.get('STK_FUSED_LOSS', '1') != '0'


class _ScoreMatching(torch.autograd.Function):
  """losses[n] = wgt[n] * reduce((score * std + z)^2) with score = -net / std (VP) or net -- the tail of the reference's
  loss_fn (losses.py:122-132 behind models/utils.py:160) as ONE kernel per direction (stk_sm_loss_*) on the raw network
  output, every element-wise operation rounded as torch rounds it.

  The forward kernel gives a sample to one workgroup: fine for 128 x 3072 (CIFAR-10), 614 us for 4 x 196608 (256 x 256 at
  batch 4).  Large samples are therefore cut into `S` equal pieces that the kernel sees as samples of their own (half the
  sum of squares each, `reduce_mean` off); the pieces of a sample are added here in a fixed order."""

  PIECE = 16384          # elements per workgroup when a sample is cut up

  @staticmethod
  def _pieces(B, inner):
    S = 1
    while inner // S > _ScoreMatching.PIECE and (inner // S) % 8 == 0 and B * S < 4096:
      S *= 2
    return S

  @staticmethod
  def forward(ctx, net, z, std, wgt, lib, neg_over_std, reduce_mean):
    from .engine import lib as stk_lib
    net, z, std, wgt = net.contiguous(), z.contiguous(), std.contiguous(), wgt.contiguous()
    B, inner = net.shape[0], net[0].numel()
    S = _ScoreMatching._pieces(B, inner)
    stdS = std.repeat_interleave(S) if S > 1 else std
    wgtS = wgt.repeat_interleave(S) if S > 1 else wgt
    rm = int(reduce_mean) if S == 1 else 0
    part = torch.empty(B * S, dtype=torch.float32, device=net.device)
    with stk_lib.device_guard(net.device):
      lib.sm_loss_fwd_f32(net.data_ptr(), z.data_ptr(), stdS.data_ptr(), wgtS.data_ptr(), part.data_ptr(), B * S, inner // S,
                          int(neg_over_std), 0, rm, stk_lib.stream_ptr(net.device))
    if S > 1:
      losses = part.view(B, S).sum(dim=1)                 # = wgt * 0.5 * sum r^2
      if reduce_mean:
        losses = losses * (2.0 / inner)
    else:
      losses = part
    ctx.save_for_backward(net, z, stdS, wgtS)
    ctx.args = (lib, B, inner, S, int(neg_over_std), int(reduce_mean))
    return losses

  @staticmethod
  def backward(ctx, dloss):
    from .engine import lib as stk_lib
    net, z, stdS, wgtS = ctx.saved_tensors
    lib, B, inner, S, vp, reduce_mean = ctx.args
    dnet = torch.empty_like(net)
    dloss = dloss.contiguous()
    rm = reduce_mean
    if S > 1:
      dloss = (dloss * (2.0 / inner) if reduce_mean else dloss).repeat_interleave(S)
      rm = 0
    with stk_lib.device_guard(net.device):
      lib.sm_loss_bwd_f32(net.data_ptr(), z.data_ptr(), stdS.data_ptr(), wgtS.data_ptr(), dloss.data_ptr(), dnet.data_ptr(),
                          B * S, inner // S, vp, 0, rm, stk_lib.stream_ptr(net.device))
    return dnet, None, None, None, None, None, None


_fused_bufs = {}


def _engine_lib(model, batch):
  """The kernel library of a score network that runs on the engine, when `batch` lives where that library computes."""
  net = getattr(model, 'module', model)
  engine = getattr(net, 'engine', None)
  if engine is None:
    return None
  lib = engine().lib
  if lib.is_device != batch.is_cuda or batch.dtype != torch.float32:
    return None
  return lib


def get_sde_loss_fn(config, sde, train, variance='scoreflow'):
  """Soft-truncation weighted denoising score matching for a continuous SDE (losses.py:61-168):
  ``loss_fn(model, batch, importance_sampling, t_min=None) -> [B]``."""
  tr = config.training
  reduce_op = _per_sample_reducer(config)

  def score_matching(batch, t, Z, z, std, score):
    if tr.importance_sampling or not tr.likelihood_weighting:
      sq = torch.square(score * _wide(std) + z)
      return 0.5 * Z * reduce_op(sq.reshape(sq.shape[0], -1), dim=-1)
    g2 = sde.sde(torch.zeros_like(batch), t)[1] ** 2
    sq = torch.square(score + z / _wide(std))
    return 0.5 * Z * reduce_op(sq.reshape(sq.shape[0], -1), dim=-1) * g2

  def reconstruction(score_fn, batch, t_min, losses):
    """Decoder term at the truncation time (losses.py:134-164; off in every BASELINE config)."""
    std, q_mean, q_std = _decoder.posterior_at(sde, score_fn, batch, t_min, variance)
    if config.data.dequantization == 'lossless':
      nll = -_decoder.discretized_gaussian_log_likelihood(batch, means=q_mean, log_scales=_wide(torch.log(q_std)))
      term = nll.sum(axis=(1, 2, 3))
    else:
      p_entropy = _decoder.entropy_of_perturbation(np.prod(batch.shape[1:]), std)
      q_recon = _decoder.gaussian_reconstruction(batch, q_mean, q_std)
      assert q_recon.shape == p_entropy.shape == torch.Size([batch.shape[0]])
      term = q_recon - p_entropy
      assert losses.shape == term.shape
    return term / np.prod(list(batch.shape[1:])) if tr.reduce_mean else term

  def fused_losses(lib, raw_fn, neg_over_std, batch, t, Z):
    """The same values from three kernels: x_t = mean + std z (stk_perturb_f32, bit-identical to the torch expression),
    the network, the weighted squared residual per sample (stk_sm_loss_fwd_f32 / _bwd_f32)."""
    from .engine import lib as stk_lib
    B = batch.shape[0]
    z = torch.randn_like(batch)
    key = (B, batch.dtype, batch.device)
    bufs = _fused_bufs.get(key)
    if bufs is None:       # per batch size: the [B,1,1,1] ones the coefficients are read off (never written again)
      bufs = _fused_bufs[key] = torch.ones((B, 1, 1, 1), dtype=batch.dtype, device=batch.device)
    ones = bufs
    coeff, std = sde.marginal_prob(ones, t)                    # mean = coeff * x: [B,1,1,1] coefficients, [B] std
    std = std.to(torch.float32).contiguous()
    x = batch.contiguous()
    xt = torch.empty_like(x)
    a = None if isinstance(sde, (VESDE, reciprocal_VESDE)) else coeff.reshape(B).to(torch.float32).contiguous()
    with stk_lib.device_guard(x.device):
      lib.perturb_f32(x.data_ptr(), z.data_ptr(), a.data_ptr() if a is not None else None, std.data_ptr(), xt.data_ptr(),
                      B, x[0].numel(), stk_lib.stream_ptr(x.device))
    net = raw_fn(xt, t)
    if torch.is_tensor(Z) and Z.device.type != 'cpu':
      wgt = (0.5 * Z) * torch.ones(B, dtype=torch.float32, device=x.device)
    else:                  # a host scalar (the normalising constant of the importance-sampled times): a fill, no host-to-device
      # copy.  (A fresh tensor per evaluation: the autograd node keeps it, and `training.mixed` holds two evaluations at once.)
      wgt = torch.full((B,), 0.5 * float(Z), dtype=torch.float32, device=x.device)
    return _ScoreMatching.apply(net, z, std, wgt, lib, neg_over_std, bool(tr.reduce_mean))

  def loss_fn(model, batch, importance_sampling, t_min=None):
    if t_min is None:
      t_min = sde.get_t_min(config)
    t, Z = sde.get_diffusion_time(config, batch.shape[0], batch.device, t_min, importance_sampling=importance_sampling)
    if FUSED_LOSS and not tr.reconstruction_loss and (tr.importance_sampling or not tr.likelihood_weighting):
      lib = _engine_lib(model, batch)
      raw_fn, neg_over_std = mutils.get_raw_fn(config, sde, model, train=train, continuous=tr.continuous) if lib is not None else (None, None)
      if raw_fn is not None:
        return fused_losses(lib, raw_fn, neg_over_std, batch, t, Z)
    score_fn = mutils.get_score_fn(config, sde, model, train=train, continuous=tr.continuous)
    z = torch.randn_like(batch)
    mean, std = sde.marginal_prob(batch, t)
    score = score_fn(mean + _wide(std) * z, t)
    losses = score_matching(batch, t, Z, z, std, score)
    if tr.reconstruction_loss:
      losses = losses + reconstruction(score_fn, batch, t_min, losses)
    return losses

  return loss_fn


def get_smld_loss_fn(config, vesde, train):
  """Legacy discrete SMLD objective (losses.py:171-192); unreachable with continuous configs."""
  assert isinstance(vesde, VESDE), "SMLD training only works for VESDEs."
  descending = torch.flip(vesde.discrete_sigmas, dims=(0,))
  reduce_op = _per_sample_reducer(config)

  def loss_fn(model, batch):
    model_fn = mutils.get_model_fn(model, train=train)
    labels = torch.randint(0, vesde.N, (batch.shape[0],), device=batch.device)
    sigmas = descending.to(batch.device)[labels]
    noise = torch.randn_like(batch) * _wide(sigmas)
    score = model_fn(noise + batch, labels)
    sq = torch.square(score - (-noise / _wide(sigmas ** 2)))
    return torch.mean(reduce_op(sq.reshape(sq.shape[0], -1), dim=-1) * sigmas ** 2)

  return loss_fn


def get_ddpm_loss_fn(config, vpsde, train):
  """Legacy discrete DDPM objective (losses.py:195-215); unreachable with continuous configs."""
  assert isinstance(vpsde, VPSDE), "DDPM training only works for VPSDEs."
  reduce_op = _per_sample_reducer(config)

  def loss_fn(model, batch):
    model_fn = mutils.get_model_fn(model, train=train)
    labels = torch.randint(0, vpsde.N, (batch.shape[0],), device=batch.device)
    keep = vpsde.sqrt_alphas_cumprod.to(batch.device)
    blur = vpsde.sqrt_1m_alphas_cumprod.to(batch.device)
    noise = torch.randn_like(batch)
    noisy = keep[labels, None, None, None] * batch + blur[labels, None, None, None] * noise
    sq = torch.square(model_fn(noisy, labels) - noise)
    return torch.mean(reduce_op(sq.reshape(sq.shape[0], -1), dim=-1))

  return loss_fn


class _KeptResidual(torch.autograd.Function):
  """What the squared-residual losses share (csrc/sqloss.h): the loss launch keeps its residual r when the raw network output F
  needs a gradient, and the backward is the gradient launch IN PLACE on that r, so a second backward through the same
  evaluation is refused.  A subclass names itself (NAME, WS_QUERY) and gives the two launches."""

  @classmethod
  def keep(cls, ctx, lib, F, launch):
    """The forward: ``launch(ws, r, losses, B, inner, stream)`` -> what the gradient launch needs beside r."""
    from .engine import lib as stk_lib
    B, inner = F.shape[0], F[0].numel()
    key = (cls.WS_QUERY, B, inner, F.device)
    ws = _fused_bufs.get(key)
    if ws is None:       # per batch shape: the partial sums, consumed by the finishing pass of the same call
      ws_bytes = int(getattr(lib, cls.WS_QUERY)(B, inner))
      if ws_bytes < 0:
        raise ValueError(f'stk_{cls.WS_QUERY} refuses a batch of {B} rows of {inner} (rc={ws_bytes})')
      ws = _fused_bufs[key] = torch.empty(ws_bytes, dtype=torch.uint8, device=F.device)
    r = torch.empty_like(F) if ctx.needs_input_grad[0] else None
    losses = torch.empty(B, dtype=torch.float32, device=F.device)
    with stk_lib.device_guard(F.device):
      extras = launch(ws, r, losses, B, inner, stk_lib.stream_ptr(F.device))
    ctx.args = (lib, B, inner, r, extras)
    return losses

  @classmethod
  def spend(cls, ctx, dloss, launch_grad):
    """The backward: ``launch_grad(lib, r, extras, dloss, B, inner, stream)`` writes dF over r, which is returned."""
    from .engine import lib as stk_lib
    lib, B, inner, r, extras = ctx.args
    if r is None:
      raise RuntimeError(f'the {cls.NAME} loss kept its residual once: a second backward through the same evaluation is not '
                         f'possible')
    ctx.args = (lib, B, inner, None, None)
    with stk_lib.device_guard(r.device):
      launch_grad(lib, r, extras, dloss.contiguous(), B, inner, stk_lib.stream_ptr(r.device))
    return r


class _EdmLoss(_KeptResidual):
  """losses[b] = lambda_b * reduce(r^2), r = c_skip (y + sigma n) + c_out F - y: the tail of the EDM loss on the raw network
  output F as stk_edm_loss_f32 (include/stk_edm.h), whose residual r is kept; the backward is stk_edm_loss_grad_f32 on that r
  (24 B per element for the pair)."""
  NAME, WS_QUERY = 'EDM', 'edm_ws_bytes'

  @staticmethod
  def forward(ctx, F, y, n, sigma, coef, lib, reduce_mean):
    F, y, n = F.contiguous(), y.contiguous(), n.contiguous()

    def launch(ws, r, losses, B, inner, stream):
      lib.edm_loss_f32(F.data_ptr(), y.data_ptr(), n.data_ptr(), sigma.data_ptr(), coef.data_ptr(), ws.data_ptr(), ws.numel(),
                       mutils.optional_ptr(r), losses.data_ptr(), B, inner, int(reduce_mean), stream)
      return coef, int(reduce_mean)

    return _EdmLoss.keep(ctx, lib, F, launch)

  @staticmethod
  def backward(ctx, dloss):
    def launch_grad(lib, r, extras, dloss, B, inner, stream):
      coef, reduce_mean = extras
      lib.edm_loss_grad_f32(r.data_ptr(), coef.data_ptr(), dloss.data_ptr(), r.data_ptr(), B, inner, reduce_mean, stream)

    return (_EdmLoss.spend(ctx, dloss, launch_grad),) + (None,) * 6


def get_edm_loss_fn(config, sde, train):
  """The EDM training loss (Karras et al. 2022, Table 1 "Ours"): ``loss_fn(model, batch, importance_sampling=None, t_min=None)
  -> [B]``, both keywords accepted and unused.  Per evaluation, in this order: ``torch.randn(B)`` for ln sigma = P_mean +
  P_std randn (``training.edm_p_mean`` = -1.2, ``training.edm_p_std`` = 1.2 where absent), then ``torch.randn_like(batch)``
  for n.  With the coefficients of include/stk_edm.h,

    x_in = c_in y + (c_in sigma) n;  F = network(x_in, c_noise);  r = c_skip (y + sigma n) + c_out F - y;
    loss[b] = lambda_b sum r^2   (the mean over C H W under ``training.reduce_mean``)

  every element in fp32 in that order, the squares summed in float64.  On an engine model with a device fp32 batch, a library
  with the header and STK_FUSED_LOSS != 0 this is stk_edm_coeffs_f32, stk_perturb_f32, the network and stk_edm_loss_f32 /
  stk_edm_loss_grad_f32; otherwise the same expressions by torch operators."""
  mutils.check_edm_config(config, training=True)
  if not isinstance(sde, EDM):
    raise ValueError(f'get_edm_loss_fn needs sde_lib.EDM, got {type(sde).__name__}')
  tr = config.training
  p_mean = float(mutils.config_option(config, 'training', 'edm_p_mean', -1.2))
  p_std = float(mutils.config_option(config, 'training', 'edm_p_std', 1.2))
  if not p_std > 0:
    raise ValueError(f'config.training.edm_p_std must be positive, got {p_std!r}')
  s_data = float(sde.sigma_data)
  reduce_mean = bool(tr.reduce_mean)

  def fused_losses(lib, F_fn, batch, sigma, n):
    from .engine import lib as stk_lib
    B = batch.shape[0]
    y = batch.contiguous()
    inner = y[0].numel()
    sigma = sigma.contiguous()
    coef = torch.empty((6, B), dtype=torch.float32, device=y.device)
    x_in = torch.empty_like(y)
    with stk_lib.device_guard(y.device):
      stream = stk_lib.stream_ptr(y.device)
      lib.edm_coeffs_f32(sigma.data_ptr(), s_data, coef.data_ptr(), B, stream)
      lib.perturb_f32(y.data_ptr(), n.data_ptr(), coef[0].data_ptr(), coef[1].data_ptr(), x_in.data_ptr(), B, inner, stream)
    F = F_fn(x_in, coef[5])
    return _EdmLoss.apply(F, y, n, sigma, coef, lib, reduce_mean)

  def torch_losses(F_fn, batch, sigma, n):
    c_in, c_in_sigma, c_skip, c_out, lam, c_noise = (v.to(torch.float32) for v in mutils.edm_coefficients(sigma, s_data))
    x_in = _wide(c_in) * batch + _wide(c_in_sigma) * n
    F = F_fn(x_in, c_noise)
    x = batch + _wide(sigma) * n
    D = _wide(c_skip) * x + _wide(c_out) * F
    r = D - batch
    total = (r * r).double().reshape(r.shape[0], -1).sum(dim=-1)
    total = lam.double() * total
    if reduce_mean:
      total = total / float(np.prod(batch.shape[1:]))
    return total.to(torch.float32)

  def loss_fn(model, batch, importance_sampling=None, t_min=None):
    B = batch.shape[0]
    sigma = torch.exp(p_mean + p_std * torch.randn(B, device=batch.device)).to(torch.float32)
    n = torch.randn_like(batch)
    F_fn = mutils.get_edm_model_fn(config, model, train=train)
    lib = _engine_lib(model, batch) if FUSED_LOSS else None
    if lib is not None and lib.has_edm:
      return fused_losses(lib, F_fn, batch, sigma, n.contiguous())
    return torch_losses(F_fn, batch, sigma, n)

  return loss_fn


class _FlowLoss(_KeptResidual):
  """losses[b] = reduce(r^2), r = F - (n - y): the tail of the rectified-flow loss on the raw network output F as
  stk_flow_loss_f32 (include/stk_flow.h), whose residual r is kept; the backward is stk_flow_loss_grad_f32 on that r (24 B per
  element for the pair)."""
  NAME, WS_QUERY = 'flow', 'flow_ws_bytes'

  @staticmethod
  def forward(ctx, F, y, n, lib, reduce_mean):
    F, y, n = F.contiguous(), y.contiguous(), n.contiguous()

    def launch(ws, r, losses, B, inner, stream):
      lib.flow_loss_f32(F.data_ptr(), y.data_ptr(), n.data_ptr(), ws.data_ptr(), ws.numel(), mutils.optional_ptr(r),
                        losses.data_ptr(), B, inner, int(reduce_mean), stream)
      return int(reduce_mean)

    return _FlowLoss.keep(ctx, lib, F, launch)

  @staticmethod
  def backward(ctx, dloss):
    def launch_grad(lib, r, reduce_mean, dloss, B, inner, stream):
      lib.flow_loss_grad_f32(r.data_ptr(), dloss.data_ptr(), r.data_ptr(), B, inner, reduce_mean, stream)

    return (_FlowLoss.spend(ctx, dloss, launch_grad),) + (None,) * 4


FLOW_TIMES = ('logit_normal', 'uniform')


def get_flow_loss_fn(config, sde, train):
  """The rectified-flow training loss (Liu et al. 2022; the time law of Esser et al. 2024): ``loss_fn(model, batch,
  importance_sampling=None, t_min=None) -> [B]``, both keywords accepted and unused.  Per evaluation, in this order: one [B]
  fp32 draw on the batch's device for the time -- ``training.flow_time = 'logit_normal'`` (the default):
  t = sigmoid(P_mean + P_std torch.randn(B)) with ``training.flow_p_mean`` = 0 and ``training.flow_p_std`` = 1 where absent;
  'uniform': t = 1 - torch.rand(B), which lies in (0, 1] -- then ``torch.randn_like(batch)`` for n.  With a = 1 - t,

    x_t = a y + t n;  F = v(x_t, t);  u = n - y;  r = F - u;  loss[b] = sum r^2   (the mean over C H W under
    ``training.reduce_mean``)

  every element in fp32 in that order, the squares summed in float64; the loss weight is 1.  On an engine model with a device
  fp32 batch, a library with include/stk_flow.h and STK_FUSED_LOSS != 0 this is stk_perturb_f32, the network and
  stk_flow_loss_f32 / stk_flow_loss_grad_f32; otherwise the same expressions by torch operators.  ValueError naming the key:
  a config the family refuses (models.utils.check_flow_config), ``flow_p_std`` <= 0, an unknown ``flow_time``."""
  mutils.check_flow_config(config, training=True)
  if not isinstance(sde, RectifiedFlow):
    raise ValueError(f'get_flow_loss_fn needs sde_lib.RectifiedFlow, got {type(sde).__name__}')
  time_law = mutils.config_option(config, 'training', 'flow_time', 'logit_normal')
  if time_law not in FLOW_TIMES:
    raise ValueError(f'config.training.flow_time must be one of {FLOW_TIMES}, got {time_law!r}')
  p_mean = float(mutils.config_option(config, 'training', 'flow_p_mean', 0.))
  p_std = float(mutils.config_option(config, 'training', 'flow_p_std', 1.))
  if not p_std > 0:
    raise ValueError(f'config.training.flow_p_std must be positive, got {p_std!r}')
  reduce_mean = bool(config.training.reduce_mean)

  def fused_losses(lib, v_fn, batch, t, a, n):
    from .engine import lib as stk_lib
    B = batch.shape[0]
    y = batch.contiguous()
    t, a = t.contiguous(), a.contiguous()
    x_t = torch.empty_like(y)
    with stk_lib.device_guard(y.device):
      lib.perturb_f32(y.data_ptr(), n.data_ptr(), a.data_ptr(), t.data_ptr(), x_t.data_ptr(), B, y[0].numel(),
                      stk_lib.stream_ptr(y.device))
    return _FlowLoss.apply(v_fn(x_t, t), y, n, lib, reduce_mean)

  def torch_losses(v_fn, batch, t, a, n):
    x_t = _wide(a) * batch + _wide(t) * n
    F = v_fn(x_t, t)
    u = n - batch
    r = F - u
    total = (r * r).double().reshape(r.shape[0], -1).sum(dim=-1)
    if reduce_mean:
      total = total / float(np.prod(batch.shape[1:]))
    return total.to(torch.float32)

  def loss_fn(model, batch, importance_sampling=None, t_min=None):
    B = batch.shape[0]
    if time_law == 'uniform':
      t = 1. - torch.rand(B, device=batch.device)
    else:
      t = torch.sigmoid(p_mean + p_std * torch.randn(B, device=batch.device)).to(torch.float32)
    a = 1. - t
    n = torch.randn_like(batch)
    v_fn = mutils.get_flow_model_fn(config, model, train=train)
    lib = _engine_lib(model, batch) if FUSED_LOSS else None
    if lib is not None and lib.has_flow:
      return fused_losses(lib, v_fn, batch, t, a, n.contiguous())
    return torch_losses(v_fn, batch, t, a, n)

  return loss_fn


class _CtLoss(_KeptResidual):
  """losses[b] = lambda_b (sqrt(S + c^2) - c) (/ inner), S = sum r^2, r = f(y + sigma_hi n; sigma_hi) - f(y + sigma_lo n;
  sigma_lo): the tail of the consistency loss on the two raw network outputs as stk_ct_loss_f32 (include/stk_consistency.h),
  which keeps r and the per-sample factor of the gradient; the backward is stk_ct_loss_grad_f32 on that r (28 B per element for
  the pair).  F_lo is the stop-gradient target: it receives no gradient."""
  NAME, WS_QUERY = 'consistency', 'ct_ws_bytes'

  @staticmethod
  def forward(ctx, F_hi, F_lo, y, n, sigma_hi, sigma_lo, coef, huber_c, lib, reduce_mean):
    F_hi, F_lo = F_hi.contiguous(), F_lo.contiguous()

    def launch(ws, r, losses, B, inner, stream):
      gfac = None if r is None else torch.empty(B, dtype=torch.float32, device=F_hi.device)
      lib.ct_loss_f32(F_hi.data_ptr(), F_lo.data_ptr(), y.data_ptr(), n.data_ptr(), sigma_hi.data_ptr(), sigma_lo.data_ptr(),
                      coef.data_ptr(), huber_c, ws.data_ptr(), ws.numel(), mutils.optional_ptr(r), mutils.optional_ptr(gfac),
                      losses.data_ptr(), B, inner, int(reduce_mean), stream)
      return gfac

    return _CtLoss.keep(ctx, lib, F_hi, launch)

  @staticmethod
  def backward(ctx, dloss):
    def launch_grad(lib, r, gfac, dloss, B, inner, stream):
      lib.ct_loss_grad_f32(r.data_ptr(), gfac.data_ptr(), dloss.data_ptr(), r.data_ptr(), B, inner, stream)

    return (_CtLoss.spend(ctx, dloss, launch_grad),) + (None,) * 9


class ConsistencyLoss:
  """What :func:`get_consistency_loss_fn` returns: ``loss_fn(model, batch, importance_sampling=None, t_min=None, levels=None)
  -> [B]`` with the curriculum's state.  ``N``: the number of levels in force;  ``set_step(k)``: N of training step k
  (get_step_fn calls it with ``state['step']`` before the micro-batches), the level grid and the index distribution cached
  per N."""

  def __init__(self, config, sde, train):
    from . import consistency
    mutils.check_edm_config(config, training=True)
    if not isinstance(sde, EDM):
      raise ValueError(f'get_consistency_loss_fn needs sde_lib.EDM, got {type(sde).__name__}')
    self._ct = consistency
    self.config, self.sde, self.train = config, sde, train
    self.p_mean, self.p_std, self.s0, self.s1, huber_c = consistency.training_options(config)
    self.huber_c = huber_c
    self.K = int(mutils.config_option(config, 'training', 'n_iters', 1))
    self.s_data, self.s_min = float(sde.sigma_data), mutils.ct_sigma_min(sde)
    self.reduce_mean = bool(config.training.reduce_mean)
    self._tables = {}       # N -> (levels, pmf), float64 numpy
    self._device = {}       # (N, device) -> (levels fp32, pmf fp32) on the device
    self.step = None
    self.N = None
    self.set_step(0)

  def set_step(self, k):
    self.step = int(k)
    self.N = self._ct.ct_num_levels(self.step, self.K, self.s0, self.s1)
    return self.N

  def tables(self, N=None):
    """(levels [N], pmf [N - 1]) of N levels (the N in force where None), float64 numpy."""
    N = self.N if N is None else N
    hit = self._tables.get(N)
    if hit is None:
      levels = self._ct.ct_levels(self.sde, N)
      hit = self._tables[N] = (levels, self._ct.ct_index_pmf(levels, self.p_mean, self.p_std))
    return hit

  def _on_device(self, device):
    key = (self.N, device)
    hit = self._device.get(key)
    if hit is None:
      levels, pmf = self.tables()
      hit = self._device[key] = (torch.tensor(levels, dtype=torch.float32).to(device), torch.tensor(pmf, dtype=torch.float32).to(device))
    return hit

  def _fused(self, lib, F_fn, batch, sigma_hi, sigma_lo, n, pinned):
    from .engine import lib as stk_lib
    B = batch.shape[0]
    y = batch.contiguous()
    inner = y[0].numel()
    coef = torch.empty((11, B), dtype=torch.float32, device=y.device)
    xin_hi, xin_lo = torch.empty_like(y), torch.empty_like(y)
    with stk_lib.device_guard(y.device):
      stream = stk_lib.stream_ptr(y.device)
      lib.ct_coeffs_f32(sigma_hi.data_ptr(), sigma_lo.data_ptr(), self.s_data, self.s_min, coef.data_ptr(), B, stream)
      lib.ct_pair_f32(y.data_ptr(), n.data_ptr(), coef.data_ptr(), xin_hi.data_ptr(), xin_lo.data_ptr(), B, inner, stream)
    with pinned():
      with torch.no_grad():
        F_lo = F_fn(xin_lo, coef[9])
      F_hi = F_fn(xin_hi, coef[4])
    c = self.huber_c * float(np.sqrt(inner))
    return _CtLoss.apply(F_hi, F_lo, y, n, sigma_hi, sigma_lo, coef, c, lib, self.reduce_mean)

  def _torch(self, F_fn, batch, sigma_hi, sigma_lo, n, pinned):
    f32 = lambda rows: tuple(v.to(torch.float32) for v in rows)
    cin_h, cis_h, csk_h, cou_h, cn_h = f32(mutils.ct_coefficients(sigma_hi, self.s_data, self.s_min))
    cin_l, cis_l, csk_l, cou_l, cn_l = f32(mutils.ct_coefficients(sigma_lo, self.s_data, self.s_min))
    lam = 1. / (sigma_hi.double() - sigma_lo.double())
    with pinned():
      with torch.no_grad():
        F_lo = F_fn(_wide(cin_l) * batch + _wide(cis_l) * n, cn_l)
      F_hi = F_fn(_wide(cin_h) * batch + _wide(cis_h) * n, cn_h)
    f_hi = _wide(csk_h) * (batch + _wide(sigma_hi) * n) + _wide(cou_h) * F_hi
    f_lo = _wide(csk_l) * (batch + _wide(sigma_lo) * n) + _wide(cou_l) * F_lo.detach()
    r = f_hi - f_lo
    inner = float(np.prod(batch.shape[1:]))
    c = float(np.float32(self.huber_c * float(np.sqrt(inner))))
    S = (r * r).double().reshape(r.shape[0], -1).sum(dim=-1)
    total = (lam * S) / (torch.sqrt(S + c * c) + c)
    if self.reduce_mean:
      total = total / inner
    return total.to(torch.float32)

  def __call__(self, model, batch, importance_sampling=None, t_min=None, levels=None):
    B = batch.shape[0]
    if levels is None:
      lv, pmf = self._on_device(batch.device)
      idx = torch.multinomial(pmf, B, replacement=True)
      sigma_hi, sigma_lo = lv[idx + 1], lv[idx]
    else:
      sigma_hi, sigma_lo = (v.to(device=batch.device, dtype=torch.float32).contiguous() for v in levels)
    n = torch.randn_like(batch)
    net = getattr(model, 'module', model)
    uses_dropout = getattr(net, '_uses_dropout', None)
    engine = getattr(net, 'engine', None)
    pinned = contextlib.nullcontext
    if self.train and callable(uses_dropout) and uses_dropout():
      # ONE seed for both evaluations: the student and its stop-gradient target see the same dropout masks
      seed = int(torch.randint(0, 2 ** 62, (1,)).item())
      if callable(engine):
        pinned = lambda: engine().dropout_seed(seed)
    F_fn = mutils.get_edm_model_fn(self.config, model, train=self.train)
    lib = _engine_lib(model, batch) if FUSED_LOSS else None
    if lib is not None and lib.has_consistency:
      return self._fused(lib, F_fn, batch, sigma_hi.contiguous(), sigma_lo.contiguous(), n.contiguous(), pinned)
    return self._torch(F_fn, batch, sigma_hi, sigma_lo, n, pinned)


def get_consistency_loss_fn(config, sde, train):
  """The consistency-training loss of iCT (Song & Dhariwal 2023) on sde_lib.EDM, chosen by ``training.consistency``: a
  :class:`ConsistencyLoss`, ``loss_fn(model, batch, importance_sampling=None, t_min=None, levels=None) -> [B]``, the first two
  keywords accepted and unused.  Per evaluation, in this order: ``torch.multinomial(pmf, B, replacement=True)`` on the batch's
  device for the pair index i (``levels = (sigma_hi, sigma_lo)``, two [B] tensors, replaces this draw), ``torch.randn_like(
  batch)`` for the ONE noise n of both levels, and -- only for a model in training mode that uses dropout -- one
  ``torch.randint(0, 2**62, (1,))``, the dropout seed both evaluations share (``Executor.dropout_seed``).  With the rows of
  include/stk_consistency.h at (sigma_hi, sigma_lo) = (sigma_{i+1}, sigma_i) of the N levels in force,

    F_lo = network(c_in y + (c_in sigma) n, c_noise) at sigma_lo under ``torch.no_grad()``: the stop-gradient target, first;
    F_hi = the same at sigma_hi with gradient: the student (one backward per step);
    r = f(y + sigma_hi n; sigma_hi) - f(y + sigma_lo n; sigma_lo);  S = sum r^2;  lambda = 1 / (sigma_hi - sigma_lo);
    loss[b] = lambda S / (sqrt(S + c^2) + c),  c = ``training.ct_huber_c`` sqrt(C H W)   (/ C H W under ``reduce_mean``)

  every element in fp32 in that order, the squares summed in float64.  On an engine model with a device fp32 batch, a library
  with the header and STK_FUSED_LOSS != 0 this is stk_ct_coeffs_f32, stk_ct_pair_f32, the network twice and stk_ct_loss_f32 /
  stk_ct_loss_grad_f32; otherwise the same expressions by torch operators around any callable network."""
  return ConsistencyLoss(config, sde, train)


def get_loss_fn(config, sde, train):
  """The loss of `sde` under `config`: what get_step_fn evaluates on every chunk."""
  if isinstance(sde, EDM):
    if mutils.config_option(config, 'training', 'consistency', False):
      return get_consistency_loss_fn(config, sde, train)
    return get_edm_loss_fn(config, sde, train)
  if isinstance(sde, RectifiedFlow):
    return get_flow_loss_fn(config, sde, train)
  if config.training.continuous:
    return get_sde_loss_fn(config, sde, train)
  assert not config.training.likelihood_weighting, \
    "Likelihood weighting is not supported for original SMLD/DDPM training."
  if isinstance(sde, VESDE):
    return get_smld_loss_fn(config, sde, train)
  if isinstance(sde, VPSDE):
    return get_ddpm_loss_fn(config, sde, train)
  raise ValueError(f"Discrete training for {sde.__class__.__name__} is not recommended.")


_pick_loss_fn = get_loss_fn      # its name before it was public


# STK_DDP_OVERLAP=0: exchange the gradients after the backward (one bucketed all-reduce) instead of during it
OVERLAP_EXCHANGE = os.environ.get('STK_DDP_OVERLAP', '1') != '0'
# STK_RANGE_CHECK=K: every K-th training step (and the first) the per-image maxima of the fp32 output gradients are computed
# (Executor.dynamic_range_report: one device reduction per 3x3 layer, one transfer) and a warning is issued when an image lies
# more than RANGE_DECADES below the batch maximum of some layer -- beyond that the one-scale-per-tensor split convolutions no
# longer give that image fp32 accuracy.  Unset: every 1000th step for likelihood-weighted losses (g^2 weights spread the
# per-sample gradients over decades, reference losses.py:126-129), never otherwise.  0 = off.  With training.mixed the report
# covers the last network evaluation of the step.
def _env_int(name):
  v = os.environ.get(name)
  if v is None or v.strip() == '':
    return None
  try:
    return int(v)
  except ValueError:
    import warnings
    warnings.warn(f'{name}={v!r} is not an integer: ignored')
    return None


RANGE_CHECK_EVERY = _env_int('STK_RANGE_CHECK')
RANGE_DECADES = 5.0
# STK_ASYNC_LOSS=0: fetch the per-sample losses with a blocking .cpu() after the backward, as the reference does (A/B switch)
ASYNC_LOSS_COPY = os.environ.get('STK_ASYNC_LOSS', '1') != '0'


def _warn_dynamic_range(model, step):
  """See RANGE_CHECK_EVERY."""
  net = getattr(model, 'module', model)
  engine = getattr(net, 'engine', None)
  if engine is None:
    return None
  rows = engine().dynamic_range_report()
  if rows and rows[0][3] > RANGE_DECADES:
    import warnings
    name, hi, lo, dec = rows[0]
    warnings.warn(f'step {step}: the output gradients of {sum(r[3] > RANGE_DECADES for r in rows)} convolution(s) span more than '
                  f'{RANGE_DECADES:g} decades across the images of the batch (worst: {name}, image maxima {lo:.3e} ... {hi:.3e}, '
                  f'{dec:.1f} decades): the split convolutions scale a tensor by one power of two, so the gradient contribution of '
                  f'the faintest images is no longer fp32-accurate (DESIGN.md section 3); a smaller spread of the per-sample loss '
                  f'weights, or STK_PLANES=0 for an exact-fp32 check, tells whether it matters')
  return rows


def _augment_pipe(config):
  """The AugmentPipe of config.training.augment = p > 0 (None when the key is absent or 0), after the checks get_step_fn
  documents."""
  from . import augment
  p = augment.check_probability(mutils.config_option(config, 'training', 'augment', 0) or 0)
  if p == 0:
    return None
  K = int(mutils.config_option(config, 'model', 'augment_dim', 0) or 0)
  if K != augment.NUM_LABELS:
    raise ValueError(f'config.training.augment = {p} needs config.model.augment_dim = {augment.NUM_LABELS} (the labels the '
                     f'pipe produces), got {K}')
  pipe = augment.AugmentPipe(p, augment.check_filter(mutils.config_option(config, 'training', 'augment_filter', None)),
                             seed=int(getattr(config, 'seed', 0) or 0) + ddp.rank())      # offset by rank, as torch's streams are
  size = int(config.data.image_size)
  pipe.check_shape(size, size)
  return pipe


def get_step_fn(config, sde, train, optimize_fn=None):
  """One training step: ``step_fn(state, batch) -> losses`` on the CPU (losses.py:218-325).

  ``state`` = {'model', 'optimizer', 'ema', 'step'}, mutated in place exactly like the reference: zero_grad, one host
  draw of t_min shared by the micro-batches, per-micro-batch loss + backward of its mean, ``optimize_fn``,
  ``step += 1``, EMA update.  With ``training.mixed`` each micro-batch is split in halves -- importance-sampled and
  uniform-time -- combined as L_is + w L_ddpm (optionally balanced by mean(L_is / L_ddpm)), and the function returns
  B/2 losses (losses.py:295-320).

  ``config.training.precision = 'fp16'`` runs every micro-batch, forward and backward, in the engine's fp16 training mode
  (models.utils.training_precision); an absent key means 'fp32', the default path, and any other value raises here.

  A class-conditional model (config.model.num_classes = C > 0) takes ``step_fn(state, batch, classes)``: a [n] integer
  tensor or sequence (C or None: the null class) that follows the images through the micro-batches and the halves of
  ``training.mixed``.  Per evaluated chunk one ``torch.rand(n) < config.training.class_dropout`` (default 0.1; 0 draws
  nothing) is drawn BEFORE the loss's own draws and sends those samples to the null class: the unconditional branch
  classifier-free guidance needs.  The values of a device tensor are not read back (no host synchronisation per step):
  an index outside [0, C] takes the null row in the kernels.  ValueError: a conditional model without classes, an
  unconditional one with classes, classes of another length than the batch.

  ``config.training.augment = p > 0`` (configs.edm_augment; any loss) trains under non-leaky augmentation (augment.py): the
  whole batch goes through ONE launch of stk_aug_warp_f32 before the loss, with per-sample transforms drawn on the host from
  a generator of the pipe's own seeded by ``config.seed`` (the device RNG stream is the unaugmented step's), and the nine
  augmentation labels follow the images through the micro-batches and the halves of ``training.mixed`` as the classes do;
  every network evaluation of a chunk -- both of the consistency loss -- sees that chunk's labels
  (models.utils.augment_condition).  ``config.training.augment_filter``: other symmetric low-pass taps.  ValueError, here:
  p outside [0, 1], ``config.model.augment_dim`` other than 9, images the kernel does not take (even sides in [8, 64]), an
  unsymmetric filter.  Absent or 0: nothing of this exists in the step."""
  precision = mutils.config_training_precision(config)
  pipe = _augment_pipe(config)
  loss_fn = get_loss_fn(config, sde, train)
  tr = config.training
  mixed = bool(tr.mixed)
  class_dropout = float(mutils.config_option(config, 'training', 'class_dropout', 0.1))

  def evaluated(model, chunk, cls, aug=None, **kw):
    """loss_fn on one chunk, under its classes (None: an unconditional model) after label dropout, and under its augmentation
    labels (None: no augmentation)."""
    if aug is not None:
      with mutils.augment_in_force(model, aug):
        return evaluated(model, chunk, cls, **kw)
    if cls is None:
      return loss_fn(model, chunk, **kw)
    if class_dropout > 0:
      cls = cls.masked_fill(torch.rand(cls.shape[0], device=cls.device) < class_dropout, float(mutils.num_classes(model)))
    with mutils.classes_in_force(model, cls):
      return loss_fn(model, chunk, **kw)

  def plain_losses(model, chunk, t_min, cls=None, aug=None):
    return evaluated(model, chunk, cls, aug, importance_sampling=tr.importance_sampling, t_min=t_min)

  def mixed_losses(model, chunk, t_min, cls=None, aug=None):
    half = chunk.shape[0] // 2
    first, second = (lambda v: None if v is None else v[:half]), (lambda v: None if v is None else v[half:])
    l_is = evaluated(model, chunk[:half], first(cls), first(aug), importance_sampling=True, t_min=t_min)
    l_ddpm = evaluated(model, chunk[half:], second(cls), second(aug), importance_sampling=False, t_min=t_min)
    weight = tr.ddpm_weight
    if tr.balanced:
      weight = weight * torch.mean(l_is / l_ddpm).detach().item()
    return l_is + weight * l_ddpm

  micro_losses = mixed_losses if mixed else plain_losses
  staging = {}       # number of losses -> pinned host buffer of the asynchronous device-to-host copy
  range_every = RANGE_CHECK_EVERY if RANGE_CHECK_EVERY is not None else (1000 if getattr(tr, 'likelihood_weighting', False) else 0)

  def step_classes(model, batch, classes):
    """`classes` as the [n] float32 tensor the engine takes, on the batch's device; None for an unconditional model."""
    C = mutils.num_classes(model)
    if C == 0:
      if classes is not None:
        raise ValueError('step_fn was given classes, but the model is not class-conditional (config.model.num_classes)')
      return None
    if classes is None:
      raise ValueError(f'a class-conditional model (config.model.num_classes = {C}) needs step_fn(state, batch, classes)')
    on_device = torch.is_tensor(classes) and classes.device.type != 'cpu'
    cls = mutils.as_class_tensor(classes, C, read_values=not on_device)
    if cls.shape[0] != batch.shape[0]:
      raise ValueError(f'{cls.shape[0]} classes for a batch of {batch.shape[0]} images')
    return cls.to(device=batch.device, dtype=torch.float32)

  def step_fn(state, batch, classes=None):
    model, optimizer = state['model'], state['optimizer']
    if not train:
      # the reference has no evaluation branch either: its `return losses_` raises exactly this (losses.py:279-293)
      raise UnboundLocalError("local variable 'losses_' referenced before assignment")
    cls = step_classes(model, batch, classes)
    aug = None
    if pipe is not None:
      batch, aug = pipe(batch)
    optimizer.zero_grad()
    n, parts = batch.shape[0], config.optim.num_micro_batch
    per = n // parts
    out_per = per // 2 if mixed else per
    losses_ = torch.zeros(n // 2 if mixed else n)
    t_min = sde.get_t_min(config)
    if hasattr(loss_fn, 'set_step'):     # a loss with a curriculum (the consistency loss): the levels of this step
      loss_fn.set_step(state['step'])
    pinned, copied = None, None
    ddp.begin_step(model)
    try:
      for k in range(parts):
        of_chunk = {name: v[per * k: per * (k + 1)] for name, v in (('cls', cls), ('aug', aug)) if v is not None}
        if precision != 'fp32':
          with mutils.training_precision(model, precision):
            losses = micro_losses(model, batch[per * k: per * (k + 1)], t_min, **of_chunk)
        else:
          losses = micro_losses(model, batch[per * k: per * (k + 1)], t_min, **of_chunk)
        if k == parts - 1 and OVERLAP_EXCHANGE:
          # multi-GPU: buckets of the flat gradient buffer are all-reduced as the last backward finishes them (with
          # several network evaluations per loss -- training.mixed -- as the LAST of their backwards does)
          ddp.arm_overlap(model)
        if losses.is_cuda and ASYNC_LOSS_COPY:
          # The reference's `losses.cpu()` (losses.py:288) after the backward makes the host wait for the whole backward
          # and only then launch clip / Adam / EMA and the next step: ~1.5-3 ms of idle GPU per 43 ms step.  The values
          # exist before the backward starts, so copy them to pinned memory asynchronously NOW (in stream order: after
          # the loss kernels, before the backward) and wait for that copy -- not for the backward -- when returning.
          if pinned is None:
            key = (losses_.numel(), losses.device)
            pinned = staging.get(key)
            if pinned is None:
              pinned = staging[key] = torch.empty(losses_.numel(), dtype=torch.float32).pin_memory()
            copied = torch.cuda.Event()
          pinned[out_per * k: out_per * (k + 1)].copy_(losses.detach(), non_blocking=True)
          copied.record(torch.cuda.current_stream(losses.device))     # the stream the copy was issued on
          torch.mean(losses).backward(retain_graph=True)
        else:
          torch.mean(losses).backward(retain_graph=True)
          losses_[out_per * k: out_per * (k + 1)] = losses.cpu().detach()
      optimize_fn(optimizer, model.parameters(), step=state['step'])
    except BaseException:
      ddp.disarm_overlap(model, wait=False)      # a step that raised must not leave its hook armed -- nor wait for its peers
      raise
    ddp.disarm_overlap(model)        # no-op after optimize_fn
    if range_every > 0 and state['step'] % range_every == 0:
      _warn_dynamic_range(model, state['step'])
    state['step'] += 1
    state['ema'].update(model.parameters())
    if pinned is not None:
      copied.synchronize()
      losses_.copy_(pinned)
    return losses_

  return step_fn


def get_div_fn(fn):
  """Hutchinson-Skilling divergence estimator (losses.py:327-338)."""

  def div_fn(x, t, eps):
    with torch.enable_grad():
      projected = torch.sum(fn(x, t) * eps)
      grad = torch.autograd.grad(projected, x)[0]
    return torch.sum(grad * eps, dim=tuple(range(1, len(x.shape))))

  return div_fn
