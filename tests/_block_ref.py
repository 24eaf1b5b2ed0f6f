"""Float64 restatement of the NCSN++ building blocks (models/layerspp.py, models/layers.py NIN, models/up_or_down_sampling.py
Conv2d) in torch.nn.functional, on a module's own parameters cast to double.  The yardstick of tests/test_gpu_blocks.py and
tests/test_blocks_cpu.py; tests/test_blocks_restatement.py pins it to the reference's own blocks.

``run(block, inputs, gout)`` -> (output, {input name: gradient}, {parameter name: gradient}) for the loss sum(out * gout).
Dropout is not restated: the blocks are compared in eval mode (or with p = 0).
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

SQRT2 = float(np.sqrt(2.))


def act_fn(act):
  if type(act) is nn.SiLU:
    return F.silu
  if type(act) is nn.ReLU:
    return F.relu
  if type(act) is nn.LeakyReLU:
    return lambda t: F.leaky_relu(t, act.negative_slope)
  if type(act) is nn.ELU:
    return lambda t: F.elu(t, act.alpha)
  raise ValueError(act)


def fir_taps(k, gain=1.0):
  k = torch.tensor(k, dtype=torch.float64)
  if k.dim() == 1:
    k = torch.outer(k, k)
  return k / k.sum() * gain


def upfirdn2d(x, k, up=1, down=1, pad=(0, 0)):
  """Zero-insertion upsampling by `up`, zero padding (pad[0] before, pad[1] after, both axes), FIR (true convolution with k),
  keep every `down`-th sample."""
  N, C, H, W = x.shape
  if up > 1:
    z = x.new_zeros(N, C, H * up, W * up)
    z[:, :, ::up, ::up] = x
    x = z
  assert pad[0] >= 0 and pad[1] >= 0
  x = F.pad(x, [pad[0], pad[1], pad[0], pad[1]])
  w = torch.flip(k, [0, 1])[None, None].repeat(C, 1, 1, 1).to(x)
  return F.conv2d(x, w, groups=C)[:, :, ::down, ::down]


def upsample_2d(x, k, factor=2):
  taps = fir_taps(k, factor ** 2)
  p = taps.shape[0] - factor
  return upfirdn2d(x, taps, up=factor, pad=((p + 1) // 2 + factor - 1, p // 2))


def downsample_2d(x, k, factor=2):
  taps = fir_taps(k)
  p = taps.shape[0] - factor
  return upfirdn2d(x, taps, down=factor, pad=((p + 1) // 2, p // 2))


def naive_upsample_2d(x):
  return F.interpolate(x, scale_factor=2, mode='nearest')


def naive_downsample_2d(x):
  return F.avg_pool2d(x, 2, stride=2)


class _Params:
  """name -> float64 leaf copy of the module's parameter (requires_grad where the parameter does)."""

  def __init__(self, module):
    self.t = {n: p.detach().cpu().double().requires_grad_(p.requires_grad) for n, p in module.named_parameters()}

  def __call__(self, name):
    return self.t[name]


def _conv(P, pre, mod, x):
  return F.conv2d(x, P(pre + 'weight'), P(pre + 'bias') if mod.bias is not None else None, stride=mod.stride,
                  padding=mod.padding)


def _nin(P, pre, x):
  return torch.einsum('bchw,cd->bdhw', x, P(pre + 'W')) + P(pre + 'b')[None, :, None, None]


def _gn(P, pre, mod, x):
  return F.group_norm(x, mod.num_groups, P(pre + 'weight'), P(pre + 'bias'), mod.eps)


def _uds_conv(P, pre, mod, x):
  w = P(pre + 'weight')
  if mod.up:
    raise NotImplementedError
  if mod.down:
    taps = fir_taps(mod.resample_kernel)
    p = (taps.shape[0] - 2) + (w.shape[-1] - 1)
    y = F.conv2d(upfirdn2d(x, taps, pad=((p + 1) // 2, p // 2)), w, stride=2)
  else:
    y = F.conv2d(x, w, padding=mod.kernel // 2)
  if mod.use_bias:
    y = y + P(pre + 'bias').reshape(1, -1, 1, 1)
  return y


def forward(m, P, x, temb=None, y=None, pre=''):
  """The block `m` (any of the classes of the table in INTEGRATION.md) on float64 tensors."""
  name = type(m).__name__
  if name == 'NIN':
    return _nin(P, pre, x)
  if name == 'Conv2d' and hasattr(m, 'resample_kernel'):
    return _uds_conv(P, pre, m, x)
  if name == 'FixedFouriereProjection':
    return torch.cat([x] + [f(x * s * np.pi) for s in (128, 256) for f in (torch.sin, torch.cos)], dim=1)
  if name == 'GaussianFourierProjection':
    proj = x[:, None] * P(pre + 'W')[None, :] * 2 * np.pi
    return torch.cat([torch.sin(proj), torch.cos(proj)], dim=-1)
  if name == 'Combine':
    h = _conv(P, pre + 'Conv_0.', m.Conv_0, x)
    if m.method == 'cat':
      return torch.cat([h, y], dim=1)
    return h + y
  if name == 'AttnBlockpp':
    B, C, H, W = x.shape
    h = _gn(P, pre + 'GroupNorm_0.', m.GroupNorm_0, x)
    q, k, v = (_nin(P, pre + f'NIN_{i}.', h).reshape(B, C, H * W) for i in range(3))
    w = torch.softmax(torch.einsum('bct,bcs->bts', q, k) * (int(C) ** (-0.5)), dim=-1)
    h = torch.einsum('bts,bcs->bct', w, v).reshape(B, C, H, W)
    h = _nin(P, pre + 'NIN_3.', h)
    return (x + h) / SQRT2 if m.skip_rescale else x + h
  if name == 'Upsample':
    if not m.fir:
      h = naive_upsample_2d(x)
      return _conv(P, pre + 'Conv_0.', m.Conv_0, h) if m.with_conv else h
    if not m.with_conv:
      return upsample_2d(x, m.fir_kernel)
    return _uds_conv(P, pre + 'Conv2d_0.', m.Conv2d_0, x)
  if name == 'Downsample':
    if not m.fir:
      if m.with_conv:
        return _conv(P, pre + 'Conv_0.', m.Conv_0, F.pad(x, (0, 1, 0, 1)))
      return naive_downsample_2d(x)
    if not m.with_conv:
      return downsample_2d(x, m.fir_kernel)
    return _uds_conv(P, pre + 'Conv2d_0.', m.Conv2d_0, x)
  if name in ('ResnetBlockBigGANpp', 'ResnetBlockDDPMpp'):
    act = act_fn(m.act)
    h = act(_gn(P, pre + 'GroupNorm_0.', m.GroupNorm_0, x))
    if getattr(m, 'up', False) or getattr(m, 'down', False):
      if m.up:
        rs = (lambda t: upsample_2d(t, m.fir_kernel)) if m.fir else naive_upsample_2d
      else:
        rs = (lambda t: downsample_2d(t, m.fir_kernel)) if m.fir else naive_downsample_2d
      h, x = rs(h), rs(x)
    h = _conv(P, pre + 'Conv_0.', m.Conv_0, h)
    if temb is not None:
      h = h + F.linear(act(temb), P(pre + 'Dense_0.weight'), P(pre + 'Dense_0.bias'))[:, :, None, None]
    h = act(_gn(P, pre + 'GroupNorm_1.', m.GroupNorm_1, h))
    h = _conv(P, pre + 'Conv_1.', m.Conv_1, h)
    if hasattr(m, 'Conv_2'):
      x = _conv(P, pre + 'Conv_2.', m.Conv_2, x)
    elif hasattr(m, 'NIN_0'):
      x = _nin(P, pre + 'NIN_0.', x)
    return (x + h) / SQRT2 if m.skip_rescale else x + h
  raise ValueError(name)


def run(m, inputs, gout=None):
  """inputs: {name: tensor} (fp32, any device; a tensor that requires grad gets a gradient).  Returns (out, input grads,
  parameter grads) in float64 on the CPU, for the loss sum(out * gout) (gout = None: forward only)."""
  P = _Params(m)
  xs = {n: t.detach().cpu().double().requires_grad_(t.requires_grad) for n, t in inputs.items() if t is not None}
  out = forward(m, P, **xs)
  want = [t for t in xs.values() if t.requires_grad] + [t for t in P.t.values() if t.requires_grad]
  if gout is None or not want:
    return out.detach(), {}, {}
  grads = torch.autograd.grad(out, want, gout.detach().cpu().double(), allow_unused=True)
  names = [n for n, t in xs.items() if t.requires_grad] + [n for n, t in P.t.items() if t.requires_grad]
  got = dict(zip(names, grads))
  n_in = sum(1 for t in xs.values() if t.requires_grad)
  return out.detach(), dict(list(got.items())[:n_in]), dict(list(got.items())[n_in:])
