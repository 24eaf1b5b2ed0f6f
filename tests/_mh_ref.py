"""Multi-head attention restated for the tests (the oracle's RefNet is single-head): a float64 attention core with its
gradients on [B, C, T] tensors whose heads are the contiguous channel slices [n d, (n + 1) d), d = C / heads, and a RefNet
whose attention blocks have the heads config.model.num_heads / num_head_channels ask for."""
import numpy as np
import torch
import torch.nn.functional as F

import ref_torch


def single_head(q, k, v, scale):
  """o, lse of ONE head: q, k, v of [B, d, T] (models/layerspp.py:95-99 with an explicit score scale)."""
  s = scale * torch.einsum('bct,bcs->bts', q, k)
  lse = torch.logsumexp(s, 2)
  p = torch.exp(s - lse[:, :, None])
  return torch.einsum('bts,bcs->bct', p, v), lse


def attention(q, k, v, heads, scale=None):
  """o of [B, C, T] in float64: the [B, heads, d, T] view, all heads at once."""
  q, k, v = (t.double() for t in (q, k, v))
  B, C, T = q.shape
  d = C // heads
  scale = d ** -0.5 if scale is None else scale
  q, k, v = (t.reshape(B, heads, d, T) for t in (q, k, v))
  s = scale * torch.einsum('bnct,bncs->bnts', q, k)
  p = torch.softmax(s, 3)
  return torch.einsum('bnts,bncs->bnct', p, v).reshape(B, C, T)


def attention_with_grads(q, k, v, do, heads, scale=None):
  """float64 o, lse [B, heads, T], delta [B, heads, T], dq, dk, dv of [B, C, T] inputs, written out head by head."""
  q, k, v, do = (t.double() for t in (q, k, v, do))
  B, C, T = q.shape
  d = C // heads
  scale = d ** -0.5 if scale is None else scale
  out = {n: torch.zeros_like(q) for n in ('o', 'dq', 'dk', 'dv')}
  out['lse'] = torch.zeros(B, heads, T, dtype=torch.float64)
  out['delta'] = torch.zeros(B, heads, T, dtype=torch.float64)
  for n in range(heads):
    c = slice(n * d, (n + 1) * d)
    s = scale * torch.einsum('bct,bcs->bts', q[:, c], k[:, c])
    lse = torch.logsumexp(s, 2)
    p = torch.exp(s - lse[:, :, None])
    o = torch.einsum('bts,bcs->bct', p, v[:, c])
    de = (do[:, c] * o).sum(1)                                         # [B, T]
    dp = torch.einsum('bct,bcs->bts', do[:, c], v[:, c])
    ds = p * (dp - de[:, :, None])
    out['o'][:, c], out['lse'][:, n], out['delta'][:, n] = o, lse, de
    out['dq'][:, c] = scale * torch.einsum('bcs,bts->bct', k[:, c], ds)
    out['dk'][:, c] = scale * torch.einsum('bct,bts->bcs', q[:, c], ds)
    out['dv'][:, c] = torch.einsum('bct,bts->bcs', do[:, c], p)
  return out


def heads_of(config, C):
  """Heads of an attention block of C channels under config.model.num_heads / num_head_channels (absent: one)."""
  m = config.model
  h, d = getattr(m, 'num_heads', None), getattr(m, 'num_head_channels', None)
  if d is not None:
    return C // int(d)
  return 1 if h is None else int(h)


class MHRefNet(ref_torch.RefNet):
  """RefNet with the attention blocks' heads taken from the config; one head runs RefNet's own _attn."""

  def _attn(self, i, x):
    B, C, H, W = x.shape
    heads = heads_of(self.config, C)
    if heads == 1:
      return super()._attn(i, x)
    pre = f'all_modules.{i}'
    d = C // heads
    h = self._gn(pre + '.GroupNorm_0', x)
    q, k, v = (self._nin(pre + f'.NIN_{j}', h).reshape(B, heads, d, H * W) for j in range(3))
    w = torch.einsum('bnct,bncs->bnts', q, k) * (int(d) ** (-0.5))
    w = F.softmax(w, dim=-1)
    h = torch.einsum('bnts,bncs->bnct', w, v).reshape(B, C, H, W)
    h = self._nin(pre + '.NIN_3', h)
    return (x + h) / np.sqrt(2.) if self.config.model.skip_rescale else x + h


def sharpen_(net, factor=8.0, out_factor=4.0):
  """Scale the query and key projections (and the output projection) of every attention block.  With the 0.1-sigma
  weights of _model_util.randomize_ the scores are ~1e-1, every softmax is almost uniform and the output almost the mean of
  v whatever the heads are, and the block adds little to its residual: a wrong head split would pass a model-level
  comparison.  Scores of a few units make the heads matter."""
  with torch.no_grad():
    for m in net.modules():
      if type(m).__name__ == 'AttnBlockpp':
        m.NIN_0.W.mul_(factor)
        m.NIN_1.W.mul_(factor)
        m.NIN_3.W.mul_(out_factor)


def block(m, x, gout, heads=None):
  """float64 restatement of a stand-alone AttnBlockpp `m` with m.num_heads heads (or `heads`): the output, the input
  gradient and the parameter gradients under the output gradient `gout`."""
  heads = m.num_heads if heads is None else heads
  P = {n: p.detach().cpu().double().requires_grad_(True) for n, p in m.named_parameters()}
  x = x.detach().cpu().double().requires_grad_(True)
  B, C, H, W = x.shape
  d = C // heads
  gn = m.GroupNorm_0
  h = F.group_norm(x, gn.num_groups, P['GroupNorm_0.weight'], P['GroupNorm_0.bias'], eps=gn.eps)
  nin = lambda i, t: torch.einsum('bct,cd->bdt', t, P[f'NIN_{i}.W']) + P[f'NIN_{i}.b'][None, :, None]
  q, k, v = (nin(i, h.reshape(B, C, H * W)) for i in range(3))
  o = attention(q, k, v, heads, d ** -0.5)
  y = x + nin(3, o).reshape(B, C, H, W)
  if m.skip_rescale:
    y = y / np.sqrt(2.)
  y.backward(gout.detach().cpu().double())
  return y.detach(), x.grad, {n: p.grad for n, p in P.items()}


def build_block(st, C, heads, device, backend=None, skip_rescale=False, seed=0, sharpen=3.0):
  """AttnBlockpp(C, num_heads=heads) with random parameters (tests/_block_cases.build), queries and keys scaled so that the
  softmax is far from uniform."""
  torch.manual_seed(seed)
  m = st.models.layerspp.AttnBlockpp(C, skip_rescale=skip_rescale, num_heads=heads)
  g = torch.Generator().manual_seed(seed + 1)
  with torch.no_grad():
    for n, p in m.named_parameters():
      if n.endswith('GroupNorm_0.weight'):
        p.copy_(1 + 0.2 * torch.randn(p.shape, generator=g))
      else:
        p.copy_(0.1 * torch.randn(p.shape, generator=g))
  sharpen_(m, sharpen, 1.0)
  m = m.to(device).eval()
  if backend is not None:
    m.set_backend(backend)
  return m
