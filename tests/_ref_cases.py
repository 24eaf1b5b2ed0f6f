"""Cases of tests/test_ref_live.py, shared with tools/make_golden.py.

make_golden.py ran each case once on the REFERENCE and stored its side under tests/golden/ref_live.{json,npz}: config values,
state_dict layouts, per-tensor digests of its weights and its network outputs.  The test runs the same case on this repository's
side and compares, so it needs nothing outside the repository.  A state_dict is pinned by the SHA-256 of every tensor's bytes
(as strict as torch.equal, and a few KB instead of megabytes of weights)."""
import hashlib

import numpy as np
import torch

# config name -> (the reference's config module, parameter count of the full-size model)
FULL = {
  'cifar10_ddpmpp_nll_st': ('configs.vp.CIFAR10.ddpmpp_nll_st', 61804419),
  'celeba_uncsnpp_st': ('configs.ve.CELEBA.uncsnpp_st', 62758915),
  'celebahq_uncsnpp_st': ('configs.ve.celebahq.uncsnpp_st', 65574549),
}
ACTIVATIONS = ['elu', 'relu', 'lrelu', 'swish+fourier_feature']
VP = 'configs.vp.CIFAR10.ddpmpp_nll_st'
VE_HQ = 'configs.ve.celebahq.uncsnpp_st'


def flatten(d, prefix=''):
  out = {}
  for k, v in d.items():
    if hasattr(v, 'items'):
      out.update(flatten(v, prefix + k + '.'))
    else:
      out[prefix + k] = v
  return out


def init_config(c):
  """test_init_statistics_match_reference: the VP config at nf = 32, one res block per level."""
  c.model.nf, c.model.num_res_blocks = 32, 1
  c.device = torch.device('cpu')
  return c


def activation_config(c, name):
  """test_other_activations_match_reference: the VP config at fixture size with nonlinearity `name` (+ fourier features)."""
  c.model.nf, c.model.ch_mult, c.model.num_res_blocks, c.model.attn_resolutions = 16, (1, 2), 1, (8,)
  c.model.dropout, c.data.image_size, c.model.nonlinearity = 0.0, 16, name.split('+')[0]
  c.model.fourier_feature = name.endswith('fourier_feature')
  c.device = torch.device('cpu')
  return c


def cat_config(c):
  """test_combine_cat_matches_reference: the NCSN++ pyramid config at fixture size with progressive_combine = 'cat'."""
  c.model.nf, c.model.ch_mult, c.model.num_res_blocks, c.model.attn_resolutions = 16, (1, 1, 2), 1, (8,)
  c.model.dropout, c.data.image_size, c.model.progressive_combine = 0.0, 16, 'cat'
  c.device = torch.device('cpu')
  return c


def randomize_(model, g):
  """Every trainable parameter, in parameters() order, to 0.1 x a standard normal draw of `g`."""
  with torch.no_grad():
    for p in model.parameters():
      if p.requires_grad:
        p.copy_(torch.randn(p.shape, generator=g) * 0.1)


def digests(sd):
  """key -> 'dtype shape sha256' of a state_dict, in its order."""
  out = {}
  for k, v in sd.items():
    a = np.ascontiguousarray(v.detach().cpu().numpy())
    out[k] = f'{a.dtype} {list(a.shape)} {hashlib.sha256(a.tobytes()).hexdigest()}'
  return out


def layout(model):
  """state_dict keys, shapes and dtypes, and requires_grad of parameters() in order."""
  return {'n_params': sum(p.numel() for p in model.parameters()),
          'state_dict': [[k, list(v.shape), str(v.dtype)] for k, v in model.state_dict().items()],
          'requires_grad': [p.requires_grad for p in model.parameters()]}
