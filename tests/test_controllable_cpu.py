"""Host side of controllable_generation.py: the colour matrices, the mask helper, the host-only mask-form check, the refusal
of host tensors and of a library without include/stk_impute.h, and the ctypes table of that header.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def cg(st):
  return st.controllable_generation


@pytest.fixture
def product_backend(st):
  """The `op` functions bound to the product library, whatever an earlier test bound them to."""
  from importlib import import_module
  backend = import_module('soft-truncation_amd.op._backend')
  saved = backend._backend
  backend.set_backend(st.engine.lib.load())
  yield backend
  backend.set_backend(saved)


def test_module_is_part_of_the_package(st, cg):
  assert 'controllable_generation' in st.__all__
  for name in ('get_pc_inpainter', 'get_pc_colorizer', 'inpaint_update', 'colorize_update', 'decouple', 'couple', 'get_mask'):
    assert callable(getattr(cg, name)), name


def test_colour_matrices(cg):
  M, inv = cg.M.double(), cg.INV_M.double()
  assert cg.M.dtype == cg.INV_M.dtype == torch.float32
  eye = torch.eye(3, dtype=torch.float64)
  assert float((M @ inv - eye).abs().max()) <= 1e-6
  assert float((M @ M.T - eye).abs().max()) <= 1e-6
  # inv M is the float64 inverse of the fp32 matrix, rounded once
  assert torch.equal(cg.INV_M, torch.from_numpy(np.linalg.inv(cg.M.numpy().astype(np.float64))).float())
  # the first decoupled channel is the gray axis (upstream's digits: orthogonal to the same 1e-6)
  assert float((M[:, 0] - 3 ** -0.5).abs().max()) <= 1e-6


def test_get_mask(cg):
  image = torch.randn(2, 3, 4, 5)
  mask = cg.get_mask(image)
  assert mask.shape == image.shape and mask.dtype == image.dtype
  assert bool((mask[:, 0] == 1).all()) and bool((mask[:, 1:] == 0).all())


def test_mask_form_is_host_only(cg):
  meta = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device='meta')
  data = meta(4, 3, 8, 6)
  assert cg.mask_form(meta(4, 3, 8, 6), data) == (4, 3)
  assert cg.mask_form(meta(1, 1, 8, 6), data) == (1, 1)
  assert cg.mask_form(meta(4, 1, 8, 6), data) == (4, 1)
  assert cg.mask_form(meta(1, 3, 8, 6), data) == (1, 3)
  assert cg.mask_form(meta(8, 6), data) == (1, 1)
  assert cg.mask_form(meta(3, 8, 6), data) == (1, 3)
  for bad in (meta(2, 3, 8, 6), meta(4, 2, 8, 6), meta(4, 3, 8, 1), meta(4, 3, 1, 6), meta(4, 3, 6, 8), meta(6),
              meta(1, 4, 3, 8, 6), meta(4, 3, 8, 6, dtype=torch.float64), meta(4, 3, 8, 6, dtype=torch.bool)):
    with pytest.raises(ValueError):
      cg.mask_form(bad, data)
  with pytest.raises(ValueError):
    cg.mask_form(meta(8, 6), meta(3, 8, 6))


def test_host_tensors_are_refused(st, cg, product_backend, monkeypatch):
  """The package's device error, before anything is computed: no launch is attempted on a host pointer."""
  lib = product_backend.get()
  assert lib.has_impute is True

  def no_launch(*a):
    raise AssertionError('stk_impute_f32 was called on host tensors')

  monkeypatch.setattr(lib, 'impute_f32', no_launch)
  x = torch.randn(2, 3, 4, 4)
  for fn in (cg.decouple, cg.couple):
    with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
      fn(x)
  cfg = st.configs.tiny(st.configs.cifar10_ddpmpp_nll_st())
  cfg.device = torch.device('cpu')
  sde = st.sde_lib.get_sde(cfg, None)
  S = st.sampling
  args = dict(predictor=S.get_predictor('reverse_diffusion'), corrector=S.get_corrector('langevin'),
              inverse_scaler=lambda v: v, snr=0.16)
  mask = torch.ones(1, 1, 4, 4)
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    cg.get_pc_inpainter(cfg, sde, **args)(None, x, mask)
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    cg.get_pc_colorizer(cfg, sde, **args)(None, x)
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    cg.inpaint_update(None, sde, None, x, mask, x, 0.5)
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    cg.colorize_update(None, sde, None, x, x, 0.5)


def test_library_without_the_header_is_refused_when_the_sampler_is_built(st, cg, ref_lib, product_backend):
  assert ref_lib.has_impute is False
  product_backend.set_backend(ref_lib)
  cfg = st.configs.tiny(st.configs.cifar10_ddpmpp_nll_st())
  sde = st.sde_lib.get_sde(cfg, None)
  S = st.sampling
  args = dict(predictor=S.get_predictor('reverse_diffusion'), corrector=S.get_corrector('langevin'),
              inverse_scaler=lambda v: v, snr=0.16)
  for build in (cg.get_pc_inpainter, cg.get_pc_colorizer):
    with pytest.raises(NotImplementedError, match='stk_impute.h'):
      build(cfg, sde, **args)
  with pytest.raises(NotImplementedError, match='stk_impute.h'):
    cg.decouple(torch.randn(1, 3, 4, 4))


def test_bad_sampling_precision_fails_when_the_sampler_is_built(st, cg, product_backend):
  cfg = st.configs.tiny(st.configs.cifar10_ddpmpp_nll_st())
  cfg.sampling.precision = 'bf16'
  sde = st.sde_lib.get_sde(cfg, None)
  S = st.sampling
  with pytest.raises(ValueError, match='precision'):
    cg.get_pc_inpainter(cfg, sde, S.get_predictor('reverse_diffusion'), S.get_corrector('langevin'), lambda v: v, 0.16)


def test_signature_table_covers_the_header(st):
  """include/stk_impute.h declares exactly the entries engine/lib.py binds, argument for argument; stk.h keeps its 84."""
  text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'stk_impute.h')).read(), flags=re.S)
  decls = re.findall(r'\b(stk_[a-z0-9_]+)\s*\(([^)]*)\)', text)
  table = st.engine.lib.SIGNATURES_IMPUTE
  assert sorted(n for n, _ in decls) == sorted(table) == ['stk_impute_f32']
  assert not set(table) & set(st.engine.lib.SIGNATURES) and len(st.engine.lib.SIGNATURES) == 84
  L = st.engine.lib
  for name, args in decls:
    kinds = [L.P if '*' in a else {'int': L.I, 'long': L.L, 'float': L.F}[a.split()[0]] for a in args.split(',')]
    assert kinds == table[name], name


def test_float64_restatement_identities():
  """The reference the GPU tests compare with: m = 0 returns x, m = 1 the perturbed data and its mean, and the colour round
  trip is the identity to float64 accuracy."""
  from test_gpu_impute import magnitude, matrices, restate
  g = torch.Generator().manual_seed(0)
  x, data, z = (torch.randn(2, 3, 4, 4, generator=g, dtype=torch.float64) for _ in range(3))
  a, s = torch.rand(2, generator=g, dtype=torch.float64), torch.rand(2, generator=g, dtype=torch.float64)
  wide = lambda v: v[:, None, None, None]
  zero, one = torch.zeros(1, 1, 4, 4, dtype=torch.float64), torch.ones(1, 1, 4, 4, dtype=torch.float64)
  out, mean = restate(x, data, z, zero, a, s)
  assert torch.equal(out, x) and torch.equal(mean, x)
  out, mean = restate(x, data, z, one, a, s)
  assert torch.equal(out, wide(a) * data + wide(s) * z) and torch.equal(mean, wide(a) * data)
  m64, u64, _, _ = matrices()
  out, _ = restate(x, data, z, zero, a, s, m64, u64)
  assert float((out - x).abs().max()) <= 1e-14
  # upstream's two-line form, with the colour transforms written out
  mask = torch.zeros(1, 3, 4, 4, dtype=torch.float64)
  mask[:, 0] = 1
  dec = lambda t: torch.einsum('bihw,ij->bjhw', t, m64)
  cpl = lambda t: torch.einsum('bihw,ij->bjhw', t, u64)
  masked_mean = wide(a) * dec(data)
  x_new = cpl(dec(x) * (1 - mask) + (masked_mean + wide(s) * z) * mask)
  x_mean = cpl(dec(x_new) * (1 - mask) + masked_mean * mask)
  out, mean = restate(x, data, z, mask, a, s, m64, u64)
  assert float((out - x_new).abs().max()) <= 1e-14 and float((mean - x_mean).abs().max()) <= 1e-14
  assert bool((magnitude(x, data, z, mask, a, s, m64, u64)[0] >= out.abs() - 1e-14).all())
