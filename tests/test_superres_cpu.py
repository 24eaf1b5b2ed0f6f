"""Host side of the super-resolution sampler (controllable_generation.py): its names, the ctypes table of
include/stk_superres.h, the refusal of host tensors and of a library without the header, the argument checks, and the float64
restatement the GPU tests compare with -- its identities and its agreement with upstream's transform-and-mask form.  No GPU."""
import os
import re

import pytest
import torch

import _superres_ref as R

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


def _sampler_args(st):
  S = st.sampling
  return dict(predictor=S.get_predictor('reverse_diffusion'), corrector=S.get_corrector('langevin'),
              inverse_scaler=lambda v: v, snr=0.16)


def _tiny(st):
  cfg = st.configs.tiny(st.configs.cifar10_ddpmpp_nll_st())
  cfg.device = torch.device('cpu')
  return cfg, st.sde_lib.get_sde(cfg, None)


def test_names_are_part_of_the_package(st, cg):
  assert 'controllable_generation' in st.__all__
  for name in ('get_pc_superresolver', 'superres_update', 'block_mean', 'superres_shape'):
    assert callable(getattr(cg, name)), name
  assert cg.FACTORS == (2, 4, 8, 16)


def test_signature_table_covers_the_header(st):
  """include/stk_superres.h declares exactly the entries engine/lib.py binds, argument for argument; stk.h keeps its 84."""
  text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'stk_superres.h')).read(), flags=re.S)
  decls = re.findall(r'\b(stk_[a-z0-9_]+)\s*\(([^)]*)\)', text)
  L = st.engine.lib
  table = L.SIGNATURES_SUPERRES
  assert sorted(n for n, _ in decls) == sorted(table) == ['stk_block_mean_f32', 'stk_superres_f32']
  assert not set(table) & set(L.SIGNATURES) and len(L.SIGNATURES) == 84
  for name, args in decls:
    kinds = [L.P if '*' in a else {'int': L.I, 'long': L.L, 'float': L.F}[a.split()[0]] for a in args.split(',')]
    assert kinds == table[name], name
  row = [h for h in L.OPTIONAL_HEADERS if h.path == 'include/stk_superres.h']
  assert len(row) == 1 and row[0].has == 'has_superres' and row[0].table is table


def test_host_tensors_are_refused(st, cg, product_backend, monkeypatch):
  """The package's device error, before anything is computed: no launch is attempted on a host pointer."""
  lib = product_backend.get()
  assert lib.has_superres is True

  def no_launch(*a):
    raise AssertionError('an entry of stk_superres.h was called on host tensors')

  monkeypatch.setattr(lib, 'superres_f32', no_launch)
  monkeypatch.setattr(lib, 'block_mean_f32', no_launch)
  cfg, sde = _tiny(st)
  x, low = torch.randn(2, 3, 16, 16), torch.randn(2, 3, 4, 4)
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    cg.block_mean(x, 4)
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    cg.superres_update(None, sde, None, low, 4, x, 0.5)
  with pytest.raises(RuntimeError, match='no CPU / PyTorch fallback'):
    cg.get_pc_superresolver(cfg, sde, **_sampler_args(st), factor=4)(None, low)


def test_library_without_the_header_is_refused_when_the_sampler_is_built(st, cg, ref_lib, product_backend):
  assert ref_lib.has_superres is False
  product_backend.set_backend(ref_lib)
  cfg, sde = _tiny(st)
  with pytest.raises(NotImplementedError, match='stk_superres.h'):
    cg.get_pc_superresolver(cfg, sde, **_sampler_args(st))
  with pytest.raises(NotImplementedError, match='stk_superres.h'):
    cg.block_mean(torch.randn(1, 3, 4, 4), 2)
  with pytest.raises(NotImplementedError, match='stk_superres.h'):
    cg.superres_update(None, sde, None, torch.randn(1, 3, 2, 2), 2, torch.randn(1, 3, 4, 4), 0.5)


def test_bad_sampling_precision_fails_when_the_sampler_is_built(st, cg, product_backend):
  cfg, sde = _tiny(st)
  cfg.sampling.precision = 'bf16'
  with pytest.raises(ValueError, match='precision'):
    cg.get_pc_superresolver(cfg, sde, **_sampler_args(st))


def test_bad_factor_shape_and_dtype_raise_value_error(st, cg, product_backend):
  meta = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device='meta')
  assert cg.superres_shape(meta(2, 3, 4, 4), 4) == (2, 3, 16, 16)
  assert cg.superres_shape(meta(1, 1, 3, 5), 2) == (1, 1, 6, 10)
  assert cg.superres_shape(meta(5, 3, 1, 2), 16) == (5, 3, 16, 32)
  for factor in (0, 1, 3, 5, 6, 32, -2, 4.0, '4', None, True):
    with pytest.raises(ValueError, match='factor'):
      cg.superres_shape(meta(2, 3, 4, 4), factor)
  for bad in (meta(3, 4, 4), meta(4, 4), meta(1, 2, 3, 4, 4), meta(2, 3, 4, 4, dtype=torch.float64),
              meta(2, 3, 4, 4, dtype=torch.float16), meta(2, 3, 0, 4)):
    with pytest.raises(ValueError, match='low'):
      cg.superres_shape(bad, 4)
  # at build time: the factor, and an image size the factor does not divide
  cfg, sde = _tiny(st)
  for factor in (3, 32, 0, 2.0):
    with pytest.raises(ValueError, match='factor'):
      cg.get_pc_superresolver(cfg, sde, **_sampler_args(st), factor=factor)
  cfg.data.image_size = 24
  with pytest.raises(ValueError, match='image_size'):
    cg.get_pc_superresolver(cfg, sde, **_sampler_args(st), factor=16)


def _operands(shape, r, seed):
  g = torch.Generator().manual_seed(seed)
  N, C, H, W = shape
  rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
  return rn(*shape), rn(N, C, H // r, W // r), rn(N, C, H // r, W // r), torch.rand(N, generator=g, dtype=torch.float64) + 0.25, \
      torch.rand(N, generator=g, dtype=torch.float64) * 3 + 0.05


@pytest.mark.parametrize('r', [2, 4, 8, 16])
def test_restatement_identities(r):
  shape = (2, 3, 2 * r, 3 * r)
  x, low, z, a, s = _operands(shape, r, seed=r)
  wide = lambda v: v[:, None, None, None]
  out, mean = R.restate(x, low, z, a, s, r)
  # the block mean of x_out is the perturbed measurement, that of x_mean its mean
  assert float((R.block_mean(out, r) - (wide(a) * low + wide(s) * z / r)).abs().max()) <= 1e-13
  assert float((R.block_mean(mean, r) - wide(a) * low).abs().max()) <= 1e-13
  # the other r^2 - 1 coefficients of x are kept
  detail = lambda t: t - R.upsample(R.block_mean(t, r), r)
  assert float((detail(out) - detail(x)).abs().max()) <= 1e-13
  assert float((detail(mean) - detail(x)).abs().max()) <= 1e-13
  # without noise the step is a projection, and x_out is x_mean
  once, once_mean = R.restate(x, low, None, a, s, r)
  twice, _ = R.restate(once, low, None, a, s, r)
  assert torch.equal(once, once_mean)
  assert float((twice - once).abs().max()) <= 1e-13
  assert bool((R.magnitude(x, low, z, a, s, r) >= out.abs() - 1e-13).all())
  assert R.DEPTH[r] <= r * r - 1


def test_restatement_is_upstreams_transform_and_mask_form():
  """r = 2 with the 4 x 4 orthonormal Haar basis of a block written out: upstream's colouriser formula,
  couple(decouple(x) (1 - mask) + (a decouple(data) + s zeta) mask) with the mask on the DC coefficient, is restate() given
  low = the block means of data and z = the DC component of zeta.  This pins the s / r factor."""
  r = 2
  g = torch.Generator().manual_seed(9)
  shape = (2, 3, 6, 10)
  N, C, H, W = shape
  x, data = (torch.randn(shape, generator=g, dtype=torch.float64) for _ in range(2))
  zeta = torch.randn(N, C, H // r, W // r, 4, generator=g, dtype=torch.float64)       # noise in the transformed space
  a = torch.rand(N, generator=g, dtype=torch.float64) + 0.25
  s = torch.rand(N, generator=g, dtype=torch.float64) * 3 + 0.05
  # columns: DC, horizontal, vertical, diagonal; pixels of a block in the order (0,0), (0,1), (1,0), (1,1)
  Q = 0.5 * torch.tensor([[1, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1]], dtype=torch.float64)
  assert torch.equal(Q @ Q.T, torch.eye(4, dtype=torch.float64))

  def blocks(t):           # [N,C,H,W] -> [N,C,H/2,W/2,4]
    return t.reshape(N, C, H // r, r, W // r, r).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H // r, W // r, 4)

  def unblocks(b):
    return b.reshape(N, C, H // r, W // r, r, r).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H, W)

  decouple = lambda t: blocks(t) @ Q
  couple = lambda b: unblocks(b @ Q.T)
  assert float((couple(decouple(x)) - x).abs().max()) <= 1e-14
  mask = torch.tensor([1., 0., 0., 0.], dtype=torch.float64)
  wide = lambda v: v[:, None, None, None, None]
  masked_mean = wide(a) * decouple(data)
  x_new = couple(decouple(x) * (1 - mask) + (masked_mean + wide(s) * zeta) * mask)
  x_mean = couple(decouple(x_new) * (1 - mask) + masked_mean * mask)
  out, mean = R.restate(x, R.block_mean(data, r), zeta[..., 0], a, s, r)
  assert float((out - x_new).abs().max()) <= 1e-13
  assert float((mean - x_mean).abs().max()) <= 1e-13
  # a wrong factor on the noise (s, or s / r^2) is far outside that
  wrong, _ = R.restate(x, R.block_mean(data, r), zeta[..., 0] * r, a, s, r)
  assert float((wrong - x_new).abs().max()) > 1e-2
