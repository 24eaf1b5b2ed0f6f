"""The fp16 mode's host side (include/stk_fp16.h, engine precision, config.sampling.precision): the signature table of the
new header, the product library's exports, the config handling and the refusals that need no GPU."""
import os
import re
import subprocess

import pytest
import torch

from _model_util import build_pair, tiny_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'stk.h')
HEADER_FP16 = os.path.join(ROOT, 'include', 'stk_fp16.h')
PRODUCT = os.path.join(ROOT, 'soft-truncation_amd', 'csrc', 'libstk.so')


def _symbols(path):
  text = re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)
  return sorted(set(re.findall(r'\b(stk_[a-z0-9_]+)\s*\(', text)))


def test_fp16_header_has_its_own_table(st):
  syms = _symbols(HEADER_FP16)
  assert syms == sorted(['stk_conv2d_fwd_pl_f16x1', 'stk_conv2d_fwd_rec_f16x1', 'stk_conv2d_fwd_wp_f16x1'])
  assert sorted(st.engine.lib.SIGNATURES_FP16) == syms
  # twins: identical argument lists to their fp32 entries, and none of them in stk.h (the checker implements stk.h only)
  for name in syms:
    assert st.engine.lib.SIGNATURES_FP16[name] == st.engine.lib.SIGNATURES[name.replace('_f16x1', '_f32')]
  assert not set(syms) & set(_symbols(HEADER))


def test_signatures_still_equal_stk_h(st):
  assert sorted(st.engine.lib.SIGNATURES) == _symbols(HEADER)


def test_product_library_exports_the_twins(st):
  if not os.path.exists(PRODUCT):
    subprocess.check_call(['make', '-C', os.path.dirname(PRODUCT), '-j4'])
  import ctypes
  dll = ctypes.CDLL(PRODUCT)
  for sym in _symbols(HEADER_FP16):
    assert hasattr(dll, sym), f'libstk.so does not export {sym}'
  assert st.engine.lib.load_path(PRODUCT).has_fp16


def test_checker_has_no_fp16_and_refuses_the_mode(st, ref_lib):
  assert not ref_lib.has_fp16
  cfg, _, _, model, _ = build_pair(st, tiny_config(st, 'vp'), ref_lib)
  with pytest.raises(st.engine.lib.StkMissingError):
    with st.models.utils.precision(model, 'fp16'):
      pass
  with st.models.utils.precision(model, 'fp32'):      # the default is always available
    pass
  with pytest.raises(ValueError):
    with st.models.utils.precision(model, 'bf16'):
      pass


def test_precision_is_a_no_op_without_an_engine(st):
  plain = torch.nn.Conv2d(3, 3, 1)
  with st.models.utils.precision(plain, 'fp16'):
    pass
  with pytest.raises(ValueError):
    st.models.utils.precision(plain, 'fp8')


def test_config_precision(st):
  cfg = st.configs.cifar10_ddpmpp_nll_st()
  mu = st.models.utils
  assert 'precision' not in cfg.sampling          # reference configs carry no such key ...
  assert mu.sampling_precision(cfg) == 'fp32'     # ... and that means fp32
  cfg.sampling.precision = 'fp16'
  assert mu.sampling_precision(cfg) == 'fp16'
  cfg.sampling.precision = 'half'
  with pytest.raises(ValueError):
    mu.sampling_precision(cfg)


def _sampler_args(st, cfg):
  sde = st.sde_lib.get_sde(cfg, None)
  shape = (1, cfg.data.num_channels, 8, 8)
  return sde, shape, st.datasets.get_data_inverse_scaler(cfg)


def test_pc_sampler_accepts_fp16_and_ode_refuses_it(st):
  cfg = tiny_config(st, 'vp')
  cfg.sampling.method = 'pc'
  sde, shape, inv = _sampler_args(st, cfg)
  st.sampling.get_sampling_fn(cfg, sde, shape, inv, 1e-3)             # absent key: fp32
  cfg.sampling.precision = 'fp16'
  st.sampling.get_sampling_fn(cfg, sde, shape, inv, 1e-3)
  cfg.sampling.method = 'ode'
  with pytest.raises(ValueError, match='ODE'):
    st.sampling.get_sampling_fn(cfg, sde, shape, inv, 1e-3)
  cfg.sampling.precision = 'fp32'
  st.sampling.get_sampling_fn(cfg, sde, shape, inv, 1e-3)
  cfg.sampling.precision = 'fp64'
  with pytest.raises(ValueError):
    st.sampling.get_sampling_fn(cfg, sde, shape, inv, 1e-3)


def test_likelihood_refuses_fp16(st):
  cfg = tiny_config(st, 'vp')
  sde, _, inv = _sampler_args(st, cfg)
  st.likelihood.get_likelihood_fn(cfg, sde, inv)
  cfg.sampling.precision = 'fp16'
  with pytest.raises(ValueError, match='fp32 only'):
    st.likelihood.get_likelihood_fn(cfg, sde, inv)
