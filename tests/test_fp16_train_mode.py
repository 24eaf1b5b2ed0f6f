"""The fp16 training mode's host side (include/stk_fp16_train.h, Executor.training_precision, config.training.precision):
the signature table of the new header, the product library's exports, the config handling and the refusals that need no
GPU."""
import os
import re
import subprocess

import pytest
import torch

from _model_util import build_pair, tiny_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'stk.h')
HEADER_FP16 = os.path.join(ROOT, 'include', 'stk_fp16.h')
HEADER_TRAIN = os.path.join(ROOT, 'include', 'stk_fp16_train.h')
PRODUCT = os.path.join(ROOT, 'soft-truncation_amd', 'csrc', 'libstk.so')
TWINS = ['stk_conv2d_dgrad_pl_f16x1', 'stk_conv2d_dgrad_rec_f16x1', 'stk_conv2d_dgrad_wp_f16x1', 'stk_conv2d_wgrad_amax_f16x1',
         'stk_conv2d_wgrad_pl_f16x1', 'stk_conv2d_wgrad_pl_wgs_f16x1']


def _symbols(path):
  text = re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)
  return sorted(set(re.findall(r'\b(stk_[a-z0-9_]+)\s*\(', text)))


def test_train_header_has_its_own_table(st):
  syms = _symbols(HEADER_TRAIN)
  assert syms == sorted(TWINS)
  lib = st.engine.lib
  assert sorted(lib.SIGNATURES_FP16_TRAIN) == syms
  for name in syms:        # twins: the argument lists of their fp32 entries
    assert lib.SIGNATURES_FP16_TRAIN[name] == lib.SIGNATURES[name.replace('_f16x1', '_f32')]
  assert not set(syms) & set(_symbols(HEADER))
  assert not set(syms) & set(_symbols(HEADER_FP16))


def test_product_library_exports_the_backward_twins(st):
  if not os.path.exists(PRODUCT):
    subprocess.check_call(['make', '-C', os.path.dirname(PRODUCT), '-j4'])
  import ctypes
  dll = ctypes.CDLL(PRODUCT)
  for sym in TWINS:
    assert hasattr(dll, sym), f'libstk.so does not export {sym}'
  lib = st.engine.lib.load_path(PRODUCT)
  assert lib.has_fp16 and lib.has_fp16_train


def test_checker_has_no_train_twins_and_refuses_the_mode(st, ref_lib):
  assert not ref_lib.has_fp16_train
  import ctypes
  dll = ctypes.CDLL(ref_lib.path)
  assert not [s for s in TWINS if hasattr(dll, s)]
  cfg, _, _, model, _ = build_pair(st, tiny_config(st, 'vp'), ref_lib)
  with pytest.raises(st.engine.lib.StkMissingError):
    with st.models.utils.training_precision(model, 'fp16'):
      pass
  with st.models.utils.training_precision(model, 'fp32'):
    pass
  with pytest.raises(ValueError):
    st.models.utils.training_precision(model, 'bf16')


def test_training_precision_is_a_no_op_without_an_engine(st):
  plain = torch.nn.Conv2d(3, 3, 1)
  with st.models.utils.training_precision(plain, 'fp16'):
    assert st.models.utils.current_training_precision(plain) == 'fp32'
  with pytest.raises(ValueError):
    st.models.utils.training_precision(plain, 'fp8')


def test_config_training_precision(st):
  cfg = st.configs.cifar10_ddpmpp_nll_st()
  mu = st.models.utils
  assert 'precision' not in cfg.training          # reference configs carry no such key ...
  assert mu.config_training_precision(cfg) == 'fp32'   # ... and that means fp32
  cfg.training.precision = 'fp16'
  assert mu.config_training_precision(cfg) == 'fp16'
  cfg.training.precision = 'half'
  with pytest.raises(ValueError):
    mu.config_training_precision(cfg)


def test_step_fn_checks_the_key_before_any_step(st):
  cfg = tiny_config(st, 'vp')
  sde = st.sde_lib.get_sde(cfg, None)
  opt = st.losses.optimization_manager(cfg)
  st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=opt)            # absent key
  cfg.training.precision = 'fp16'
  st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=opt)
  cfg.training.precision = 'fp64'
  with pytest.raises(ValueError, match='training.precision'):
    st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=opt)


def test_fp16_step_with_the_checker_raises_missing(st, ref_lib):
  """a config asking for the mode on a library without it fails at the first step, not silently in fp32"""
  from _model_util import make_state
  cfg, _, sde, model, _ = build_pair(st, tiny_config(st, 'vp'), ref_lib)
  cfg.training.precision = 'fp16'
  state = make_state(st, cfg, model)
  step_fn = st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg))
  batch = st.datasets.synthetic_batch(cfg, 2, generator=torch.Generator().manual_seed(0))
  with pytest.raises(st.engine.lib.StkMissingError):
    step_fn(state, batch)
