"""Host side of scale-shift GroupNorm conditioning (config.model.scale_shift_norm, include/stk_adagn.h) and the yardstick
of its kernel tests: the closed-form gradients of the header against autograd in float64, the identity that makes the layer
a GroupNorm with per-sample affine parameters, condition (c) of tests/_gn_cases.py for every kernel-test case (a plain fp32
evaluation stays within HALF the tolerance on every figure), the ctypes table, and the config plumbing.  No GPU."""
import os
import re

import pytest
import torch

import _adagn_ref as R
from _model_util import tiny_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mask(case, shape):
  if 'drop' not in case[6]:
    return None
  keep = torch.rand(shape, generator=torch.Generator().manual_seed(9)) >= 0.1
  return keep.float() / 0.9


def _ref(case):
  d = R.inputs(case)
  N, C, HW = d['x'].shape
  mask = _mask(case, d['x'].shape)
  return d, mask, R.closed_form(d['x'], d['gamma'], d['beta'], d['s'], d['b'], d['dy'], case[4], case[5], mask)


@pytest.mark.parametrize('case', R.CASES, ids=R.CASE_IDS)
def test_closed_forms_agree_with_autograd(case):
  d, mask, ref = _ref(case)
  ag = R.by_autograd(d['x'], d['gamma'], d['beta'], d['s'], d['b'], d['dy'], case[4], case[5], mask)
  for k, v in ag.items():
    e = (ref[k] - v).abs().max().item() / (v.abs().max().item() + 1e-300)
    assert e <= 1e-11, f'{case[0]}: {k} of the closed form is {e:.3e} from autograd'


@pytest.mark.parametrize('case', R.CASES, ids=R.CASE_IDS)
def test_layer_is_a_groupnorm_with_per_sample_affine(case):
  d, mask, ref = _ref(case)
  N, C, HW = d['x'].shape
  args = [d[k].double() for k in ('x', 'gamma', 'beta', 's', 'b')]
  y = R.folded(*args, case[4], case[5], mask.double() if mask is not None else None)
  e = (y - ref['y']).abs().max().item() / ref['y'].abs().max().item()
  assert e <= 1e-12, f'{case[0]}: {e:.3e}'


def test_cases_reach_every_route_and_every_act():
  assert {R.route(c)[0] for c in R.CASES} == {'flat', 'loop', 'split'}
  assert {R.route(c)[1] for c in R.CASES} == {'flat', 'loop', 'split'}
  assert {c[5] for c in R.CASES} == {0, 1, 2, 3, 4}
  assert any(c[1] == 1 for c in R.CASES) and any('off4' in c[6] for c in R.CASES) and any(c[3] % 4 for c in R.CASES)
  assert any((c[2] // c[4]) * c[3] == 16384 for c in R.CASES), 'the largest one-workgroup group'
  for c in R.CASES:
    d = R.inputs(c)
    assert bool((d['s'] == -1).any()), 'gamma\' = 0 somewhere'
    assert c[1] == 1 or (not d['s'][-1].any() and not d['b'][-1].any()), 'an all-zero row'


@pytest.mark.parametrize('case', R.CASES, ids=R.CASE_IDS)
def test_fp32_evaluation_keeps_half_the_tolerance(case):
  """Condition (c) of tests/_gn_cases.py: the inputs ask nothing of the kernels that plain fp32 arithmetic cannot give."""
  d, mask, ref = _ref(case)
  got = R.closed_form(d['x'], d['gamma'], d['beta'], d['s'], d['b'], d['dy'], case[4], case[5], mask, dtype=torch.float32)
  fig = R.figures({k: got[k] for k in ('mean', 'rstd', 'y', 'dx', 'ds', 'db', 'dgamma', 'dbeta')}, ref, case[4])
  print(case[0], {k: f'{v * R.TOL:.2e}' for k, v in fig.items()})
  assert len(fig) == 8
  for k, v in fig.items():
    assert v <= 0.5, f'{case[0]}: fp32 {k} at {v * R.TOL:.3e} > TOL / 2 = {R.TOL / 2:.1e}'


# ---- the ABI table ------------------------------------------------------------------------------------------------------
def test_signature_table_covers_the_header(st):
  text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'stk_adagn.h')).read(), flags=re.S)
  decls = re.findall(r'\b(stk_[a-z0-9_]+)\s*\(([^)]*)\)', text)
  L = st.engine.lib
  table = L.SIGNATURES_ADAGN
  assert sorted(n for n, _ in decls) == sorted(table) == ['stk_gn_mod_bwd_f32', 'stk_gn_mod_fwd_f32', 'stk_gn_mod_ok',
                                                          'stk_gn_mod_ws_bytes']
  assert not set(table) & set(L.SIGNATURES) and len(L.SIGNATURES) == 84
  kind = {'int': L.I, 'long': L.L, 'float': L.F, 'unsigned': L.U64}
  for name, args in decls:
    kinds = [L.P if '*' in a else kind[a.split()[0]] for a in args.split(',')]
    assert kinds == table[name], name
  row = [h for h in L.OPTIONAL_HEADERS if h.path == 'include/stk_adagn.h']
  assert len(row) == 1 and row[0].has == 'has_adagn' and row[0].table is table
  assert row[0].restype == {'stk_gn_mod_ws_bytes': L.c_long} and set(row[0].unchecked) == {'stk_gn_mod_ws_bytes', 'stk_gn_mod_ok'}


def test_product_library_has_the_header_and_the_checker_has_not(st, ref_lib):
  lib = st.engine.lib.load()
  assert lib.has_adagn is True and ref_lib.has_adagn is False and not hasattr(ref_lib, 'gn_mod_fwd_f32')
  # the queries answer without a device
  assert int(lib.gn_mod_ok(128, 64, 32)) == 1 and int(lib.gn_mod_ok(48, 25, 5)) == 0 and int(lib.gn_mod_ok(0, 4, 1)) == 0
  for N, C, HW, G in [(2, 8, 16, 2), (2, 32, 8192, 8), (1, 128, 4096, 32)]:
    assert int(lib.gn_mod_ws_bytes(N, C, HW, G)) == int(lib.gn_ws_bytes(N, C, HW, G)) >= 8 * N * C
  assert int(lib.gn_mod_ws_bytes(2, 32, 8192, 8)) > 8 * 2 * 32          # the split route's partials


# ---- config plumbing ----------------------------------------------------------------------------------------------------
def _net(st, lib, family, **model):
  cfg = tiny_config(st, family)
  for k, v in model.items():
    setattr(cfg.model, k, v)
  torch.manual_seed(0)
  net = st.models.ncsnpp.NCSNpp(cfg, st.sde_lib.get_sde(cfg, None))
  net.set_backend(lib)
  return cfg, net


@pytest.mark.parametrize('family', ['vp', 'rve', 'wide'])
def test_switch_changes_the_dense_shapes_and_nothing_else(st, ref_lib, family):
  _, plain = _net(st, ref_lib, family)
  _, off = _net(st, ref_lib, family, scale_shift_norm=False)
  _, on = _net(st, ref_lib, family, scale_shift_norm=True)
  sd0, sd_off, sd1 = plain.state_dict(), off.state_dict(), on.state_dict()
  assert list(sd0) == list(sd_off) == list(sd1)
  assert all(torch.equal(sd0[k], sd_off[k]) for k in sd0), 'the switch set to False is not the network without the key'
  dense = 0
  for i, mod in enumerate(on.all_modules):
    if hasattr(mod, 'Dense_0'):
      dense += 1
      assert mod.scale_shift_norm is True
      assert tuple(mod.Dense_0.weight.shape) == (2 * mod.out_ch, plain.all_modules[i].Dense_0.weight.shape[1])
      assert tuple(mod.Dense_0.bias.shape) == (2 * mod.out_ch,) and not mod.Dense_0.bias.any()
      assert bool(mod.Dense_0.weight.any())
  assert dense >= 4
  for k in sd0:
    assert sd0[k].shape == sd1[k].shape or '.Dense_0.' in k, k
  # a checkpoint of the network without the switch does not fit: it fails on shape
  with pytest.raises(RuntimeError, match='size mismatch'):
    on.load_state_dict(sd0)


def test_switch_needs_a_conditional_network(st, ref_lib):
  with pytest.raises(ValueError, match='scale_shift_norm'):
    _net(st, ref_lib, 'vp', scale_shift_norm=True, conditional=False)
  _net(st, ref_lib, 'vp', scale_shift_norm=False, conditional=False)


def test_network_with_the_switch_on_the_checker_is_refused_when_planned(st, ref_lib):
  _, net = _net(st, ref_lib, 'vp', scale_shift_norm=True)
  x, t = torch.randn(2, 3, 16, 16), torch.rand(2) * 999
  with pytest.raises(NotImplementedError, match='stk_adagn.h'):
    net(x, t)
  _, plain = _net(st, ref_lib, 'vp')
  assert plain(x, t).shape == x.shape


@pytest.mark.parametrize('cls', ['ResnetBlockBigGANpp', 'ResnetBlockDDPMpp'])
def test_stand_alone_blocks_take_the_switch(st, ref_lib, cls):
  B = getattr(st.models.layerspp, cls)
  act = torch.nn.SiLU()
  m = B(act=act, in_ch=16, out_ch=32, temb_dim=24, dropout=0., scale_shift_norm=True)
  assert tuple(m.Dense_0.weight.shape) == (64, 24) and m.scale_shift_norm
  assert [n for n, _ in m.named_parameters()] == [n for n, _ in B(act=act, in_ch=16, out_ch=32, temb_dim=24).named_parameters()]
  with pytest.raises(ValueError, match='temb_dim'):
    B(act=act, in_ch=16, out_ch=32, scale_shift_norm=True)
  m.set_backend(ref_lib)
  with pytest.raises(ValueError, match='needs temb'):
    m(torch.randn(1, 16, 8, 8))
  with pytest.raises(NotImplementedError, match='stk_adagn.h'):
    m(torch.randn(1, 16, 8, 8), torch.randn(1, 24))
