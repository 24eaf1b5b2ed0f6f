"""Multi-head attention without a GPU: the float64 restatement the GPU tests compare against (tests/_mh_ref.py), the
config keys model.num_heads / model.num_head_channels, what AttentionCore plans for heads > 1, and the GEMM + softmax form
with its host loop over the heads run on the plain-C checker against the multi-head RefNet."""
import copy
import importlib

import pytest
import torch
import torch.nn.functional as F

import _mh_ref
import ref_torch
from _model_cases import TOL, _inputs
from _model_util import grads_close, randomize_, rel_err, tiny_config
from _util import rnd


def _graph():
  return importlib.import_module('soft-truncation_amd.engine.graph')


# ---- the reference itself -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,C,T,heads', [(2, 64, 16, 2), (3, 96, 36, 3), (1, 128, 20, 4), (2, 32, 8, 1)])
def test_reference_is_a_per_head_loop_and_sdpa(B, C, T, heads):
  q, k, v, do = (rnd(B, C, T, seed=3 + i).double() for i in range(4))
  d = C // heads
  o = _mh_ref.attention(q, k, v, heads)
  full = _mh_ref.attention_with_grads(q, k, v, do, heads)
  for n in range(heads):
    c = slice(n * d, (n + 1) * d)
    on, lse = _mh_ref.single_head(q[:, c], k[:, c], v[:, c], d ** -0.5)
    assert (o[:, c] - on).abs().max().item() <= 1e-12
    assert (full['o'][:, c] - on).abs().max().item() <= 1e-12 and (full['lse'][:, n] - lse).abs().max().item() <= 1e-12
  # F.scaled_dot_product_attention on [B, h, T, d] (its default scale is d^-0.5)
  qs, ks, vs = (t.reshape(B, heads, d, T).transpose(2, 3) for t in (q, k, v))
  sd = F.scaled_dot_product_attention(qs, ks, vs).transpose(2, 3).reshape(B, C, T)
  assert (o - sd).abs().max().item() <= 1e-12
  # the hand-written gradients are autograd's
  qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
  (_mh_ref.attention(qa, ka, va, heads) * do).sum().backward()
  for n, t in (('dq', qa), ('dk', ka), ('dv', va)):
    assert (full[n] - t.grad).abs().max().item() <= 1e-12 * max(1.0, t.grad.abs().max().item()), n


def _mh_cfg(st, family='vp', **model_keys):
  cfg = tiny_config(st, family)
  for k, v in model_keys.items():
    setattr(cfg.model, k, v)
  return cfg


def _net(st, cfg, seed=0):
  torch.manual_seed(seed)
  return st.models.ncsnpp.NCSNpp(cfg, st.sde_lib.get_sde(cfg, None))


def test_one_head_refnet_subclass_is_refnet(st):
  cfg = _mh_cfg(st, num_heads=1)
  net = _net(st, cfg)
  randomize_(net, 0)
  sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
  a, b = ref_torch.RefNet(cfg, sd).eval(), _mh_ref.MHRefNet(cfg, sd).eval()
  x, t, cond = _inputs(cfg, st.sde_lib.get_sde(cfg, None), 2)
  assert torch.equal(a(x, cond), b(x, cond))


# ---- configuration ------------------------------------------------------------------------------------------------------
def _attn_blocks(net):
  return [(i, m) for i, m in enumerate(net.all_modules) if type(m).__name__ == 'AttnBlockpp']


def test_state_dict_does_not_depend_on_heads(st):
  base = _net(st, _mh_cfg(st)).state_dict()
  blocks = _attn_blocks(_net(st, _mh_cfg(st)))
  assert blocks and all(m.num_heads == 1 for _, m in blocks)
  for h in (1, 2, 4):
    net = _net(st, _mh_cfg(st, num_heads=h))
    sd = net.state_dict()
    assert list(sd) == list(base)
    for k in base:
      assert sd[k].shape == base[k].shape and torch.equal(sd[k], base[k]), k
    assert [m.num_heads for _, m in _attn_blocks(net)] == [h] * len(blocks)


def test_num_head_channels_resolves_per_block(st):
  # `ve` tiny: attention at two widths would need two resolutions; build a config whose blocks differ in C
  cfg = st.configs.tiny(st.configs.cifar10_ddpmpp_nll_st(), nf=32, ch_mult=(1, 2), num_res_blocks=1, image_size=8,
                        attn_resolutions=(8, 4), dropout=0.0)
  cfg.device = torch.device('cpu')
  cfg.model.num_head_channels = 32
  got = {m.NIN_0.W.shape[1]: m.num_heads for _, m in _attn_blocks(_net(st, cfg))}
  assert got == {32: 1, 64: 2}


def test_config_errors(st):
  with pytest.raises(ValueError, match='both set'):
    _net(st, _mh_cfg(st, num_heads=2, num_head_channels=32))
  C = _attn_blocks(_net(st, _mh_cfg(st)))[0][1].NIN_0.W.shape[1]
  i = _attn_blocks(_net(st, _mh_cfg(st)))[0][0]
  with pytest.raises(ValueError, match=rf'C = {C} channels of attention block all_modules\.{i}\b'):
    _net(st, _mh_cfg(st, num_heads=5))
  with pytest.raises(ValueError, match=rf'C = {C} channels of attention block all_modules\.{i}\b'):
    _net(st, _mh_cfg(st, num_head_channels=C - 1))
  with pytest.raises(ValueError, match='must be positive'):
    _net(st, _mh_cfg(st, num_heads=0))
  with pytest.raises(ValueError, match='num_heads = 3 does not divide the C = 128'):
    st.models.layerspp.AttnBlockpp(128, num_heads=3)


# ---- planning -----------------------------------------------------------------------------------------------------------
def _plan_core(lib, B, C, H, heads, stacked=False):
  G = _graph()
  g = G.Graph(None, lib)
  if stacked:
    qkv = g.input('qkv', (B, 3 * C, H, H), needs_grad=True)
    return G.AttentionCore(g, None, None, None, qkv=qkv, heads=heads)
  q, k, v = (g.input(n, (B, C, H, H), needs_grad=True) for n in 'qkv')
  return G.AttentionCore(g, q, k, v, heads=heads)


class _WithMh:
  """The checker's library, seeming to export include/stk_attention_mh.h (queries only: nothing is launched)."""

  def __init__(self, lib):
    self._lib, self.has_attention_mh, self.asked = lib, True, []

  def __getattr__(self, name):
    return getattr(self._lib, name)

  def attention_mh_ok(self, B, C, T, heads):
    self.asked.append((B, C, T, heads))
    return int(C % heads == 0 and (C // heads) % 32 == 0)

  def attention_mh_ws_bytes(self, B, C, T, heads):
    return 0 if T <= 256 else 12345


@pytest.mark.parametrize('stacked', [False, True], ids=['separate', 'stacked'])
def test_library_with_the_header_plans_the_mh_form(ref_lib, stacked):
  lib = _WithMh(ref_lib)
  op = _plan_core(lib, 2, 128, 8, 4, stacked)
  assert op.mh and not op.fused and not op.long and not hasattr(op, 's')
  assert op.lse.shape == (2, 4, 64) and op.delta.shape == (2, 4, 64) and op.rec.shape == (1024,)
  assert op.scale == 32 ** -0.5 and op.flops == 4.0 * 2 * 64 * 64 * 128
  assert lib.asked == [(2, 128, 64, 4)] and op.ws_bytes(lib) == 0
  assert _plan_core(lib, 2, 128, 32, 4, stacked).ws_bytes(lib) == 12345
  # a shape the entries refuse (d = 16) keeps the GEMM form
  op = _plan_core(lib, 2, 64, 8, 4, stacked)
  assert not op.mh and op.s.shape == (2, 4, 64, 64)


def test_library_without_the_header_plans_the_gemm_form(ref_lib):
  assert ref_lib.has_attention_mh is False
  op = _plan_core(ref_lib, 2, 128, 8, 4)
  assert not op.mh and not op.fused and not op.long
  assert op.s.shape == (2, 4, 64, 64) and op.p.shape == (2, 4, 64, 64) and not hasattr(op, 'lse')


def test_attn_fused_0_forces_the_gemm_form(ref_lib, monkeypatch):
  monkeypatch.setenv('STK_ATTN_FUSED', '0')
  op = _plan_core(_WithMh(ref_lib), 2, 128, 8, 4)
  assert not op.mh and op.s.shape == (2, 4, 64, 64)


def test_core_refuses_heads_that_do_not_divide(ref_lib):
  with pytest.raises(ValueError, match='heads = 3 does not divide C = 128'):
    _plan_core(ref_lib, 2, 128, 8, 3)


def test_product_library_exports_the_header(st):
  try:
    lib = st.engine.lib.load()
  except st.engine.lib.StkMissingError:
    pytest.fail('libstk.so is not built (run __graft_entry__.build())')
  assert lib.has_attention_mh is True
  ok, ws = lib.attention_mh_ok, lib.attention_mh_ws_bytes
  assert ok(1, 256, 256, 4) == 1 and ok(2, 512, 64, 2) == 1 and ok(2, 128, 320, 4) == 1 and ok(1, 64, 16384, 2) == 1
  assert ok(2, 96, 64, 2) == 0 and ok(2, 64, 64, 4) == 0 and ok(2, 64, 30, 2) == 0 and ok(2, 100, 64, 3) == 0
  assert ok(2, 1024, 64, 2) == 0                                  # d = 512
  assert ws(1, 256, 256, 4) == 0 and ws(2, 100, 64, 3) == -1 and ws(2, 96, 64, 2) == -3
  assert ws(2, 128, 320, 4) == lib.attention_long_ws_bytes(2, 128, 320)
  op = _plan_core(lib, 1, 256, 16, 4, stacked=True)
  assert op.mh and op.lse.shape == (1, 4, 256)
  one = _plan_core(lib, 1, 256, 16, 1, stacked=True)
  assert one.fused and not one.mh and one.lse.shape == (1, 256)


def _ops(st, cfg, lib, B=2):
  G = _graph()
  net = _net(st, cfg)
  flat = st.engine.flat.FlatParams(list(net.parameters()), 'cpu', groups=net._flat_groups())
  g = G.Graph(flat, lib)
  H = cfg.data.image_size
  g.finalize(net._emit(g, B, H, H, False), lib)
  return [(type(op).__name__, tuple(getattr(op, 'y', None).shape) if getattr(op, 'y', None) is not None else None,
           {k: v for k, v in vars(op).items() if isinstance(v, (bool, int, float, str))}) for op in g.ops]


def test_one_head_builds_the_program_of_a_config_without_the_key(st, ref_lib):
  assert _ops(st, _mh_cfg(st, num_heads=1), ref_lib) == _ops(st, _mh_cfg(st), ref_lib)
  assert _ops(st, _mh_cfg(st, num_heads=2), ref_lib) != _ops(st, _mh_cfg(st), ref_lib)


# ---- the GEMM + softmax form with its loop over the heads, on the checker --------------------------------------------------
def _pair(st, cfg, lib, seed=0):
  cfg = copy.deepcopy(cfg)
  sde = st.sde_lib.get_sde(cfg, None)
  net = _net(st, cfg, seed)
  net.set_backend(lib)
  randomize_(net, seed)
  _mh_ref.sharpen_(net)
  model = st.models.utils.DataParallel(net)
  net.engine().ensure_flat()
  sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
  return cfg, sde, model, st.models.utils.DataParallel(_mh_ref.MHRefNet(cfg, sd))


@pytest.mark.parametrize('keys', [dict(num_heads=2), dict(num_heads=4), dict(num_head_channels=16)], ids=str)
def test_gemm_form_matches_the_multi_head_refnet(st, ref_lib, keys):
  cfg, sde, model, ref = _pair(st, _mh_cfg(st, **keys), ref_lib)
  x, t, cond = _inputs(cfg, sde, 2)
  model.eval(); ref.eval()
  xg, xr = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
  y, yr = model(xg, cond), ref(xr, cond)
  assert rel_err(y, yr) <= TOL, rel_err(y, yr)
  go = torch.randn(yr.shape, generator=torch.Generator().manual_seed(5))
  (y * go).sum().backward()
  (yr * go).sum().backward()
  assert rel_err(xg.grad, xr.grad) <= TOL
  grads_close(model, ref, TOL)


@pytest.mark.parametrize('C,heads,H', [(64, 2, 4), (96, 3, 6), (64, 1, 4)])
def test_stand_alone_block_on_the_checker(st, ref_lib, C, heads, H):
  """AttnBlockpp(C, num_heads=h) as a module of its own (GEMM form on the checker): output, input and parameter gradients
  against float64 -- and the single-head evaluation of the same weights is far away, so the comparison sees the heads."""
  from _block_cases import ATTN_RTOL, compare_param_grads
  from _util import close
  m = _mh_ref.build_block(st, C, heads, 'cpu', ref_lib, skip_rescale=True)
  x = rnd(2, C, H, H, seed=2).requires_grad_(True)
  gout = rnd(2, C, H, H, seed=5)
  y = m(x)
  want, want_dx, want_p = _mh_ref.block(m, x, gout)
  close(y, want, rtol=ATTN_RTOL, what='output')
  m.zero_grad(set_to_none=False)
  y.backward(gout)
  close(x.grad, want_dx, rtol=ATTN_RTOL, what='dx')
  named = dict(m.named_parameters())
  compare_param_grads({n: named[n].grad for n in want_p}, want_p, ATTN_RTOL, 'block')
  if heads > 1:
    one = _mh_ref.block(m, x, gout, heads=1)[0]
    assert (one - want).abs().max().item() > 1e-2 * want.abs().max().item()
