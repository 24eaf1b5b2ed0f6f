"""Multi-head attention in the network and in the stand-alone block on the HIP kernels: NCSNpp with model.num_heads /
model.num_head_channels against the multi-head RefNet of tests/_mh_ref.py (forward, input gradient, parameter gradients at
the TOL of tests/_model_cases.py), the fused entries against the GEMM form (STK_ATTN_FUSED=0), AttnBlockpp(num_heads=4) on
its own against float64, a training step and a PC iteration, and one head against a config without the key."""
import copy
import importlib

import numpy as np
import pytest
import torch

import _launch_trace as lt
import _mh_ref
from _block_cases import ATTN_RTOL, compare_param_grads
from _model_cases import TOL, _inputs
from _model_util import grads_close, make_state, patched_rng, randomize_, rel_err, tiny_config
from _util import close, rnd

pytestmark = pytest.mark.gpu


def _graph():
  return importlib.import_module('soft-truncation_amd.engine.graph')


def _config(st, family, **model_keys):
  if family == 'map32':       # attention on a 32 x 32 map (T = 1024: the streaming form) and at the 16 x 16 bottleneck
    cfg = st.configs.tiny(st.configs.cifar10_ddpmpp_nll_st(), nf=64, ch_mult=(1, 1), num_res_blocks=1, image_size=32,
                          attn_resolutions=(32,), dropout=0.0)
    cfg.device = torch.device('cpu')
  else:
    cfg = tiny_config(st, family)
  for k, v in model_keys.items():
    setattr(cfg.model, k, v)
  return cfg


def _pair(st, cfg, lib, seed=0, with_ref=True):
  """Product model on `lib` and the multi-head RefNet with the same (randomised, sharpened) weights."""
  cfg = copy.deepcopy(cfg)
  cfg.device = torch.device('cuda:0')
  sde = st.sde_lib.get_sde(cfg, None)
  torch.manual_seed(seed)
  net = st.models.ncsnpp.NCSNpp(cfg, sde)
  net.set_backend(lib)
  net = net.to(cfg.device)
  randomize_(net, seed)
  _mh_ref.sharpen_(net)
  model = st.models.utils.DataParallel(net)
  net.engine().ensure_flat()
  cfg_cpu = copy.deepcopy(cfg)
  cfg_cpu.device = torch.device('cpu')
  ref = None
  if with_ref:
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    ref = st.models.utils.DataParallel(_mh_ref.MHRefNet(cfg_cpu, sd))
  return cfg, cfg_cpu, sde, model, ref


def _fwd_bwd(model, x, cond, go):
  dev = next(model.parameters()).device
  model.zero_grad()
  xg = x.clone().to(dev).requires_grad_(True)
  y = model(xg, cond.to(dev))
  (y * go.to(dev)).sum().backward()
  return y.detach(), xg.grad.detach(), [p.grad.detach().clone() for p in model.parameters() if p.grad is not None]


CASES = [('wide', dict(num_heads=2)), ('wide', dict(num_heads=3)), ('wide', dict(num_head_channels=64)),
         ('map32', dict(num_heads=2))]


@pytest.mark.parametrize('family,keys', CASES, ids=lambda v: str(v))
def test_network_matches_the_multi_head_refnet(st, hip_lib, family, keys):
  cfg, cfg_cpu, sde, model, ref = _pair(st, _config(st, family, **keys), hip_lib)
  B = 2
  x, t, cond = _inputs(cfg, sde, B)
  model.eval(); ref.eval()
  go = torch.randn(x.shape, generator=torch.Generator().manual_seed(5))
  y, gx, _ = _fwd_bwd(model, x, cond, go)
  xr = x.clone().requires_grad_(True)
  yr = ref(xr, cond)
  (yr * go).sum().backward()
  print(f'{family} {keys}: forward {rel_err(y, yr):.2e}, input gradient {rel_err(gx, xr.grad):.2e}')
  assert rel_err(y, yr) <= TOL, f'forward mismatch {rel_err(y, yr):.3e}'
  assert rel_err(gx, xr.grad) <= TOL, f'input-gradient mismatch {rel_err(gx, xr.grad):.3e}'
  grads_close(model, ref, TOL)
  # every attention block ran the fused multi-head entries, with the heads the config asks for
  blocks = [m for m in model.module.all_modules if type(m).__name__ == 'AttnBlockpp']
  assert blocks and all(m.num_heads == _mh_ref.heads_of(cfg, m.NIN_0.W.shape[1]) > 1 for m in blocks)
  G = _graph()
  cores = [op for ex in [model.module.engine()] for p in ex.programs.values() for op in p.graph.ops
           if isinstance(op, G.AttentionCore)]
  assert cores and all(op.mh and op.heads > 1 for op in cores)
  if family == 'map32':
    assert {op.T for op in cores} == {1024, 256}


@pytest.mark.parametrize('family,keys', [('wide', dict(num_heads=3)), ('map32', dict(num_heads=2))], ids=lambda v: str(v))
def test_fused_entries_agree_with_the_gemm_form(st, hip_lib, monkeypatch, family, keys):
  cfg, _, sde, model, _ = _pair(st, _config(st, family, **keys), hip_lib, with_ref=False)
  x, t, cond = _inputs(cfg, sde, 2)
  go = torch.randn(x.shape, generator=torch.Generator().manual_seed(5))
  model.eval()
  y, gx, gp = _fwd_bwd(model, x, cond, go)
  monkeypatch.setenv('STK_ATTN_FUSED', '0')                        # read when a program is planned: a fresh model plans anew
  _, _, _, gemm, _ = _pair(st, _config(st, family, **keys), hip_lib, with_ref=False)
  gemm.eval()
  y2, gx2, gp2 = _fwd_bwd(gemm, x, cond, go)
  G = _graph()
  cores = [op for p in gemm.module.engine().programs.values() for op in p.graph.ops if isinstance(op, G.AttentionCore)]
  assert cores and all(not op.mh and op.s.shape[1] == op.heads > 1 for op in cores)
  assert rel_err(y, y2) <= ATTN_RTOL and rel_err(gx, gx2) <= ATTN_RTOL
  scale = max(g.abs().max().item() for g in gp2)
  assert max((a - b).abs().max().item() for a, b in zip(gp, gp2)) <= ATTN_RTOL * scale


@pytest.mark.parametrize('H', [8, 32])
def test_stand_alone_block_with_four_heads(st, hip_lib, H):
  m = _mh_ref.build_block(st, 128, 4, 'cuda', hip_lib, skip_rescale=True)
  x = rnd(2, 128, H, H, seed=2).cuda().requires_grad_(True)
  gout = rnd(2, 128, H, H, seed=5).cuda()
  y = m(x)
  want, want_dx, want_p = _mh_ref.block(m, x, gout)
  close(y, want, rtol=ATTN_RTOL, what='output')
  m.zero_grad(set_to_none=False)
  y.backward(gout)
  close(x.grad, want_dx, rtol=ATTN_RTOL, what='dx')
  named = dict(m.named_parameters())
  compare_param_grads({n: named[n].grad for n in want_p}, want_p, ATTN_RTOL, f'block {H}x{H}')
  one = _mh_ref.block(m, x, gout, heads=1)[0]
  assert (one - want).abs().max().item() > 1e-2 * want.abs().max().item()     # the comparison sees the heads


def _train_step(st, lib, cfg):
  base = copy.deepcopy(cfg)
  base.optim.warmup = 2
  cfg, cfg_cpu, sde, model, _ = _pair(st, base, lib, with_ref=False)
  state = make_state(st, cfg, model)
  state['optimizer']._backend = lib
  state['ema'].set_backend(lib)
  step_fn = st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg))
  batch = st.datasets.synthetic_batch(cfg_cpu, 4, generator=torch.Generator().manual_seed(100))
  np.random.seed(7)
  with patched_rng(50):
    loss = step_fn(state, batch.to(cfg.device))
  return loss, [p.detach().cpu().clone() for p in model.parameters()]


def test_training_step_and_pc_iteration_are_finite_and_deterministic(st, hip_lib):
  cfg = _config(st, 'wide', num_heads=3)
  (l1, p1), (l2, p2) = _train_step(st, hip_lib, cfg), _train_step(st, hip_lib, cfg)
  assert torch.isfinite(l1).all() and all(torch.isfinite(p).all() for p in p1)
  assert torch.equal(l1, l2) and all(torch.equal(a, b) for a, b in zip(p1, p2))
  base = copy.deepcopy(cfg)
  base.sampling.method, base.sampling.predictor, base.sampling.corrector = 'pc', 'euler_maruyama', 'none'
  cfg2, _, sde, model, _ = _pair(st, base, hip_lib, with_ref=False)
  sde.N = 1
  shape = (2, cfg2.data.num_channels, cfg2.data.image_size, cfg2.data.image_size)
  fn = st.sampling.get_sampling_fn(cfg2, sde, shape, st.datasets.get_data_inverse_scaler(cfg2), 1e-3)
  out = []
  for _ in range(2):
    with patched_rng(11):
      xs, nfe = fn(model)
    out.append(xs.detach().cpu())
  assert torch.isfinite(out[0]).all() and torch.equal(out[0], out[1])


def test_one_head_is_the_network_without_the_key(st, hip_lib):
  cfg_a, cfg_b = _config(st, 'wide'), _config(st, 'wide', num_heads=1)
  _, _, sde, a, _ = _pair(st, cfg_a, hip_lib, with_ref=False)
  cfg, _, _, b, _ = _pair(st, cfg_b, hip_lib, with_ref=False)
  x, t, cond = _inputs(cfg, sde, 2)
  go = torch.randn(x.shape, generator=torch.Generator().manual_seed(5))
  a.eval(); b.eval()
  ya, gxa, gpa = _fwd_bwd(a, x, cond, go)
  yb, gxb, gpb = _fwd_bwd(b, x, cond, go)
  assert torch.equal(ya, yb) and torch.equal(gxa, gxb) and all(torch.equal(p, q) for p, q in zip(gpa, gpb))
  score = lambda m: st.models.utils.get_score_fn(cfg, sde, m, train=False, continuous=True)(x.cuda(), t.cuda())
  assert torch.equal(score(a), score(b))
  # the launches, read from the plan (nothing runs): the same lines, and the single-head entries among them
  traces = []
  for c in (cfg_a, cfg_b):
    c = copy.deepcopy(c)
    net = st.models.ncsnpp.NCSNpp(c, st.sde_lib.get_sde(c, None))
    flat = st.engine.flat.FlatParams(list(net.parameters()), 'cpu', groups=net._flat_groups())
    log, _ = lt.trace(st, (net, flat, 4, c.data.image_size, c.data.image_size), hip_lib)
    traces.append(lt.lines(log))
  assert traces[0] == traces[1]
  names = {line.split()[0] for line in traces[0]}
  assert 'attention_fwd_f32' in names and 'attention_bwd_f32' in names and not any('attention_mh' in n for n in names)
