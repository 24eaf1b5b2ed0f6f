"""config.model.scale_shift_norm on the device against the float64 / oracle restatement of tests/_adagn_ref.py: the network
(tiny families vp, rve, wide; with classes; training steps; the input-only backward; dropout), the stand-alone residual
blocks, and the switch set to False.  Tolerances: TOL = 2e-4 of tests/_model_cases.py for the network, GN_RTOL = 2e-5 of
tests/_block_cases.py for the blocks."""
import copy

import numpy as np
import pytest
import torch

import _adagn_ref as R
from _block_cases import GN_RTOL, compare_param_grads
from _model_cases import TOL, _inputs
from _model_util import grads_close, make_state, patched_rng, randomize_, rel_err, tiny_config
from _util import close

pytestmark = pytest.mark.gpu

FAMILIES = ['vp', 'rve', 'wide']
_built = {}


def _build(st, lib, family, switch=True, num_classes=0, dropout=0.0):
  """(cfg, cfg_cpu, sde, model, host state_dict) of a tiny network with randomised weights."""
  key = (family, switch, num_classes, dropout)
  if key in _built:
    return _built[key]
  cfg = tiny_config(st, family, dropout=dropout)
  if switch is not None:
    cfg.model.scale_shift_norm = switch
  if num_classes:
    cfg.model.num_classes = num_classes
  cfg.device = torch.device('cuda:0')
  sde = st.sde_lib.get_sde(cfg, None)
  torch.manual_seed(0)
  net = st.models.ncsnpp.NCSNpp(cfg, sde)
  net.set_backend(lib)
  net = net.to(cfg.device)
  randomize_(net, 0)
  if num_classes:
    # rows of 0.1 randn move the embedding by a fraction of its own size and the output by ~1e-2 relative: rows of 0.4 randn
    # make the class matter as much as the noise level does, so that a lost class row cannot hide in the tolerance
    with torch.no_grad():
      net.class_emb.weight.mul_(4.0)
  model = st.models.utils.DataParallel(net)
  net.engine().ensure_flat()
  model.eval()
  cfg_cpu = copy.deepcopy(cfg)
  cfg_cpu.device = torch.device('cpu')
  sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
  _built[key] = (cfg, cfg_cpu, sde, model, sd)
  return _built[key]


def _zero_grads(model):
  model.zero_grad()
  for p in model.parameters():
    if p.grad is not None:
      p.grad.zero_()


@pytest.mark.parametrize('family', FAMILIES)
def test_forward_backward_against_the_reference(st, hip_lib, family):
  cfg, cfg_cpu, sde, model, sd = _build(st, hip_lib, family)
  ref = st.models.utils.DataParallel(R.AdaRefNet(cfg_cpu, sd)).eval()
  dev = cfg.device
  x, t, cond = _inputs(cfg, sde, 3)
  _zero_grads(model)
  xg = x.clone().to(dev).requires_grad_(True)
  y = model(xg, cond.to(dev))
  xr = x.clone().requires_grad_(True)
  yr = ref(xr, cond)
  assert rel_err(y, yr) <= TOL, f'forward mismatch {rel_err(y, yr):.3e}'
  go = torch.randn(yr.shape, generator=torch.Generator().manual_seed(5))
  (y * go.to(dev)).sum().backward()
  (yr * go).sum().backward()
  assert rel_err(xg.grad, xr.grad) <= TOL, f'input-gradient mismatch {rel_err(xg.grad, xr.grad):.3e}'
  grads_close(model, ref, TOL)
  # a second forward under no_grad (sampling path) gives the same values
  with torch.no_grad():
    assert torch.equal(model(x.to(dev), cond.to(dev)), y.detach())


def _bias_key(cfg):
  return f'module.all_modules.{2 if cfg.model.embedding_type == "fourier" else 1}.bias'


def _ref_name(key):
  return key[len('module.'):].replace('.', '__')


@pytest.mark.parametrize('family', FAMILIES)
def test_mixed_class_batch(st, hip_lib, family):
  """num_classes = 3: per class the network is AdaRefNet with table[c] added to the bias of the time MLP's second layer
  (tests/test_gpu_class_cond_model.py); the class reaches the blocks through the modulation alone."""
  mu = st.models.utils
  C = 3
  cfg, cfg_cpu, sde, model, sd = _build(st, hip_lib, family, num_classes=C)
  net, dev = model.module, cfg.device
  classes, rows = [1, 1, None, 0], [1, 1, C, 0]
  x, t, cond = _inputs(cfg, sde, 4)
  go = torch.randn(x.shape, generator=torch.Generator().manual_seed(5))
  _zero_grads(model)
  xg = x.clone().to(dev).requires_grad_(True)
  with mu.class_condition(model, classes):
    y = model(xg, cond.to(dev))
  (y * go.to(dev)).sum().backward()

  yr, gxr, grads, row_grads = torch.zeros_like(x), torch.zeros_like(x), {}, {}
  for c in sorted(set(rows)):
    idx = [i for i, r in enumerate(rows) if r == c]
    shifted = {k: v.clone() for k, v in sd.items() if k != 'module.class_emb.weight'}
    shifted[_bias_key(cfg_cpu)] += sd['module.class_emb.weight'][c]
    ref = R.AdaRefNet(cfg_cpu, shifted).eval()
    xr = x[idx].clone().requires_grad_(True)
    out = ref(xr, cond[idx])
    (out * go[idx]).sum().backward()
    yr[idx], gxr[idx] = out.detach(), xr.grad
    for k, p in ref.named_parameters():
      if p.grad is not None:
        grads[k] = grads.get(k, 0) + p.grad
    row_grads[c] = getattr(ref, _ref_name(_bias_key(cfg))).grad
  assert rel_err(y, yr) <= TOL, f'forward mismatch {rel_err(y, yr):.3e}'
  assert rel_err(xg.grad, gxr) <= TOL, f'input-gradient mismatch {rel_err(xg.grad, gxr):.3e}'
  scale = max(g.abs().max().item() for g in grads.values())
  for k, p in model.named_parameters():
    if not p.requires_grad or k == 'module.class_emb.weight':
      continue
    g = grads[_ref_name(k)]
    e = (p.grad.detach().cpu() - g).abs().max().item() / max(g.abs().max().item(), 1e-3 * scale)
    assert e <= TOL, f'parameter gradient mismatch {e:.3e} at {k}'
  gtab = net.class_emb.weight.grad.detach().cpu()
  for c, g in row_grads.items():
    e = (gtab[c] - g).abs().max().item() / max(g.abs().max().item(), 1e-3 * scale)
    assert e <= TOL, f'table gradient mismatch {e:.3e} at row {c}'
  # the modulation differs per class: the same samples under other classes give another output
  with torch.no_grad():
    with mu.class_condition(model, [None] * 4):
      u = model(x.to(dev), cond.to(dev))
  assert rel_err(y[:2], u[:2]) > 100 * TOL and rel_err(y[3:], u[3:]) > 100 * TOL, 'the classes do not reach the output'
  assert rel_err(y[2:3], u[2:3]) <= TOL


@pytest.mark.parametrize('family', FAMILIES)
def test_two_training_steps_against_torch_adam(st, hip_lib, family):
  """tests/_model_cases.py train_steps with the switch: losses within TOL, parameters and EMA within 5 % of the total update."""
  steps, B = 2, 4
  base = tiny_config(st, family)
  base.model.scale_shift_norm = True
  base.optim.warmup = 2
  cfg, cfg_cpu = copy.deepcopy(base), copy.deepcopy(base)
  cfg.device, cfg_cpu.device = torch.device('cuda:0'), torch.device('cpu')
  sde = st.sde_lib.get_sde(cfg, None)
  torch.manual_seed(0)
  net = st.models.ncsnpp.NCSNpp(cfg, sde)
  net.set_backend(hip_lib)
  net = net.to(cfg.device)
  randomize_(net, 0)
  model = st.models.utils.DataParallel(net)
  net.engine().ensure_flat()
  sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
  ref = st.models.utils.DataParallel(R.AdaRefNet(cfg_cpu, sd))
  state = make_state(st, cfg, model)
  assert type(state['optimizer']).__name__ == 'FusedAdam'
  state['optimizer']._backend = hip_lib
  state['ema'].set_backend(hip_lib)
  rstate = make_state(st, cfg_cpu, ref)
  step_fn = st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg))
  rstep_fn = st.losses.get_step_fn(cfg_cpu, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg_cpu))
  for i in range(steps):
    batch = st.datasets.synthetic_batch(cfg_cpu, B, generator=torch.Generator().manual_seed(100 + i))
    np.random.seed(7 + i)
    with patched_rng(50 + i):
      loss = step_fn(state, batch.to(cfg.device))
    np.random.seed(7 + i)
    with patched_rng(50 + i):
      rloss = rstep_fn(rstate, batch)
    assert loss.shape == rloss.shape and rel_err(loss, rloss) <= TOL, f'step {i}: loss mismatch {rel_err(loss, rloss):.3e}'
  lr = cfg.optim.lr
  moved = 0.0
  for (k, p), (rk, rp) in zip(model.named_parameters(), ref.named_parameters()):
    if not p.requires_grad:
      continue
    d = (p.detach().cpu() - rp.detach()).abs().max().item()
    assert d <= 0.05 * lr * steps + 1e-7, f'{k}: parameter drift {d:.3e} after {steps} steps'
    if '.Dense_0.' in k:
      moved = max(moved, (p.detach().cpu() - sd[k]).abs().max().item())
  assert moved > 0.5 * lr, f'the conditioning projections moved by {moved:.3e} only'
  for s, rs in zip(state['ema'].shadow_params, rstate['ema'].shadow_params):
    assert (s.detach().cpu() - rs).abs().max().item() <= 0.05 * lr * steps + 1e-7


def test_input_only_backward_gives_the_same_input_gradient(st, hip_lib):
  cfg, _, sde, model, _ = _build(st, hip_lib, 'vp')
  net = model.module
  x, t, cond = _inputs(cfg, sde, 3)
  x, cond = x.to(cfg.device), cond.to(cfg.device)
  go = torch.randn(x.shape, generator=torch.Generator().manual_seed(5)).to(cfg.device)
  _zero_grads(model)
  xg = x.clone().requires_grad_(True)
  (model(xg, cond) * go).sum().backward()
  full = xg.grad.clone()
  flat_grad = net.engine().flat.grad
  flat_grad.fill_(7.0)
  for _ in range(2):                  # the second call replays the captured backward
    xi = x.clone().requires_grad_(True)
    gx, = torch.autograd.grad((model(xi, cond) * go).sum(), xi)
    assert rel_err(gx, full) <= 1e-6, f'input-only backward {rel_err(gx, full):.3e} from the full one'
    assert bool((flat_grad == 7.0).all()), 'an input-only backward wrote a parameter gradient'
  _zero_grads(model)


def test_dropout_same_seed_same_bits(st, hip_lib):
  cfg, _, sde, model, _ = _build(st, hip_lib, 'vp', dropout=0.1)
  x, t, cond = _inputs(cfg, sde, 2)
  x, cond = x.to(cfg.device), cond.to(cfg.device)
  model.train()
  try:
    outs = []
    for seed in (123, 123, 124):
      torch.manual_seed(seed)           # the engine draws its per-call dropout seed from torch's CPU generator
      xg = x.clone().requires_grad_(True)
      y = model(xg, cond)
      gx, = torch.autograd.grad(y.sum(), xg)
      outs.append((y.detach().clone(), gx.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][0], outs[2][0]), 'dropout does not depend on the seed'
  finally:
    model.eval()
  with torch.no_grad():
    assert not torch.equal(model(x, cond), outs[0][0]), 'dropout is not applied in training mode'


BLOCKS = {
  'biggan_plain_b3_16': ('ResnetBlockBigGANpp', dict(in_ch=64, out_ch=64, temb_dim=48), (3, 64, 16, 16)),
  'biggan_down_fir_64to128_b2_16': ('ResnetBlockBigGANpp', dict(in_ch=64, out_ch=128, temb_dim=32, down=True, fir=True),
                                    (2, 64, 16, 16)),
  'biggan_up_naive_b1_8': ('ResnetBlockBigGANpp', dict(in_ch=32, out_ch=32, temb_dim=32, up=True, skip_rescale=False),
                           (1, 32, 8, 8)),
  'ddpm_nin_shortcut_b3_16': ('ResnetBlockDDPMpp', dict(in_ch=64, out_ch=128, temb_dim=64, skip_rescale=True), (3, 64, 16, 16)),
  'ddpm_conv_shortcut_b1_8': ('ResnetBlockDDPMpp', dict(in_ch=32, out_ch=64, temb_dim=32, conv_shortcut=True), (1, 32, 8, 8)),
}


@pytest.mark.parametrize('case', list(BLOCKS))
def test_stand_alone_blocks(st, hip_lib, case):
  cls, kw, shape = BLOCKS[case]
  torch.manual_seed(0)
  m = getattr(st.models.layerspp, cls)(act=torch.nn.SiLU(), dropout=0., scale_shift_norm=True, **kw)
  g = torch.Generator().manual_seed(1)
  with torch.no_grad():
    for n, p in m.named_parameters():
      if n.endswith('GroupNorm_0.weight') or n.endswith('GroupNorm_1.weight'):
        p.copy_(1 + 0.2 * torch.randn(p.shape, generator=g))
      else:
        p.copy_(0.1 * torch.randn(p.shape, generator=g))
  dev = torch.device('cuda:0')
  m = m.to(dev).eval()
  m.set_backend(hip_lib)
  g = torch.Generator().manual_seed(2)
  x = torch.randn(shape, generator=g).to(dev).requires_grad_(True)
  temb = torch.randn(shape[0], kw['temb_dim'], generator=g).to(dev).requires_grad_(True)
  out = m(x, temb)
  gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).to(dev)
  want_out, want_in, want_p = R.block_run(m, x, temb, gout)
  close(out, want_out, rtol=GN_RTOL, what=f'{case}: output')
  m.zero_grad(set_to_none=False)
  out.backward(gout)
  close(x.grad, want_in['x'], rtol=GN_RTOL, what=f'{case}: dx')
  close(temb.grad, want_in['temb'], rtol=GN_RTOL, what=f'{case}: dtemb')
  named = dict(m.named_parameters())
  compare_param_grads({n: named[n].grad for n in want_p}, want_p, GN_RTOL, case)
  # the input-only backward (no parameter asked for): temb's gradient comes through d(scale), d(shift) alone.  Twice: the
  # second call replays what the first one planned
  for _ in range(2):
    gx, gt = torch.autograd.grad(m(x, temb), (x, temb), gout)
    close(gx, want_in['x'], rtol=GN_RTOL, what=f'{case}: dx, input-only')
    close(gt, want_in['temb'], rtol=GN_RTOL, what=f'{case}: dtemb, input-only')
  gt, = torch.autograd.grad(m(x.detach(), temb), temb, gout)
  close(gt, want_in['temb'], rtol=GN_RTOL, what=f'{case}: dtemb alone')
  with pytest.raises(ValueError, match='needs temb'):
    m(x.detach())


@pytest.mark.parametrize('family', ['vp', 'wide'])
def test_switch_off_is_the_network_without_the_key(st, hip_lib, family):
  cfg, _, sde, off, sd_off = _build(st, hip_lib, family, switch=False)
  _, _, _, plain, sd = _build(st, hip_lib, family, switch=None)
  assert list(sd) == list(sd_off) and all(torch.equal(sd[k], sd_off[k]) for k in sd)
  x, t, cond = _inputs(cfg, sde, 3)
  x, cond = x.to(cfg.device), cond.to(cfg.device)
  with torch.no_grad():
    assert torch.equal(off(x, cond), plain(x, cond))
  go = torch.randn(x.shape, generator=torch.Generator().manual_seed(5)).to(cfg.device)
  gs = []
  for model in (off, plain):
    _zero_grads(model)
    xg = x.clone().requires_grad_(True)
    (model(xg, cond) * go).sum().backward()
    gs.append((xg.grad.clone(), model.module.engine().flat.grad.clone()))
  assert torch.equal(gs[0][0], gs[1][0]) and torch.equal(gs[0][1], gs[1][1])


def test_guidance_fp16_modes_and_a_sampler_see_an_ordinary_network(st, hip_lib):
  """The wide family (its 3x3 convolutions take planes: Conv_1 now makes its own from the modulated layer's fp32 output)
  with classes: guidance at batch 2 B, the fp16 sampling and training modes, and a PC sampler."""
  mu = st.models.utils
  cfg, _, sde, model, _ = _build(st, hip_lib, 'wide', num_classes=3)
  dev = cfg.device
  x, t, cond = _inputs(cfg, sde, 3)
  x, cond = x.to(dev), cond.to(dev)
  y = torch.tensor([2, 0, 3])
  with torch.no_grad():
    with mu.class_condition(model, y):
      c = model(x, cond)
    with mu.class_condition(model, [None] * 3):
      u = model(x, cond)
    with mu.class_condition(model, y, guidance=1.5):
      g = model(x, cond)
    assert rel_err(g, c + 1.5 * (c - u)) <= TOL, f'guided evaluation off by {rel_err(g, c + 1.5 * (c - u)):.3e}'
    with mu.precision(model, 'fp16'), mu.class_condition(model, y):
      h = model(x, cond)
  # one fp16 x fp16 product per multiply-add: each operand keeps 11 bits, a product is within 2^-10 of the fp32 one, and
  # the errors of a sum do not all add up: ten times that bounds the output of a network this shallow with room to spare
  e = rel_err(h, c)
  assert 0 < e <= 10 * 2.0 ** -10, f'fp16 evaluation {e:.3e} from the fp32 one'
  go = torch.randn(x.shape, generator=torch.Generator().manual_seed(5)).to(dev)
  grads = []
  for prec in ('fp32', 'fp16'):
    _zero_grads(model)
    xg = x.clone().requires_grad_(True)
    with mu.training_precision(model, prec), mu.class_condition(model, y):
      (model(xg, cond) * go).sum().backward()
    grads.append(xg.grad.clone())
  assert bool(torch.isfinite(grads[1]).all()) and 0 < rel_err(grads[1], grads[0]) < 0.1
  _zero_grads(model)
  c2 = copy.deepcopy(cfg)
  c2.sampling.method, c2.sampling.predictor, c2.sampling.corrector = 'pc', 'euler_maruyama', 'none'
  s2 = copy.deepcopy(sde)
  s2.N = 3
  shape = (2, cfg.data.num_channels, cfg.data.image_size, cfg.data.image_size)
  fn = st.sampling.get_sampling_fn(c2, s2, shape, st.datasets.get_data_inverse_scaler(c2), 1e-3)
  outs = []
  for classes in ([0, 2], [0, 2], [1, 1]):
    torch.manual_seed(3)
    with mu.class_condition(model, classes, 1.5):
      outs.append(fn(model)[0])
  assert outs[0].shape == shape and bool(torch.isfinite(outs[0]).all())
  assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
