"""A tiny NCSNpp(resblock_type='ddpm', fir=True, resamp_with_conv=True) -- the network whose Upsample is the FIR-upsampling
convolution -- on the GPU against tests/golden/model_vp_ddpm_fir.npz: the reference's own network, loss, Adam and EMA with this
repository's restatement standing in for its one broken function (tools/make_golden_upconv.py).  Reads only the fixture.
Tolerances are those of tests/_model_cases.py for the VP family.  The training steps seed numpy's stream, which draws
the truncation time, with the fixture's step{i}.np_seed: draws at which the float32 normalising constant of the importance-
sampled times does not hang on the last place of the host's exp (tools/make_golden_upconv.py says why)."""
import os
import sys

import numpy as np
import pytest
import torch

from _model_cases import TOL
from _model_util import make_state, patched_rng, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, 'tools') not in sys.path:
  sys.path.insert(0, os.path.join(ROOT, 'tools'))

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'model_vp_ddpm_fir.npz')


@pytest.fixture(scope='module')
def fx():
  return {k: torch.from_numpy(v) for k, v in np.load(GOLDEN).items()}


def _model(st, lib, fx):
  import make_golden_upconv as mk
  dev = torch.device('cuda:0')
  cfg = mk.shrink(st.configs.cifar10_ddpmpp_nll_st())
  cfg.device = dev
  sde = st.sde_lib.get_sde(cfg, None)
  torch.manual_seed(0)
  net = st.models.ncsnpp.NCSNpp(cfg, sde)
  net.set_backend(lib)
  model = st.models.utils.DataParallel(net.to(dev))
  model.load_state_dict({k[3:]: v for k, v in fx.items() if k.startswith('sd.')})
  net.engine().ensure_flat()
  G = net.engine().program(4, 16, 16, True).graph
  import importlib
  UpConv = importlib.import_module('soft-truncation_amd.engine.graph').UpConv
  assert sum(isinstance(op, UpConv) for op in G.ops) == 1      # one Upsample between the two levels
  return cfg, sde, model


def test_forward_and_backward_match_the_fixture(st, hip_lib, fx):
  cfg, sde, model = _model(st, hip_lib, fx)
  dev = cfg.device
  model.eval()
  x = fx['x'].to(dev).requires_grad_(True)
  y = model(x, fx['cond'].to(dev))
  e = rel_err(y, fx['net'])
  print(f'ddpm-fir model: forward {e:.3e}')
  assert e <= TOL, f'forward mismatch {e:.3e}'
  (y * fx['go'].to(dev)).sum().backward()
  e = rel_err(x.grad, fx['gx'])
  print(f'ddpm-fir model: input gradient {e:.3e}')
  assert e <= TOL, f'input-gradient mismatch {e:.3e}'
  want = {k[5:]: v for k, v in fx.items() if k.startswith('grad.')}
  scale = max(g.abs().max().item() for g in want.values())
  worst, wk = 0.0, None
  for k, p in model.named_parameters():
    if not p.requires_grad:
      continue
    g = want[k]
    per = max(g.abs().max().item(), 1e-3 * scale)
    e = (p.grad.detach().cpu() - g).abs().max().item() / per
    if e > worst:
      worst, wk = e, k
  print(f'ddpm-fir model: parameter gradients {worst:.3e} at {wk}')
  assert worst <= TOL, f'parameter gradient mismatch {worst:.3e} at {wk}'


def test_three_training_steps_match_the_fixture(st, hip_lib, fx):
  cfg, sde, model = _model(st, hip_lib, fx)
  dev = cfg.device
  state = make_state(st, cfg, model)
  state['optimizer']._backend = hip_lib
  state['ema'].set_backend(hip_lib)
  step_fn = st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg))
  steps = 3
  for i in range(steps):
    np.random.seed(int(fx[f'step{i}.np_seed']))       # a well-conditioned t_min draw: tools/make_golden_upconv.py
    with patched_rng(50 + i):
      loss = step_fn(state, fx[f'step{i}.batch'].to(dev))
    e = rel_err(loss, fx[f'step{i}.loss'])
    print(f'ddpm-fir model: step {i} loss {e:.3e}')
    assert e <= TOL, f'step {i}: loss mismatch {e:.3e}'
  lr = float(fx['lr'])
  assert lr == cfg.optim.lr
  for k, p in model.named_parameters():
    if p.requires_grad:
      d = (p.detach().cpu() - fx['after.' + k]).abs().max().item()
      assert d <= 0.05 * lr * steps + 1e-7, f'{k}: parameter drift {d:.3e} after {steps} steps'
