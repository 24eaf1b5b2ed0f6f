#!/usr/bin/env python
"""Generate tests/golden/model_vp_ddpm_fir.npz: the reference's own NCSNpp with resblock_type='ddpm', fir=True and
resamp_with_conv=True -- the network whose Upsample goes through upsample_conv_2d -- on small seeded inputs.

    python tools/make_golden_upconv.py          (where the reference is present; it never travels)

The reference's upsample_conv_2d raises (its weight reversal is a negative-stride slice).  The live reference is imported
through oracle/refimport.py and that one function is replaced AT RUN TIME by this repository's float32 restatement of what it
means (tests/_upconv_ref.py); everything else -- the network, the loss, the optimizer, the EMA -- is the reference's.  The
fixture is data only: the state_dict, the inputs and every noise draw made explicit, outputs, gradients and losses.

The training steps draw their truncation time t_min from numpy's stream (sde_lib.py:200-207), log-uniform down to 1e-5.
The importance-sampled times and their normalising constant then go through A(t_min) = log(1 - exp(-B(t_min))) + B(t_min)
in float32 on the host (sde_lib.py:183-198), and 1 - exp(-B) keeps only B / 2^-24 units of its last place: at
t_min = 2.4e-5 that is 40 of them, so two hosts whose exp differ in the last place disagree by 2.5 % in that term and by
1e-3 in the loss -- five times the tolerance of the comparison, with the network right to 5e-7.  Such a draw pins a
host's libm, not this repository, so the steps are seeded (T_MIN_SEEDS, recorded in the fixture as step{i}.np_seed) with
draws whose last-place sensitivity 2^-24 / (1 - exp(-B(t_min))) is at most T_MIN_SENSITIVITY = 1e-5, a twentieth of the
tolerance; generate() asserts it.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
  if p not in sys.path:
    sys.path.insert(0, p)

import numpy as np
import torch

import _upconv_ref
import refimport
from _model_util import patched_rng

OUT = os.path.join(ROOT, 'tests', 'golden', 'model_vp_ddpm_fir.npz')
STEPS = 3
T_MIN_SEEDS = (51, 10, 8)          # t_min = 2.4e-2, 7.2e-2, 2.3e-1
T_MIN_SENSITIVITY = 1e-5


def shrink(cfg):
  """The fixture's network, on the reference's config or on this package's restatement of it (same field names)."""
  cfg.model.nf = 8
  cfg.model.ch_mult = (1, 2)
  cfg.model.num_res_blocks = 1
  cfg.model.attn_resolutions = (8,)
  cfg.model.dropout = 0.0
  cfg.model.resblock_type = 'ddpm'
  cfg.model.fir = True
  cfg.model.resamp_with_conv = True
  cfg.data.image_size = 16
  cfg.optim.warmup = 2
  return cfg


def npy(t):
  return t.detach().cpu().numpy().copy()


def _upsample_conv_2d(x, w, k=None, factor=2, gain=1):
  assert factor == 2 and x.shape[1] == w.shape[1]
  return _upconv_ref.forward(x, w, k, gain)[0]


def t_min_sensitivity(sde, cfg, seed):
  """Relative change of 1 - exp(-B(t_min)) per last place of the float32 exp, for the t_min that `seed` draws."""
  np.random.seed(seed)
  t_min = sde.get_t_min(cfg)
  return 2. ** -24 / -np.expm1(-float(sde.integral_beta(t_min)))


def generate():
  """name -> array, from the live reference."""
  ns = refimport.load()
  cfg = shrink(refimport.get_config('configs.vp.CIFAR10.ddpmpp_nll_st'))
  saved = ns.uds.upsample_conv_2d
  ns.uds.upsample_conv_2d = _upsample_conv_2d
  try:
    torch.manual_seed(0)
    sde = ns.sde_lib.get_sde(cfg, None)
    model = ns.mutils.create_model(cfg, sde)
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
      for p in model.parameters():
        if p.requires_grad:
          p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    out = {'sd.' + k: npy(v) for k, v in model.state_dict().items()}
    B, H = 4, cfg.data.image_size
    x = torch.randn(B, 3, H, H, generator=g)
    t = torch.rand(B, generator=g) * 0.9 + 0.05
    cond = t * 999
    model.eval()
    xr = x.clone().requires_grad_(True)
    y = model(xr, cond)
    go = torch.randn(y.shape, generator=g)
    (y * go).sum().backward()
    out.update(x=npy(x), cond=npy(cond), net=npy(y), go=npy(go), gx=npy(xr.grad))
    for n, p in model.named_parameters():
      if p.grad is not None:
        out['grad.' + n] = npy(p.grad)
    # training steps through the reference's own step_fn (noise injected)
    model.zero_grad()
    opt = ns.losses.get_optimizer(cfg, model.parameters())
    ema = ns.ema.ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate)
    state = dict(optimizer=opt, model=model, ema=ema, step=0)
    step_fn = ns.losses.get_step_fn(cfg, sde, train=True, optimize_fn=ns.losses.optimization_manager(cfg))
    for i in range(STEPS):
      batch = torch.rand(B, 3, H, H, generator=torch.Generator().manual_seed(100 + i)) * 2. - 1.
      seed = T_MIN_SEEDS[i]
      assert t_min_sensitivity(sde, cfg, seed) <= T_MIN_SENSITIVITY, f'step {i}: seed {seed} draws an ill-conditioned t_min'
      np.random.seed(seed)
      with patched_rng(50 + i):
        losses = step_fn(state, batch)
      out[f'step{i}.batch'], out[f'step{i}.loss'] = npy(batch), npy(losses)
      out[f'step{i}.np_seed'] = np.asarray(seed, dtype=np.int64)
    for n, p in model.named_parameters():
      out['after.' + n] = npy(p)
    out['lr'] = np.asarray(cfg.optim.lr, dtype=np.float64)
    return out
  finally:
    ns.uds.upsample_conv_2d = saved


def main():
  out = generate()
  np.savez_compressed(OUT, **out)
  print('wrote', OUT, os.path.getsize(OUT), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
  main()
