#!/usr/bin/env python
"""The launches of consistency training and sampling (include/stk_consistency.h) measured on the GPU, beside their torch
compositions.

Part 1, at (B, n) = (16, 3 * 256^2) and (128, 3 * 32^2): back-to-back launches between two device events, on ONE set of buffers
(resident in the 256 MB Infinity Cache where it fits) and on a rotation of sets (up to 64, together 1 GiB where that many fit:
every launch from HBM).  Five rounds, the forms alternating inside each round, their order reversed in every second round;
the figure is the median of the five.  TB/s are those of the algorithmic byte count, in bytes per element:

  pair               stk_ct_pair_f32: read y, n, write xin_hi, xin_lo                                                 16
  two perturbs       two stk_perturb_f32 launches of stk.h: read y, n, write xin, twice                               24
  torch pair         a y + s n at both levels by torch operators: counted as the 16 of the pair
  loss pair          stk_ct_loss_f32 (read F_hi, F_lo, y, n, write r: 20) and stk_ct_loss_grad_f32 in place on r (8)  28
  torch loss pair    the torch-expression tail of losses.ConsistencyLoss behind F_hi, forward and autograd backward:
                     counted as the 28 of the loss pair, whatever torch moves
  step               stk_ct_step_f32 with noise: read x, F, z, write x, xin                                           20
  torch step         x0 = clamp(cs x + co F); x = x0 + c_z z; xin = c x: counted as 20
  last step          stk_ct_step_f32 without noise: read x, F, write x0                                               12
  torch last step    x0 = clamp(cs x + co F): counted as 12

Part 2, on the CIFAR-10 DDPM++ network with random weights, wall time over a synchronisation, median of five alternating
rounds: one training step under configs.consistency beside the step under configs.edm on the same batch, and a 1-step and a
2-step consistency run beside the 18-step EDM Heun run (35 evaluations).

Writes profiles/consistency_eval.txt.  Sample quality is not measured: no checkpoint trained under this formulation exists.

    python tools/consistency_eval.py
"""
import argparse
import gc
import os
import statistics

import torch

import _sampler_eval as E
from _sampler_eval import st

ap = argparse.ArgumentParser()
ap.add_argument('--shapes', nargs='*', default=['16,196608', '128,3072'], help='B,n')
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--batch', type=int, default=128, help='batch of the whole-run and training-step parts')
ap.add_argument('--skip-network', action='store_true', help='part 1 only')
ap.add_argument('--out', default=os.path.join(E.ROOT, 'profiles', 'consistency_eval.txt'))
args = ap.parse_args()
assert torch.cuda.is_available(), 'consistency_eval.py measures on the GPU: there is nothing to report without one'
device = torch.device('cuda', 0)
ROW = (0.27, 0.426, -1., 1., 0.05, 1.99)   # (cs, co, lo, hi, c_z, c_in_next): a step at 0.821 towards 0.05, clamped
PAIRS = ('pair', 'loss pair', 'step', 'last step')


def measure(lib, B, n, lines):
  total = B * n
  per_set = 9 * 4 * total                       # y, n, F_hi, F_lo, z, r, and three outputs
  sets = E.set_count(per_set)
  s = torch.cuda.current_stream().cuda_stream
  p = lambda t: t.data_ptr()
  nbytes = int(lib.ct_ws_bytes(B, n))
  ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
  lo = torch.exp(-1.1 + 2.0 * torch.randn(B, device=device)).clamp(0.002, 60.)
  hi = lo * 1.1
  coef = torch.empty(11, B, device=device)
  lib.ct_coeffs_f32(p(hi), p(lo), 0.5, 0.002, p(coef), B, s)
  c = 0.00054 * n ** 0.5
  loss, gfac, go = torch.empty(B, device=device), torch.empty(B, device=device), torch.full((B,), 1. / B, device=device)
  wide = lambda v: v[:, None]
  cs, co, lo_c, hi_c, cz, cn = ROW
  forms = {k: [] for k in ('pair', 'two perturbs', 'torch pair', 'loss pair', 'torch loss pair', 'step', 'torch step', 'last step',
                           'torch last step')}
  for _ in range(sets):
    y, nz, Fh, Fl, z = (torch.randn(B, n, device=device) * k for k in (1.5, 2.0, 1.0, 0.8, 1.0))
    r, o1, o2 = (torch.empty(B, n, device=device) for _ in range(3))

    def two_perturbs(y=y, nz=nz, o1=o1, o2=o2):
      lib.perturb_f32(p(y), p(nz), p(coef[0]), p(coef[1]), p(o1), B, n, s)
      lib.perturb_f32(p(y), p(nz), p(coef[5]), p(coef[6]), p(o2), B, n, s)

    def torch_pair(y=y, nz=nz):
      return wide(coef[0]) * y + wide(coef[1]) * nz, wide(coef[5]) * y + wide(coef[6]) * nz

    def loss_pair(Fh=Fh, Fl=Fl, y=y, nz=nz, r=r):
      lib.ct_loss_f32(p(Fh), p(Fl), p(y), p(nz), p(hi), p(lo), p(coef), c, p(ws), nbytes, p(r), p(gfac), p(loss), B, n, 1, s)
      lib.ct_loss_grad_f32(p(r), p(gfac), p(go), p(r), B, n, s)

    def torch_loss_pair(Fh=Fh, Fl=Fl, y=y, nz=nz):
      Fg = Fh.detach().requires_grad_(True)
      f_hi = wide(coef[2]) * (y + wide(hi) * nz) + wide(coef[3]) * Fg
      f_lo = wide(coef[7]) * (y + wide(lo) * nz) + wide(coef[8]) * Fl
      rr = f_hi - f_lo
      S = (rr * rr).double().sum(dim=1)
      out = ((coef[10].double() * S) / (torch.sqrt(S + c * c) + c) / n).to(torch.float32)
      out.backward(go)
      return Fg.grad

    def torch_step(x=y, F=Fh, z=z):
      x0 = torch.clamp(cs * x + co * F, lo_c, hi_c)
      xn = x0 + cz * z
      return xn, cn * xn

    forms['pair'].append(lambda y=y, nz=nz, o1=o1, o2=o2: lib.ct_pair_f32(p(y), p(nz), p(coef), p(o1), p(o2), B, n, s))
    forms['two perturbs'].append(two_perturbs)
    forms['torch pair'].append(torch_pair)
    forms['loss pair'].append(loss_pair)
    forms['torch loss pair'].append(torch_loss_pair)
    forms['step'].append(lambda x=y, F=Fh, z=z, o1=o1, o2=o2: lib.ct_step_f32(p(x), p(F), p(z), cs, co, lo_c, hi_c, cz, cn, None, p(o1),
                                                                             p(o2), total, s))
    forms['torch step'].append(torch_step)
    forms['last step'].append(lambda x=y, F=Fh, o1=o1: lib.ct_step_f32(p(x), p(F), None, cs, co, lo_c, hi_c, 0., 0., p(o1), None, None,
                                                                      total, s))
    forms['torch last step'].append(lambda x=y, F=Fh: torch.clamp(cs * x + co * F, lo_c, hi_c))
  per_elem = {'pair': 16, 'two perturbs': 24, 'torch pair': 16, 'loss pair': 28, 'torch loss pair': 28, 'step': 20, 'torch step': 20,
              'last step': 12, 'torch last step': 12}
  lines.append(f'  (B, n) = ({B}, {n}), {4 * total / 2 ** 20:.1f} MiB per tensor, {sets} buffer sets in the rotation '
               f'({sets * per_set / 2 ** 20:.0f} MiB):')
  for label, pick in (('one set (cache-resident where it fits)', lambda c_: c_[:1]), ('rotating sets', lambda c_: c_)):
    rounds = [{k: E.timed(pick(forms[k]), args.reps) for k in (list(forms) if r_ % 2 == 0 else reversed(list(forms)))}
              for r_ in range(args.rounds)]
    med = {k: statistics.median(r_[k] for r_ in rounds) for k in forms}
    lines.append(f'    {label}:')
    for k in forms:
      lines.append(f'      {k:18s} {med[k]:9.1f} us = {per_elem[k] * total / (med[k] * 1e-6) / 1e12:5.2f} TB/s of {per_elem[k]} B per element')
    lines.append('      fused / torch: ' + ', '.join(f'{k} {med[k] / med["torch " + k]:.3f}x' for k in PAIRS)
                 + f';  pair / two perturbs {med["pair"] / med["two perturbs"]:.3f}x')


def network_parts(lines):
  B = args.batch
  base = st.configs.get_config('cifar10_ddpmpp_nll_st')
  base.device = device
  edm, ct = st.configs.edm(base), st.configs.consistency(base)
  shape = (B, 3, 32, 32)
  inv = lambda v: v
  runs, steps = {}, {}
  for name, cfg in (('edm', edm), ('ct', ct)):
    sde = st.sde_lib.get_sde(cfg, None)
    torch.manual_seed(0)
    model = st.models.utils.create_model(cfg, sde)
    model.eval()
    if name == 'edm':
      sample = st.edm.get_edm_sampler(cfg, sde, shape, inv, steps=18, device=device)
      runs['heun'] = (lambda sample=sample, model=model: sample(model))
    else:
      for key, levels in (('one', (80.,)), ('two', (80., 0.821))):
        sample = st.consistency.get_consistency_sampler(cfg, sde, shape, inv, levels=levels, device=device)
        runs[key] = (lambda sample=sample, model=model: sample(model))
    opt = st.losses.get_optimizer(cfg, model.parameters())
    ema = st.models.ema.ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate)
    state = dict(optimizer=opt, model=model, ema=ema, step=0)
    step_fn = st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg))
    batch = st.datasets.synthetic_batch(cfg, B, device=device, generator=torch.Generator().manual_seed(4321))
    steps[name] = (lambda step_fn=step_fn, state=state, batch=batch: [step_fn(state, batch) for _ in range(5)])
  ms = E.wall(steps, args.rounds)
  lines.append(f'  training step on the CIFAR-10 DDPM++ network, batch {B}, dropout {base.model.dropout} (five steps per figure):')
  lines.append(f'    EDM step (configs.edm)                   {ms["edm"] / 5:7.2f} ms = {B / (ms["edm"] / 5) * 1e3:.0f} images/s')
  lines.append(f'    consistency step (configs.consistency)   {ms["ct"] / 5:7.2f} ms = {B / (ms["ct"] / 5) * 1e3:.0f} images/s'
               f' = {ms["ct"] / ms["edm"]:.3f}x the EDM step')
  ms = E.wall(runs, args.rounds)
  lines.append(f'  whole run, batch {B}, random weights:')
  lines.append(f'    EDM Heun, 18 steps (35 evaluations)        {ms["heun"]:8.1f} ms = {ms["heun"] / 35:.2f} ms per evaluation')
  lines.append(f'    consistency, 1 step  (1 evaluation)        {ms["one"]:8.1f} ms = {ms["one"] / ms["heun"]:.4f}x the Heun run')
  lines.append(f'    consistency, 2 steps (2 evaluations)       {ms["two"]:8.1f} ms = {ms["two"] / ms["heun"]:.4f}x the Heun run')


lines = ['consistency_eval.py: the launches of consistency training and sampling on one MI355X.',
         f'{args.reps} calls per figure, {args.rounds} alternating rounds, medians.  torch {torch.__version__}.']
lib = st.engine.lib.load()
for spec in args.shapes:
  B, n = (int(v) for v in spec.split(','))
  measure(lib, B, n, lines)
  gc.collect()
  torch.cuda.empty_cache()
if not args.skip_network:
  network_parts(lines)
lines.append('Sample quality is unmeasured: no checkpoint trained under this formulation exists.')
E.write(lines, args.out)
