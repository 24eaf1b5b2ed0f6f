#!/usr/bin/env python
"""The EDM loss pair and sampler launches (include/stk_edm.h) measured on the GPU, beside their torch compositions.

Part 1, at (B, n) = (16, 3 * 256^2) and (128, 3 * 32^2): back-to-back launches between two device events, on ONE set of buffers
(resident in the 256 MB Infinity Cache where it fits) and on a rotation of sets (up to 64, together 1 GiB where that many fit:
every launch from HBM).  Five rounds, the forms alternating inside each round, their order reversed in every second round;
the figure is the median of the five.  TB/s are those of the algorithmic byte count, in bytes per element:

  dpm update         stk_dpm_update_f32, second order: read x, score, d_prev, write x, d                              20
  loss pair          stk_edm_loss_f32 (read F, y, n, write r: 16) and stk_edm_loss_grad_f32 in place on r (8)         24
  torch loss pair    the torch-expression loss of losses.get_edm_loss_fn behind F, forward and autograd backward:
                     counted as the 24 of the loss pair, whatever torch moves
  euler              stk_edm_step_f32, xe == xb: read x, F, write x', d, xin                                          20
  torch euler        D = cs x + co F; d = (x - D) / t; x' = x + h d; xin = c x': counted as 20
  correction         stk_edm_step_f32: read x^, x', F, d, write x, xin                                                24
  torch correction   the same lines with the averaged slope: counted as 24

Part 2: a whole 18-step EDM run (35 evaluations) on the CIFAR-10 DDPM++ network with random weights beside the 20-step
DPM-Solver++ run (21 evaluations) on the same network under VP, wall time over a synchronisation, median of five alternating
rounds; and one training step under configs.edm beside the VP step of the same config, the same way.

Writes profiles/edm_eval.txt.  Sample quality is not measured: no checkpoint trained under this formulation exists.

    python tools/edm_eval.py
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
ap.add_argument('--out', default=os.path.join(E.ROOT, 'profiles', 'edm_eval.txt'))
args = ap.parse_args()
assert torch.cuda.is_available(), 'edm_eval.py measures on the GPU: there is nothing to report without one'
device = torch.device('cuda', 0)
DPM_ROW = (1.3, 0.7, 0.45, 0.8, 0.35)      # (cx, cs, g, A, B): a second-order step
ROW = (0.0357, 0.491, 2.6, -0.7, 0.509)    # (cs, co, t, h, c_next): a step from t^ = 2.6 to 1.9 at sigma_data = 0.5
INF = float('inf')


def measure(lib, B, n, lines):
  total = B * n
  per_set = 9 * 4 * total                       # x, x', F, d, n, r, x-out, d-out, xin-out
  sets = E.set_count(per_set)
  s = torch.cuda.current_stream().cuda_stream
  p = lambda t: t.data_ptr()
  nbytes = int(lib.edm_ws_bytes(B, n))
  ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
  sigma = torch.exp(-1.2 + 1.2 * torch.randn(B, device=device))
  coef = torch.empty(6, B, device=device)
  lib.edm_coeffs_f32(p(sigma), 0.5, p(coef), B, s)
  loss, go = torch.empty(B, device=device), torch.full((B,), 1. / B, device=device)
  wide = lambda v: v[:, None]
  cs, co, t, h, cn = ROW
  forms = {k: [] for k in ('dpm update', 'loss pair', 'torch loss pair', 'euler', 'torch euler', 'correction', 'torch correction')}
  for _ in range(sets):
    x, x1, F, d, nz = (torch.randn(B, n, device=device) * k for k in (1.5, 2.0, 1.0, 0.8, 1.0))
    r, xo, do, xi = (torch.empty(B, n, device=device) for _ in range(4))

    def loss_pair(F=F, x=x, nz=nz, r=r):
      lib.edm_loss_f32(p(F), p(x), p(nz), p(sigma), p(coef), p(ws), nbytes, p(r), p(loss), B, n, 1, s)
      lib.edm_loss_grad_f32(p(r), p(coef), p(go), p(r), B, n, 1, s)

    def torch_loss_pair(F=F, y=x, nz=nz):
      Fg = F.detach().requires_grad_(True)
      xs = y + wide(sigma) * nz
      rr = (wide(coef[2]) * xs + wide(coef[3]) * Fg) - y
      out = (coef[4].double() * (rr * rr).double().sum(dim=1) / n).to(torch.float32)
      out.backward(go)
      return Fg.grad

    def torch_euler(x=x, F=F):
      D = cs * x + co * F
      dn = (x - D) / t
      xn = x + h * dn
      return xn, dn, cn * xn

    def torch_correction(x=x, x1=x1, F=F, d=d):
      D = cs * x1 + co * F
      dn = (x1 - D) / t
      xn = x + h * (0.5 * d + 0.5 * dn)
      return xn, cn * xn

    forms['dpm update'].append(lambda x=x, F=F, d=d, xo=xo, do=do: lib.dpm_update_f32(p(x), p(F), p(d), *DPM_ROW, -INF, INF, p(xo), p(do),
                                                                                     total, s))
    forms['loss pair'].append(loss_pair)
    forms['torch loss pair'].append(torch_loss_pair)
    forms['euler'].append(lambda x=x, F=F, xo=xo, do=do, xi=xi: lib.edm_step_f32(p(x), p(x), p(F), None, cs, co, t, h, cn, p(xo), p(do),
                                                                                p(xi), total, s))
    forms['torch euler'].append(torch_euler)
    forms['correction'].append(lambda x=x, x1=x1, F=F, d=d, xo=xo, xi=xi: lib.edm_step_f32(p(x), p(x1), p(F), p(d), cs, co, t, h, cn, p(xo),
                                                                                          None, p(xi), total, s))
    forms['torch correction'].append(torch_correction)
  per_elem = {'dpm update': 20, 'loss pair': 24, 'torch loss pair': 24, 'euler': 20, 'torch euler': 20, 'correction': 24,
              'torch correction': 24}
  lines.append(f'  (B, n) = ({B}, {n}), {4 * total / 2 ** 20:.1f} MiB per tensor, {sets} buffer sets in the rotation '
               f'({sets * per_set / 2 ** 20:.0f} MiB):')
  for label, pick in (('one set (cache-resident where it fits)', lambda c: c[:1]), ('rotating sets', lambda c: c)):
    rounds = [{k: E.timed(pick(forms[k]), args.reps) for k in (list(forms) if r % 2 == 0 else reversed(list(forms)))}
              for r in range(args.rounds)]
    med = {k: statistics.median(r[k] for r in rounds) for k in forms}
    lines.append(f'    {label}:')
    for k in forms:
      lines.append(f'      {k:18s} {med[k]:9.1f} us = {per_elem[k] * total / (med[k] * 1e-6) / 1e12:5.2f} TB/s of {per_elem[k]} B per element')
    lines.append('      fused / torch: ' + ', '.join(f'{k} {med[k] / med["torch " + k]:.3f}x' for k in ('loss pair', 'euler', 'correction')))


def network_parts(lines):
  B = args.batch
  vp = st.configs.get_config('cifar10_ddpmpp_nll_st')
  vp.device = device
  edm = st.configs.edm(vp)
  shape = (B, 3, 32, 32)
  inv = lambda v: v
  runs, steps = {}, {}
  for name, cfg in (('vp', vp), ('edm', edm)):
    sde = st.sde_lib.get_sde(cfg, None)
    torch.manual_seed(0)
    model = st.models.utils.create_model(cfg, sde)
    model.eval()
    if name == 'vp':
      sample = st.dpm_solver.get_dpm_sampler(cfg, sde, shape, inv, steps=20, order=2, denoise=True, device=device)
    else:
      sample = st.edm.get_edm_sampler(cfg, sde, shape, inv, steps=18, device=device)
    runs[name] = (lambda sample=sample, model=model: sample(model))
    opt = st.losses.get_optimizer(cfg, model.parameters())
    ema = st.models.ema.ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate)
    state = dict(optimizer=opt, model=model, ema=ema, step=0)
    step_fn = st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg))
    batch = st.datasets.synthetic_batch(cfg, B, device=device, generator=torch.Generator().manual_seed(4321))
    steps[name] = (lambda step_fn=step_fn, state=state, batch=batch: [step_fn(state, batch) for _ in range(5)])
  ms = E.wall(runs, args.rounds)
  lines.append(f'  whole run on the CIFAR-10 DDPM++ network, batch {B}, random weights:')
  lines.append(f'    DPM-Solver++ 2M, 20 steps + denoise (21 evaluations, VP)  {ms["vp"]:8.1f} ms = {ms["vp"] / 21:.2f} ms per evaluation')
  lines.append(f'    EDM Heun, 18 steps (35 evaluations)                       {ms["edm"]:8.1f} ms = {ms["edm"] / 35:.2f} ms per evaluation')
  ms = E.wall(steps, args.rounds)
  lines.append(f'  training step, batch {B} (five steps per figure):')
  lines.append(f'    VP soft-truncation step   {ms["vp"] / 5:7.2f} ms = {B / (ms["vp"] / 5) * 1e3:.0f} images/s')
  lines.append(f'    EDM step (configs.edm)    {ms["edm"] / 5:7.2f} ms = {B / (ms["edm"] / 5) * 1e3:.0f} images/s')


lines = ['edm_eval.py: the EDM loss pair and sampler launches on one MI355X.',
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
