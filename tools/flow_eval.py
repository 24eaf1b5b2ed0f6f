#!/usr/bin/env python
"""The rectified-flow loss pair and step launches (include/stk_flow.h) measured on the GPU, beside their torch compositions
and beside stk_edm_step_f32.  The protocol is that of tools/edm_eval.py.

Part 1, at (B, n) = (16, 3 * 256^2) and (128, 3 * 32^2): back-to-back launches between two device events, on ONE set of buffers
(resident in the 256 MB Infinity Cache where it fits) and on a rotation of sets (up to 64, together 1 GiB where that many fit:
every launch from HBM).  Five rounds, the forms alternating inside each round, their order reversed in every second round;
the figure is the median of the five.  TB/s are those of the algorithmic byte count, in bytes per element:

  edm euler          stk_edm_step_f32, xe == xb: read x, F, write x', d, xin                                         20
  loss pair          stk_flow_loss_f32 (read F, y, n, write r: 16) and stk_flow_loss_grad_f32 in place on r (8)      24
  torch loss pair    the torch-expression loss of losses.get_flow_loss_fn behind F, forward and autograd backward:
                     counted as the 24 of the loss pair, whatever torch moves
  euler              stk_flow_step_f32: read x, v, write x'                                                          12
  torch euler        x' = x + cv v: counted as 12
  correction         stk_flow_step_f32 with v_prev, in place: read x, v', v, write x                                  16
  torch correction   x = x + cv (0.5 v + 0.5 v'): counted as 16
  stochastic         stk_flow_step_f32 with eps, in place: read x, v, eps, write x                                    16
  torch stochastic   x = cx x + cv v + cn eps: counted as 16

Part 2: a 50-step Euler run (50 evaluations) and a 25-step Heun run (49 evaluations) of the CIFAR-10 DDPM++ network with random
weights under configs.flow, beside the 18-step EDM run (35 evaluations) of the same network under configs.edm, wall time over
a synchronisation, median of five alternating rounds; and one training step under configs.flow beside the configs.edm step,
the same way.

Writes profiles/flow_eval.txt.  Sample quality is not measured: no checkpoint trained under this formulation exists.

    python tools/flow_eval.py
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
ap.add_argument('--out', default=os.path.join(E.ROOT, 'profiles', 'flow_eval.txt'))
args = ap.parse_args()
assert torch.cuda.is_available(), 'flow_eval.py measures on the GPU: there is nothing to report without one'
device = torch.device('cuda', 0)
EDM_ROW = (0.0357, 0.491, 2.6, -0.7, 0.509)    # (cs, co, t, h, c_next): a step from t^ = 2.6 to 1.9 at sigma_data = 0.5
CV = -0.04                                     # a deterministic step of length 0.04: the row (1, CV, 0)
NOISE_ROW = (0.972, -0.05064, 0.186333)        # (cx, cv, cn): the same step from t = 0.62 at eta = 0.7
PER_ELEM = {'edm euler': 20, 'loss pair': 24, 'torch loss pair': 24, 'euler': 12, 'torch euler': 12, 'correction': 16,
            'torch correction': 16, 'stochastic': 16, 'torch stochastic': 16}


def measure(lib, B, n, lines):
  total = B * n
  per_set = 9 * 4 * total                       # x, v, v', eps / n, F, r, x-out, and the two further outputs of the EDM step
  sets = E.set_count(per_set)
  s = torch.cuda.current_stream().cuda_stream
  p = lambda t: t.data_ptr()
  nbytes = int(lib.flow_ws_bytes(B, n))
  ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
  loss, go = torch.empty(B, device=device), torch.full((B,), 1. / B, device=device)
  cx, cv, cn = NOISE_ROW
  forms = {k: [] for k in PER_ELEM}
  for _ in range(sets):
    x, v, v1, nz, F = (torch.randn(B, n, device=device) * k for k in (1.5, 2.0, 1.0, 1.0, 0.8))
    r, xo, do, xi = (torch.empty(B, n, device=device) for _ in range(4))

    def loss_pair(F=F, y=x, nz=nz, r=r):
      lib.flow_loss_f32(p(F), p(y), p(nz), p(ws), nbytes, p(r), p(loss), B, n, 1, s)
      lib.flow_loss_grad_f32(p(r), p(go), p(r), B, n, 1, s)

    def torch_loss_pair(F=F, y=x, nz=nz):
      Fg = F.detach().requires_grad_(True)
      rr = Fg - (nz - y)
      out = ((rr * rr).double().sum(dim=1) / n).to(torch.float32)
      out.backward(go)
      return Fg.grad

    forms['edm euler'].append(lambda x=x, F=F, xo=xo, do=do, xi=xi: lib.edm_step_f32(p(x), p(x), p(F), None, *EDM_ROW, p(xo), p(do),
                                                                                    p(xi), total, s))
    forms['loss pair'].append(loss_pair)
    forms['torch loss pair'].append(torch_loss_pair)
    forms['euler'].append(lambda x=x, v=v, xo=xo: lib.flow_step_f32(p(x), p(v), None, None, 1., CV, 0., p(xo), total, s))
    forms['torch euler'].append(lambda x=x, v=v: x + CV * v)
    forms['correction'].append(lambda x=x, v=v, v1=v1: lib.flow_step_f32(p(x), p(v1), p(v), None, 1., CV, 0., p(x), total, s))
    forms['torch correction'].append(lambda x=x, v=v, v1=v1: x.add_(0.5 * v + 0.5 * v1, alpha=CV))
    forms['stochastic'].append(lambda x=x, v=v, nz=nz: lib.flow_step_f32(p(x), p(v), None, p(nz), cx, cv, cn, p(x), total, s))
    forms['torch stochastic'].append(lambda x=x, v=v, nz=nz: x.mul_(cx).add_(v, alpha=cv).add_(nz, alpha=cn))
  lines.append(f'  (B, n) = ({B}, {n}), {4 * total / 2 ** 20:.1f} MiB per tensor, {sets} buffer sets in the rotation '
               f'({sets * per_set / 2 ** 20:.0f} MiB):')
  for label, pick in (('one set (cache-resident where it fits)', lambda c: c[:1]), ('rotating sets', lambda c: c)):
    rounds = [{k: E.timed(pick(forms[k]), args.reps) for k in (list(forms) if r % 2 == 0 else reversed(list(forms)))}
              for r in range(args.rounds)]
    med = {k: statistics.median(r[k] for r in rounds) for k in forms}
    lines.append(f'    {label}:')
    for k in forms:
      lines.append(f'      {k:18s} {med[k]:9.1f} us = {PER_ELEM[k] * total / (med[k] * 1e-6) / 1e12:5.2f} TB/s of {PER_ELEM[k]} B per element')
    lines.append('      fused / torch: ' + ', '.join(f'{k} {med[k] / med["torch " + k]:.3f}x'
                                                     for k in ('loss pair', 'euler', 'correction', 'stochastic')))


def network_parts(lines):
  B = args.batch
  base = st.configs.get_config('cifar10_ddpmpp_nll_st')
  base.device = device
  shape = (B, 3, 32, 32)
  inv = lambda v: v
  runs, steps = {}, {}
  for name, cfg in (('edm', st.configs.edm(base)), ('flow', st.configs.flow(base))):
    sde = st.sde_lib.get_sde(cfg, None)
    torch.manual_seed(0)
    model = st.models.utils.create_model(cfg, sde)
    model.eval()
    if name == 'edm':
      samplers = {'edm': st.edm.get_edm_sampler(cfg, sde, shape, inv, steps=18, device=device)}
    else:
      samplers = {'euler': st.flow.get_flow_sampler(cfg, sde, shape, inv, steps=50, order=1, device=device),
                  'heun': st.flow.get_flow_sampler(cfg, sde, shape, inv, steps=25, order=2, device=device)}
    for key, sample in samplers.items():
      runs[key] = (lambda sample=sample, model=model: sample(model))
    opt = st.losses.get_optimizer(cfg, model.parameters())
    ema = st.models.ema.ExponentialMovingAverage(model.parameters(), decay=cfg.model.ema_rate)
    state = dict(optimizer=opt, model=model, ema=ema, step=0)
    step_fn = st.losses.get_step_fn(cfg, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg))
    batch = st.datasets.synthetic_batch(cfg, B, device=device, generator=torch.Generator().manual_seed(4321))
    steps[name] = (lambda step_fn=step_fn, state=state, batch=batch: [step_fn(state, batch) for _ in range(5)])
  ms = E.wall(runs, args.rounds)
  lines.append(f'  whole run on the CIFAR-10 DDPM++ network, batch {B}, random weights:')
  lines.append(f'    EDM Heun, 18 steps (35 evaluations)     {ms["edm"]:8.1f} ms = {ms["edm"] / 35:.2f} ms per evaluation')
  lines.append(f'    flow Euler, 50 steps (50 evaluations)   {ms["euler"]:8.1f} ms = {ms["euler"] / 50:.2f} ms per evaluation')
  lines.append(f'    flow Heun, 25 steps (49 evaluations)    {ms["heun"]:8.1f} ms = {ms["heun"] / 49:.2f} ms per evaluation')
  ms = E.wall(steps, args.rounds)
  lines.append(f'  training step, batch {B} (five steps per figure):')
  lines.append(f'    EDM step (configs.edm)     {ms["edm"] / 5:7.2f} ms = {B / (ms["edm"] / 5) * 1e3:.0f} images/s')
  lines.append(f'    flow step (configs.flow)   {ms["flow"] / 5:7.2f} ms = {B / (ms["flow"] / 5) * 1e3:.0f} images/s')


lines = ['flow_eval.py: the rectified-flow loss pair and step launches on one MI355X.',
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
