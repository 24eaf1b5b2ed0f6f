#!/usr/bin/env python
"""Scale-shift GroupNorm conditioning (config.model.scale_shift_norm, include/stk_adagn.h) measured on the GPU.

1. The modulated forward / backward (stk_gn_mod_fwd_f32 / stk_gn_mod_bwd_f32, SiLU, no dropout, 32 groups) against the
   plain stk_gn_fwd_f32 / stk_gn_bwd_f32 on the same tensors, at (N, C, HW) = (128, 128, 1024), (128, 256, 256) and
   (4, 128, 65536): back-to-back launches between two device events, on ONE set of buffers (resident in the 256 MB
   Infinity Cache where it fits) and on a rotation of sets that together exceed 1 GiB (every launch from HBM).  Five rounds,
   the four forms alternating inside each round, their order reversed in every second round; the figure is the median of
   the five.  TB/s are those of the algorithmic byte count: read x, write y (forward); read x, read dy, write dx
   (backward); + the 2 N C floats of `mod`.
2. A training step (losses.get_step_fn) and a sampling evaluation (score_fn under sampling_run) of the CIFAR-10 DDPM++
   network at batch 128, without the switch and with it: wall time over a device synchronisation, five alternating rounds,
   the median.  The switch forgoes the one-pass GroupNorm -> planes writer on GroupNorm_1 and the by-products that the
   GroupNorm_1 backward leaves for Conv_0; this is what that costs.

Writes profiles/adagn_eval.txt.  Sample quality with the switch is not measured: no checkpoint exists.

    python tools/adagn_eval.py
"""
import argparse
import gc
import os
import statistics
import time

import torch

import _sampler_eval as E
from _sampler_eval import st

ap = argparse.ArgumentParser()
ap.add_argument('--shapes', nargs='*', default=['128,128,1024', '128,256,256', '4,128,65536'], help='N,C,HW')
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--steps', type=int, default=10)
ap.add_argument('--batch', type=int, default=128)
ap.add_argument('--skip-network', action='store_true')
ap.add_argument('--out', default=os.path.join(E.ROOT, 'profiles', 'adagn_eval.txt'))
args = ap.parse_args()
assert torch.cuda.is_available(), 'adagn_eval.py measures on the GPU: there is nothing to report without one'
device = torch.device('cuda', 0)
G, EPS, ACT = 32, 1e-6, 1


def kernels(lib, N, C, HW, lines):
  n = N * C * HW
  sets = E.set_count(16 * n, most=None)           # x, y, dy, dx of 4 n bytes each per set
  s = torch.cuda.current_stream().cuda_stream
  p = lambda t: t.data_ptr()
  gamma, beta = 1 + 0.2 * torch.randn(C, device=device), 0.3 * torch.randn(C, device=device)
  mod, dmod = torch.randn(N, 2 * C, device=device), torch.empty(N, 2 * C, device=device)
  dgamma, dbeta = torch.zeros(C, device=device), torch.zeros(C, device=device)
  mean, rstd = torch.empty(N * G, device=device), torch.empty(N * G, device=device)
  ws = torch.empty(max(int(lib.gn_mod_ws_bytes(N, C, HW, G)) // 4, 1), device=device)
  forms = {k: [] for k in ('plain fwd', 'mod fwd', 'plain bwd', 'mod bwd')}
  for _ in range(sets):
    x, dy = torch.randn(N, C, HW, device=device), torch.randn(N, C, HW, device=device)
    y, dx = torch.empty_like(x), torch.empty_like(x)
    forms['plain fwd'].append(lambda x=x, y=y: lib.gn_fwd_f32(p(x), C, None, 0, p(gamma), p(beta), p(y), p(mean), p(rstd), N, HW, G, EPS,
                                                                ACT, 0.0, 0, None, p(ws), s))
    forms['mod fwd'].append(lambda x=x, y=y: lib.gn_mod_fwd_f32(p(x), p(gamma), p(beta), p(mod), 2 * C, p(y), p(mean), p(rstd), N, C, HW, G,
                                                                  EPS, ACT, 0.0, 0, None, p(ws), s))
    forms['plain bwd'].append(lambda x=x, dy=dy, dx=dx: lib.gn_bwd_f32(p(dy), p(x), C, None, 0, p(gamma), p(beta), p(mean), p(rstd), p(dx),
                                                                         0.0, None, 0.0, p(dgamma), p(dbeta), p(ws), N, HW, G, ACT, 0.0, 0,
                                                                         None, s))
    forms['mod bwd'].append(lambda x=x, dy=dy, dx=dx: lib.gn_mod_bwd_f32(p(dy), p(x), p(gamma), p(beta), p(mod), 2 * C, p(mean), p(rstd),
                                                                           p(dx), 0.0, p(dmod), p(dgamma), p(dbeta), p(ws), N, C, HW, G, ACT,
                                                                           0.0, 0, None, s))
  # One (mean, rstd) pair serves every set: each forward overwrites it and each backward reads whatever the last forward left,
  # i.e. the statistics of ANOTHER set's x.  The sets are draws of one distribution, so the values are finite and of the right
  # size and the time of a backward does not depend on them; its dx is not a gradient of anything and is never looked at.
  forms['plain fwd'][0]()
  nbytes = {'plain fwd': 8 * n, 'mod fwd': 8 * n + 8 * N * C, 'plain bwd': 12 * n, 'mod bwd': 12 * n + 8 * N * C}
  lines.append(f'  (N, C, HW) = ({N}, {C}, {HW}), {4 * n / 2 ** 20:.0f} MiB per tensor, {sets} buffer sets in the rotation:')
  for label, pick in (('one set (cache-resident where it fits)', lambda c: c[:1]), ('rotating sets (from HBM)', lambda c: c)):
    # the four forms in one order in the even rounds and in the reverse order in the odd ones: no form always runs behind the same one
    rounds = [{k: E.timed(pick(forms[k]), args.reps, warm=None) for k in (list(forms) if r % 2 == 0 else reversed(list(forms)))}
              for r in range(args.rounds)]
    med = {k: statistics.median(r[k] for r in rounds) for k in forms}
    lines.append(f'    {label}: ' + '; '.join(f'{k} {med[k]:.1f} us = {nbytes[k] / (med[k] * 1e-6) / 1e12:.2f} TB/s' for k in forms)
                 + f'.  mod / plain: forward {med["mod fwd"] / med["plain fwd"]:.3f}x, backward {med["mod bwd"] / med["plain bwd"]:.3f}x'
                 + f' (rounds of the forward ratio: ' + ' '.join(f'{r["mod fwd"] / r["plain fwd"]:.3f}' for r in rounds) + ').')


def network(lines):
  cfg_name, _, desc = E.bench.WORKLOADS['cifar10']
  B = args.batch
  built = {}
  for switch in (False, True):
    cfg = st.configs.get_config(cfg_name)
    cfg.device = device
    if switch:
      cfg.model.scale_shift_norm = True
    sde = st.sde_lib.get_sde(cfg, None)
    torch.manual_seed(0)
    state, step_fn = E.bench.build_training(st, cfg, sde)
    batch = st.datasets.synthetic_batch(cfg, B, device=device, generator=torch.Generator().manual_seed(1234))
    model = state['model']
    score_fn = st.models.utils.get_score_fn(cfg, sde, model, train=False, continuous=cfg.training.continuous)
    x = sde.prior_sampling((B, cfg.data.num_channels, cfg.data.image_size, cfg.data.image_size)).to(device).contiguous()
    t = torch.ones(B, device=device) * 0.5
    built[switch] = (state, step_fn, batch, model, score_fn, x, t, sum(p.numel() for p in model.parameters()))

  def train_ms(switch):
    state, step_fn, batch = built[switch][:3]
    state['model'].train()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
      step_fn(state, batch)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / args.steps

  def eval_ms(switch):
    model, score_fn, x, t = built[switch][3:7]
    model.eval()
    with st.models.utils.sampling_run(model):
      score_fn(x, t)
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for _ in range(args.steps):
        score_fn(x, t)
      torch.cuda.synchronize()
      return 1e3 * (time.perf_counter() - t0) / args.steps

  for switch in (False, True):                       # warm-up: programs, captured graphs, optimizer state
    for _ in range(6):
      built[switch][1](built[switch][0], built[switch][2])
    eval_ms(switch)
  rounds = []
  for r in range(args.rounds):                       # without / with in the even rounds, with / without in the odd ones
    a, b = (False, True) if r % 2 == 0 else (True, False)
    t, e = {a: train_ms(a)}, {}
    t[b] = train_ms(b)
    e[a] = eval_ms(a)
    e[b] = eval_ms(b)
    rounds.append([t[False], t[True], e[False], e[True]])
  med = [statistics.median(r[j] for r in rounds) for j in range(4)]
  lines.append(f'{desc}, batch {B}: {args.steps} calls per figure, {args.rounds} alternating rounds, medians.')
  lines.append(f'  parameters: {built[False][7]} without the switch, {built[True][7]} with it (every Dense_0 twice as wide).')
  lines.append(f'  training step: {med[0]:.2f} ms without, {med[1]:.2f} ms with the switch = {med[1] / med[0]:.3f}x (rounds: '
               + ' '.join(f'{r[1] / r[0]:.3f}' for r in rounds) + ').')
  lines.append(f'  sampling evaluation: {med[2]:.2f} ms without, {med[3]:.2f} ms with the switch = {med[3] / med[2]:.3f}x (rounds: '
               + ' '.join(f'{r[3] / r[2]:.3f}' for r in rounds) + ').')


lines = ['adagn_eval.py: scale-shift GroupNorm conditioning on one MI355X.',
         f'1. stk_gn_mod_fwd_f32 / stk_gn_mod_bwd_f32 against stk_gn_fwd_f32 / stk_gn_bwd_f32 (SiLU, {G} groups, no dropout): '
         f'{args.reps} launches per figure, {args.rounds} alternating rounds, medians.']
lib = st.engine.lib.load()
for spec in args.shapes:
  N, C, HW = (int(v) for v in spec.split(','))
  kernels(lib, N, C, HW, lines)
  gc.collect()
  torch.cuda.empty_cache()
if not args.skip_network:
  lines.append('2. The network with and without config.model.scale_shift_norm.')
  network(lines)
lines.append('Sample quality with the switch is unmeasured: no trained checkpoint exists.')
E.write(lines, args.out)
