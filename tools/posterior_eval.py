#!/usr/bin/env python
"""The posterior sampler (posterior_sampling.py, include/stk_posterior.h) measured on the GPU.

1. The four launches of a guided step -- stk_tweedie_f32, stk_residual_f32, stk_guide_seed_f32, stk_guide_update_f32 -- timed
   together on a [batch,3,size,size] state with a measurement of [batch,3,size/4,size/4], against the same work composed from
   torch operations on the same box, and against their byte count: tweedie 3 state-sized tensors, seed 3, update 6 (x_mean
   written), residual 3 measurement-sized ones.  The buffers of one step stay in the 256 MiB last-level cache between launches,
   so every figure is taken twice: on one set of buffers (resident) and rotating over enough sets to exceed the cache.
2. One guided predictor step (dps_update: one forward, one input-only backward, the operator and its adjoint, the four
   launches, the predictor) against one unguided predictor-corrector iteration (two forwards) on the benchmark networks at
   256^2 and at 32^2: wall time over a synchronisation, alternating, three rounds, all printed.
3. Peak device memory per batch size (the forward of a guided step keeps its activations for the backward): a fresh process
   per (network, batch) runs two unguided iterations, reads the allocator's peak, then runs two guided iterations and reads
   it again -- what a sampling run holds, since the corrector's forward-only program and the guided program live side by side.

Writes profiles/posterior_eval.txt.  Sample quality is not measured here or anywhere else.

    python tools/posterior_eval.py
"""
import argparse
import os
import subprocess
import sys
import time

import torch

import _sampler_eval as E
from _sampler_eval import st

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=16)
ap.add_argument('--size', type=int, default=256)
ap.add_argument('--reps', type=int, default=500)
ap.add_argument('--step-reps', type=int, default=5)
ap.add_argument('--batches256', type=int, nargs='*', default=[1, 4])
ap.add_argument('--batches32', type=int, nargs='*', default=[16, 128])
ap.add_argument('--child', nargs=2, metavar=('WORKLOAD', 'BATCH'), help='internal: print the peak memory of one case')
ap.add_argument('--out', default=os.path.join(E.ROOT, 'profiles', 'posterior_eval.txt'))
args = ap.parse_args()
assert torch.cuda.is_available(), 'posterior_eval.py measures on the GPU: there is nothing to report without one'
device = torch.device('cuda', 0)
ps, S = st.posterior_sampling, st.sampling
lib = ps._library()
CACHE = 256 << 20
LO, HI, ZETA = -1., 1., 0.5
wide = lambda v: v[:, None, None, None]


# ---- 1. the four launches ------------------------------------------------------------------------------------------------
def launch_buffers(B, C, H):
  state = lambda: torch.randn(B, C, H, H, device=device)
  meas = lambda: torch.randn(B, C, H // 4, H // 4, device=device)
  k = C * (H // 4) ** 2
  ws_bytes = lib.posterior_ws_bytes(B, k)
  return dict(x=state(), score=state(), v=state(), gnet=state(), xp=state(), xpm=state(), x0=state(), seed=state(), out=state(),
              mean=state(), y=meas(), m=meas(), r=meas(), rnorm=torch.empty(B, device=device),
              ws=torch.empty(ws_bytes // 8, dtype=torch.float64, device=device), ws_bytes=ws_bytes, k=k)


def four_launches(b, a, s):
  B, n = b['x'].shape[0], b['x'][0].numel()
  stream = torch.cuda.current_stream().cuda_stream
  p = lambda name: b[name].data_ptr()
  lib.tweedie_f32(p('x'), p('score'), a.data_ptr(), s.data_ptr(), LO, HI, p('x0'), B, n, stream)
  lib.residual_f32(p('y'), p('m'), p('r'), p('ws'), b['ws_bytes'], B, b['k'], stream)
  lib.guide_seed_f32(p('v'), p('x0'), a.data_ptr(), s.data_ptr(), LO, HI, p('ws'), b['ws_bytes'], b['k'], p('seed'), p('rnorm'),
                     B, n, stream)
  lib.guide_update_f32(p('xp'), p('xpm'), p('v'), p('gnet'), p('x0'), a.data_ptr(), p('rnorm'), ZETA, LO, HI, p('out'), p('mean'),
                       B, n, stream)


def composed(b, a, s):
  """The four launches as torch operations -> (x0, r, rnorm, seed, x, x_mean)."""
  x0 = ((b['x'] + wide(s * s) * b['score']) / wide(a)).clamp(LO, HI)
  r = b['y'] - b['m']
  rnorm = (r * r).reshape(r.shape[0], -1).sum(dim=1, dtype=torch.float64).sqrt().float()
  inside = (x0 > LO) & (x0 < HI)
  seed = torch.where(inside, wide(s * s / a) * b['v'], 0.)
  g = torch.where(inside, b['v'] / wide(a) + b['gnet'], b['gnet'])
  step = wide(torch.where(rnorm > 0, ZETA / rnorm, 0.)) * g
  return x0, r, rnorm, seed, b['xp'] + step, b['xpm'] + step


def launches_section(lines):
  B, C, H = args.batch, 3, args.size
  state_bytes, meas_bytes = 4 * B * C * H * H, 4 * B * C * (H // 4) ** 2
  moved = 12 * state_bytes + 3 * meas_bytes
  a = torch.rand(B, device=device) * 0.7 + 0.3
  s = torch.rand(B, device=device) + 0.05
  n_sets = CACHE // (14 * state_bytes) + 2
  sets = [launch_buffers(B, C, H) for _ in range(n_sets)]
  four_launches(sets[0], a, s)
  want = composed(sets[0], a, s)
  for name, w in zip(('x0', 'r', 'rnorm', 'seed', 'out', 'mean'), want):
    assert float((sets[0][name] - w).abs().max()) <= 1e-4 * float(w.abs().max()), name     # the float64 check is the tests'
  kernel, torch_form = (lambda b: four_launches(b, a, s)), (lambda b: composed(b, a, s))
  rounds = []
  for _ in range(3):
    rounds.append((E.launches_alone(lambda: kernel(sets[0]), args.reps, moved),
                   E.launches_alone(lambda: torch_form(sets[0]), args.reps, moved),
                   E.launches_alone(E.rotating(kernel, sets), args.reps, moved),
                   E.launches_alone(E.rotating(torch_form, sets), args.reps, moved)))
  lines.append(f'1. The four launches of include/stk_posterior.h on a [{B},{C},{H},{H}] fp32 state with a [{B},{C},{H // 4},{H // 4}] '
               f'measurement, clamp [-1, 1], x_mean written: {moved / 1e6:.1f} MB per step by their byte count (12 state-sized and 3 '
               f'measurement-sized tensors).  {args.reps} back-to-back steps between two device events after 10 warm-ups; three '
               f'rounds, kernels and torch composition alternating.  "resident": one set of buffers; "rotating": {n_sets} sets, '
               f'more than the 256 MiB last-level cache.')
  for j, name in enumerate(('kernels, resident', 'torch,   resident', 'kernels, rotating', 'torch,   rotating')):
    best = min(rd[j][0] for rd in rounds)
    lines.append(f'  {name}: ' + ' / '.join(f'{rd[j][0]:.1f}' for rd in rounds) + f' us per step; fastest {best:.1f} us = '
                 f'{moved / (best * 1e-6) / 1e12:.2f} TB/s of the byte count')
  k_res, t_res, k_rot, t_rot = (min(rd[j][0] for rd in rounds) for j in range(4))
  lines.append(f'  torch composition / kernels: {t_res / k_res:.1f}x resident, {t_rot / k_rot:.1f}x rotating')


# ---- 2. and 3. a guided step against an unguided iteration, and peak memory ---------------------------------------------------
def wall_ms(call, reps):
  call()
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(reps):
    call()
  torch.cuda.synchronize()
  return 1e3 * (time.perf_counter() - t0) / reps


def case(workload, B):
  """(desc, model, guided predictor step, unguided PC iteration, guided PC iteration) of one network at batch B; the calls
  run inside sampling_run."""
  wl = argparse.Namespace(workload=workload, batch=B)
  _, desc, cfg, _, sde, model, shp = E.workload(wl)
  cont = cfg.training.continuous
  predictor, corrector = S.get_predictor('reverse_diffusion'), S.get_corrector('langevin')
  predict, correct = S.pc_updates(cfg, sde, predictor, corrector, cfg.sampling.snr, 1, False, cont)
  operator = ps.BlockAveraging(4)
  x = sde.prior_sampling(shp).to(device).contiguous()
  vec_t = torch.ones(B, device=device) * 0.5
  with torch.no_grad():
    y = operator(torch.rand(shp, device=device))
  score_fn = st.models.utils.get_score_fn(cfg, sde, model, train=False, continuous=cont)

  def guided():
    return ps.dps_update(cfg, sde, score_fn, predictor, operator, y, x, vec_t, ZETA)

  def unguided():
    xc, _ = correct(x, vec_t, model=model)
    return predict(xc, vec_t, model=model)

  def guided_iteration():
    xc, _ = correct(x, vec_t, model=model)
    return ps.dps_update(cfg, sde, score_fn, predictor, operator, y, xc, vec_t, ZETA)

  return desc, model, guided, unguided, guided_iteration


def peak_mb(call):
  for _ in range(2):
    call()
  torch.cuda.synchronize()
  return torch.cuda.max_memory_allocated(device) / 2 ** 20


def child(workload, B):
  _, model, _, unguided, guided_iteration = case(workload, B)
  with st.models.utils.sampling_run(model):
    print(f'PEAK {peak_mb(unguided):.0f} {peak_mb(guided_iteration):.0f}', flush=True)


def peaks_of(workload, B):
  out = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', workload, str(B)], check=True, capture_output=True,
                       text=True, timeout=300).stdout
  return [int(v) for v in [line for line in out.splitlines() if line.startswith('PEAK ')][-1].split()[1:]]


def step_section(lines, workload, batches):
  for i, B in enumerate(batches):
    desc, model, guided, unguided, guided_iteration = case(workload, B)
    if i == 0:
      lines.append(f'{desc}; operator: 4 x 4 block averages; reverse diffusion + Langevin; {args.step_reps} steps per figure after '
                   f'a warm-up, wall time over a synchronisation, three rounds, the forms alternating.  Weights: '
                   f'{model_mb(model):.0f} MiB.')
    with st.models.utils.sampling_run(model):
      rounds = [(wall_ms(guided, args.step_reps), wall_ms(unguided, args.step_reps), wall_ms(guided_iteration, args.step_reps))
                for _ in range(3)]
    g, u, gi = (min(r[j] for r in rounds) for j in range(3))
    del model, guided, unguided, guided_iteration
    torch.cuda.empty_cache()
    mem = peaks_of(workload, B)
    lines.append(f'  batch {B}: guided predictor step ' + ' / '.join(f'{r[0]:.1f}' for r in rounds) + ' ms; unguided PC iteration '
                 + ' / '.join(f'{r[1]:.1f}' for r in rounds) + ' ms; guided PC iteration ' + ' / '.join(f'{r[2]:.1f}' for r in rounds)
                 + f' ms.  Fastest: guided iteration / unguided iteration = {gi / u:.2f}x, guided step alone {g:.1f} ms.  Peak '
                 f'device memory of a fresh process: {mem[0]} MiB after unguided iterations, {mem[1]} MiB after guided ones.')


def model_mb(model):
  return sum(p.numel() * p.element_size() for p in model.parameters()) / 2 ** 20


if args.child:
  child(args.child[0], int(args.child[1]))
  sys.exit(0)

lines = ['posterior_eval.py: the posterior sampler on one MI355X.']
launches_section(lines)
torch.cuda.empty_cache()
lines.append('2. and 3. One guided predictor step (dps_update) and one guided PC iteration (unguided corrector + guided predictor: two '
             'forwards and one input-only backward) against one unguided PC iteration (two forwards), and the peak device memory '
             '(the torch allocator\'s, which holds the engine\'s arenas too).')
step_section(lines, 'celebahq256', args.batches256)
step_section(lines, 'cifar10', args.batches32)
lines.append('Sample quality of the posterior sampler is unmeasured.')
E.write(lines, args.out)
