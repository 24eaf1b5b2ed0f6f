#!/usr/bin/env python
"""Class conditioning and classifier-free guidance (models.utils.class_condition, include/stk_cond.h) measured on the GPU.

Per network and batch -- DDPM++ 32^2 at batches 16 and 128, NCSN++ 256^2 at batch 4, each with num_classes = 10 and a
random table -- the wall time over a device synchronisation, after warm-up, of
  an unguided evaluation          class_condition(model, y, 0): one pass at batch B
  a guided evaluation             class_condition(model, y, 1.5): one pass at batch 2 B and stk_cfg_combine_f32
  two separate evaluations at B   with y, then with the null class: what guidance costs without the 2 B form
in three rounds, the forms alternating, and the three new launches alone (back-to-back launches between two device events):
the embedding forward and backward on the network's [B, 4 nf] time embedding and the combination on its [B, 3, H, H] output.
Also the device memory the torch allocator holds before and after the guided (2 B) program is first built.

Writes profiles/cond_eval.txt.  Sample quality under guidance is not measured here or anywhere else.

    python tools/cond_eval.py
"""
import argparse
import gc
import os
import time

import torch

import _sampler_eval as E
from _sampler_eval import st

ap = argparse.ArgumentParser()
ap.add_argument('--cases', nargs='*', default=['cifar10:16', 'cifar10:128', 'celebahq256:4'], help='workload:batch')
ap.add_argument('--classes', type=int, default=10)
ap.add_argument('--guidance', type=float, default=1.5)
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--launch-reps', type=int, default=500)
ap.add_argument('--out', default=os.path.join(E.ROOT, 'profiles', 'cond_eval.txt'))
args = ap.parse_args()
assert torch.cuda.is_available(), 'cond_eval.py measures on the GPU: there is nothing to report without one'
device = torch.device('cuda', 0)
mu = st.models.utils


def conditional_model(workload):
  cfg_name, _, desc = E.bench.WORKLOADS[workload]
  cfg = st.configs.get_config(cfg_name)
  cfg.device = device
  cfg.model.num_classes = args.classes
  sde = st.sde_lib.get_sde(cfg, None)
  torch.manual_seed(0)
  model = mu.create_model(cfg, sde)
  model.eval()
  with torch.no_grad():
    model.module.class_emb.weight.normal_(0., 0.1)
  return desc, cfg, sde, model


def wall_ms(call, reps):
  call()
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(reps):
    call()
  torch.cuda.synchronize()
  return 1e3 * (time.perf_counter() - t0) / reps


def launches(lib, B, D, n, C):
  """us of each of the three launches alone."""
  t, y, gy, gt = (torch.randn(B, D, device=device) for _ in range(4))
  table, gtable = torch.randn(C + 1, D, device=device), torch.zeros(C + 1, D, device=device)
  idx = torch.randint(0, C + 1, (B,), device=device).float()
  c, u, out = (torch.randn(n, device=device) for _ in range(3))
  s = torch.cuda.current_stream().cuda_stream
  p = lambda v: v.data_ptr()
  fwd = lambda: lib.class_embed_fwd_f32(p(t), p(table), p(idx), p(y), B, C, D, s)
  bwd = lambda: lib.class_embed_bwd_f32(p(gy), p(idx), p(gt), 1.0, p(gtable), B, C, D, s)
  comb = lambda: lib.cfg_combine_f32(p(c), p(u), args.guidance, p(out), n, s)
  return [E.launches_alone(f, args.launch_reps, 1)[0] for f in (fwd, bwd, comb)]


def case(lines, workload, B, first):
  desc, cfg, sde, model = conditional_model(workload)
  if first:
    lines.append(f'{desc}, num_classes = {args.classes}, guidance weight {args.guidance}: {args.reps} evaluations per figure after a '
                 f'warm-up, three rounds.')
  shape = (B, cfg.data.num_channels, cfg.data.image_size, cfg.data.image_size)
  score_fn = mu.get_score_fn(cfg, sde, model, train=False, continuous=cfg.training.continuous)
  x = sde.prior_sampling(shape).to(device).contiguous()
  t = torch.ones(B, device=device) * 0.5
  y = st.datasets.synthetic_classes(cfg, B, device=device, generator=None)
  null = [None] * B

  def under(classes, w):
    def call():
      with mu.class_condition(model, classes, w):
        return score_fn(x, t)
    return call

  unguided, guided = under(y, 0.0), under(y, args.guidance)
  cond_only, null_only = under(y, 0.0), under(null, 0.0)

  def two():
    cond_only()
    null_only()

  with mu.sampling_run(model):
    unguided()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(device) / 2 ** 20
    guided()
    torch.cuda.synchronize()
    after = torch.cuda.memory_allocated(device) / 2 ** 20
    rounds = [(wall_ms(unguided, args.reps), wall_ms(guided, args.reps), wall_ms(two, args.reps)) for _ in range(3)]
  un, gd, tw = (min(r[j] for r in rounds) for j in range(3))
  D = model.module.class_emb.weight.shape[1]
  us = launches(model.module.engine().lib, B, D, x.numel(), args.classes)
  lines.append(f'  batch {B}: unguided ' + ' / '.join(f'{r[0]:.2f}' for r in rounds) + ' ms; guided (one pass at 2 B) '
               + ' / '.join(f'{r[1]:.2f}' for r in rounds) + ' ms; two evaluations at B ' + ' / '.join(f'{r[2]:.2f}' for r in rounds)
               + f' ms.  Fastest: guided / unguided = {gd / un:.2f}x, guided / two evaluations = {gd / tw:.2f}x.  Launches alone: '
               f'embedding forward [{B}, {D}] {us[0]:.1f} us, backward {us[1]:.1f} us, combination of {x.numel()} elements '
               f'{us[2]:.1f} us.  Allocated device memory: {before:.0f} MiB with the program of batch {B}, {after:.0f} MiB once that '
               f'of batch {2 * B} exists too (+{after - before:.0f} MiB).')


lines = ['cond_eval.py: class-conditional evaluation and classifier-free guidance on one MI355X.']
last = None
for spec in args.cases:
  workload, B = spec.split(':')
  case(lines, workload, int(B), workload != last)
  last = workload
  gc.collect()                 # the model and its engine refer to each other: free the arenas before the next case
  torch.cuda.empty_cache()
lines.append('Sample quality under guidance is unmeasured: no trained class-conditional checkpoint exists.')
E.write(lines, args.out)
