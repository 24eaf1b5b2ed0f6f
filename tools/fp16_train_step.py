#!/usr/bin/env python
"""fp32 and fp16 training steps (config.training.precision) of bench.py workloads, timed alternately in ONE process on one
device: the same model, optimizer and EMA, the same batches, `--repeats` rounds of `--steps` fp32 steps then `--steps` fp16
steps, each round timed between two device synchronisations.  Prints ms/step and images/s per round and the spread.

    python tools/fp16_train_step.py --workload cifar10 celeba64 celebahq256 --repeats 5 --steps 10
"""
import argparse
import copy
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
import soft_truncation_amd as st

ap = argparse.ArgumentParser()
ap.add_argument('--workload', nargs='+', default=['cifar10'], choices=sorted(bench.WORKLOADS))
ap.add_argument('--batch', type=int, default=0, help='per-step batch (0 = the workload\'s)')
ap.add_argument('--steps', type=int, default=10)
ap.add_argument('--warmup', type=int, default=3)
ap.add_argument('--repeats', type=int, default=5)
args = ap.parse_args()

dev = torch.device('cuda', 0)
for name in args.workload:
  cfg_name, batch, desc = bench.WORKLOADS[name]
  B = args.batch or batch
  cfg = st.configs.get_config(cfg_name)
  cfg.device = dev
  torch.manual_seed(0)
  sde = st.sde_lib.get_sde(cfg, None)
  state, step32 = bench.build_training(st, cfg, sde)
  cfg16 = copy.deepcopy(cfg)
  cfg16.training.precision = 'fp16'
  step16 = st.losses.get_step_fn(cfg16, sde, train=True, optimize_fn=st.losses.optimization_manager(cfg16))
  batches = [st.datasets.synthetic_batch(cfg, B, generator=torch.Generator().manual_seed(i)).to(dev) for i in range(4)]
  fns = {'fp32': step32, 'fp16': step16}
  for p, fn in fns.items():
    for i in range(args.warmup):
      fn(state, batches[i % 4])
  torch.cuda.synchronize()
  ms = {'fp32': [], 'fp16': []}
  for r in range(args.repeats):
    for p, fn in fns.items():
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for i in range(args.steps):
        fn(state, batches[i % 4])
      torch.cuda.synchronize()
      ms[p].append(1e3 * (time.perf_counter() - t0) / args.steps)
  print(f'{name} ({desc}), batch {B}, {args.repeats} rounds of {args.steps} steps per precision, alternating:')
  for p in ('fp32', 'fp16'):
    a = np.array(ms[p])
    print(f'  {p}: ms/step median {np.median(a):.2f} (min {a.min():.2f}, max {a.max():.2f}), images/s {B * 1e3 / np.median(a):.1f}'
          f'   rounds: ' + ' '.join(f'{v:.2f}' for v in a))
  ratio = np.median(ms['fp32']) / np.median(ms['fp16'])
  print(f'  fp32 / fp16 step time: {ratio:.3f}', flush=True)
  del state, step32, step16, fns
  torch.cuda.empty_cache()
