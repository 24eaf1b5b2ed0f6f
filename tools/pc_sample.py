#!/usr/bin/env python
"""One complete predictor-corrector sampler run (sampling.get_sampling_fn, the config's own N, predictor, corrector and
final denoising step) of a bench.py workload on random live weights: wall seconds, NFE, and the uint8 samples saved for a
comparison between precisions.  The same --seed gives the same weights and the same noise in either precision, so the
distance between the two runs' samples measures what the fp16 mode changes along one trajectory (a distance, not a
sample-quality figure).

    python tools/pc_sample.py --workload celebahq256 --batch 16 --precision fp32 --out pc_fp32.npz
    python tools/pc_sample.py --workload celebahq256 --batch 16 --precision fp16 --out pc_fp16.npz \\
        --compare pc_fp32.npz
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np
import torch

import bench
import soft_truncation_amd as st
from _fullsize_cases import live_init_

ap = argparse.ArgumentParser()
ap.add_argument('--workload', default='celebahq256', choices=sorted(bench.WORKLOADS))
ap.add_argument('--batch', type=int, default=16)
ap.add_argument('--precision', default='fp32', choices=('fp32', 'fp16'))
ap.add_argument('--seed', type=int, default=0)
ap.add_argument('--N', type=int, default=0, help='shorter grid (0 = the config\'s N)')
ap.add_argument('--out', default='')
ap.add_argument('--compare', default='', help='npz of another run: max / mean |delta| of the uint8 samples')
args = ap.parse_args()
cfg_name, _, desc = bench.WORKLOADS[args.workload]
cfg = st.configs.get_config(cfg_name)
cfg.device = torch.device('cuda', 0)
cfg.sampling.method = 'pc'
cfg.sampling.precision = args.precision
sde = st.sde_lib.get_sde(cfg, None)
if args.N:
  sde.N = args.N
torch.manual_seed(args.seed)
net = st.models.ncsnpp.NCSNpp(cfg, sde)
live_init_(net, args.seed)
net = net.to(cfg.device)
model = st.models.utils.DataParallel(net)
model.eval()
S = cfg.data.image_size
shape = (args.batch, cfg.data.num_channels, S, S)
fn = st.sampling.get_sampling_fn(cfg, sde, shape, st.datasets.get_data_inverse_scaler(cfg), 1e-3)
torch.manual_seed(args.seed + 1)
torch.cuda.synchronize()
t0 = time.perf_counter()
x, nfe = fn(model)
torch.cuda.synchronize()
sec = time.perf_counter() - t0
u8 = (x.clamp(0, 1) * 255.).round().to(torch.uint8).cpu().numpy()
print(f'{desc} [{args.precision}]: PC sampler N = {sde.N}, batch {args.batch}, nfe {nfe}: {sec:.1f} s '
      f'({1e3 * sec / nfe:.2f} ms per evaluation incl. the update arithmetic); finite {bool(torch.isfinite(x).all())}')
if args.out:
  np.savez_compressed(args.out, u8=u8, sec=sec, nfe=nfe)
if args.compare:
  o = np.load(args.compare)['u8'].astype(np.int32)
  d = np.abs(u8.astype(np.int32) - o)
  print(f'uint8 distance to {os.path.basename(args.compare)} (same seed; a distance, NOT a quality figure): '
        f'max {d.max()}, mean {d.mean():.3f}, fraction of values differing {float((d > 0).mean()):.4f}')
