#!/usr/bin/env python
"""The plane-operand 3x3 weight gradient alone: stk_conv2d_wgrad_pl_wgs_f32 against its one-product twin
stk_conv2d_wgrad_pl_wgs_f16x1 (include/stk_fp16_train.h), kernel + slab reduction, on the layer shapes of the benched nets,
alternating the two in one process: `--repeats` rounds of `--launches` launches each, HIP events around every round.

    python tools/fp16_wgrad_alone.py --repeats 5 --launches 20
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import soft_truncation_amd as st

SHAPES = [   # N, Cin, Cout, H: DDPM++ CIFAR-10 (batch 128) and UNCSN++ CelebA-64 (batch 128) levels
  (128, 128, 128, 32), (128, 256, 256, 16), (128, 256, 256, 8), (128, 256, 256, 4), (128, 128, 128, 64),
]
ap = argparse.ArgumentParser()
ap.add_argument('--repeats', type=int, default=5)
ap.add_argument('--launches', type=int, default=20)
args = ap.parse_args()
lib = st.engine.lib.load()
assert lib.has_fp16_train
dev = torch.device('cuda', 0)


def planes(t):
  rec = torch.zeros(256, device=dev)
  lib.amax_partial_f32(t.data_ptr(), t.numel(), rec.data_ptr(), torch.cuda.current_stream().cuda_stream)
  N, C, H, W = t.shape
  pl = torch.zeros(int(lib.planes_bytes(N, C, H * W)), dtype=torch.uint8, device=dev)
  lib.split_planes_f32(t.data_ptr(), N, C, H * W, rec.data_ptr(), 256, pl.data_ptr(), torch.cuda.current_stream().cuda_stream)
  return pl, rec


print(f'{"N, Cin -> Cout, map":<26} {"wgs":>4} {"fp32 us":>9} {"fp16 us":>9} {"ratio":>6}   (median of {args.repeats} rounds; min-max)')
for N, Cin, Cout, H in SHAPES:
  x = torch.randn(N, Cin, H, H, device=dev)
  dy = torch.randn(N, Cout, H, H, device=dev)
  (xp, rx), (yp, ry) = planes(x), planes(dy)
  nb = int(lib.conv2d_wgrad_pl_ws_bytes(N, H, H, Cin, Cout))
  ws = torch.empty(nb // 4 + 64, device=dev)
  dw = torch.zeros(Cout, Cin, 3, 3, device=dev)
  s = torch.cuda.current_stream().cuda_stream
  for wgs in (256, 512):
    fns = {'fp32': lib.conv2d_wgrad_pl_wgs_f32, 'fp16': lib.conv2d_wgrad_pl_wgs_f16x1}
    a = (xp.data_ptr(), rx.data_ptr(), yp.data_ptr(), ry.data_ptr(), dw.data_ptr(), 1.0, ws.data_ptr(), nb, N, H, H, Cin, Cout,
         wgs, s)
    for fn in fns.values():
      for _ in range(3):
        fn(*a)
    us = {k: [] for k in fns}
    for r in range(args.repeats):
      for k, fn in fns.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.launches):
          fn(*a)
        e1.record()
        e1.synchronize()
        us[k].append(1e3 * e0.elapsed_time(e1) / args.launches)
    m32, m16 = np.median(us['fp32']), np.median(us['fp16'])
    print(f'{N}, {Cin} -> {Cout}, {H}x{H}'.ljust(26) + f' {wgs:4d} {m32:9.1f} {m16:9.1f} {m32 / m16:6.2f}   '
          f'({min(us["fp32"]):.1f}-{max(us["fp32"]):.1f} / {min(us["fp16"]):.1f}-{max(us["fp16"]):.1f})', flush=True)
