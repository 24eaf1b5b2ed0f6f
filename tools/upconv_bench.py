#!/usr/bin/env python
"""Times the FIR-upsampling convolution (include/stk_upconv.h) against the only way include/stk.h alone can produce the same
values: the zero-stuffed tensor, stk_conv2d_fwd_f32 at pad K-1 with its gradients, and stk_upfirdn2d_f32 at 1:1.

    python tools/upconv_bench.py [--reps 21] [--out profiles/upconv_bench.txt]

Per shape and direction: HIP events around one call on the launch stream, three warm-up calls, the median of `reps` (>= 20)
repetitions; achieved TFLOP/s = 2 N H W Cin Cout K^2 (one product per tap and input pixel: the algorithm's count, FIR
excluded) over the whole call's time, against 157.3 TFLOP/s of the f32-input MFMA.  What each row brackets:
  fwd     new: the four parity GEMMs + the FIR.           composition: stuffing + convolution + FIR
  dgrad   new: the FIR adjoint + the stride-2 gather.     composition: FIR adjoint + data gradient + the stride-2 pick of dz
  wgrad   both from a du / z already made (a backward makes them once): the per-tap GEMMs + the slab sum
Both sides are checked against each other before they are timed.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
  if p not in sys.path:
    sys.path.insert(0, p)

import numpy as np
import torch

import soft_truncation_amd as st
from _util import call

PEAK = 157.3
SHAPES = [(64, 64, 16), (128, 128, 32), (256, 256, 64)]      # Cin, Cout, H
BATCHES = [16, 128]
K = 3
FIR = (1, 3, 3, 1)


def median_us(fn, reps):
  for _ in range(3):
    fn()
  torch.cuda.synchronize()
  times = []
  for _ in range(reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    times.append(s.elapsed_time(e) * 1e3)
  return statistics.median(times)


def ws_for(nbytes, dev):
  return torch.empty(max(int(nbytes) // 4, 64), dtype=torch.float32, device=dev), int(nbytes)


def rel(a, b):
  return ((a - b).abs().max() / b.abs().max()).item()


def bench_shape(lib, N, Cin, Cout, H, reps, dev):
  W = H
  taps = np.outer(FIR, FIR).astype(np.float32)
  taps = taps / taps.sum() * 4
  KT = taps.shape[0]
  p = (KT - 2) - (K - 1)
  pad0, pad1 = (p + 1) // 2 + 1, p // 2 + 1
  kf = torch.tensor(taps, device=dev)
  kflip = torch.tensor(taps[::-1, ::-1].copy(), device=dev)
  x = torch.randn(N, Cin, H, W, device=dev)
  w = torch.randn(Cout, Cin, K, K, device=dev) * 0.05
  dout = torch.randn(N, Cout, 2 * H, 2 * W, device=dev)
  U, Z = 2 * H - 2 + K, 2 * H - 1
  dims = (N, H, W, Cin, Cout, K, KT)
  out = {}

  # ---- the new entries
  y = torch.empty(N, Cout, 2 * H, 2 * W, device=dev)
  du = torch.empty(N, Cout, U, U, device=dev)
  dx = torch.empty_like(x)
  dw = torch.zeros_like(w)
  ws0, nb0 = ws_for(lib.upconv2d_ws_bytes(0, *dims), dev)
  ws2, nb2 = ws_for(lib.upconv2d_ws_bytes(2, *dims), dev)
  new = {
    'fwd': lambda: call(lib, 'upconv2d_fwd_f32', x, w, kf, None, None, 1.0, y, *dims, pad0, ws0, nb0),
    'dgrad': lambda: call(lib, 'upconv2d_dgrad_f32', dout, w, kf, du, 0, dx, 0.0, 1.0, *dims, pad0),
    'wgrad': lambda: call(lib, 'upconv2d_wgrad_f32', x, None, None, du, 1, dw, 1.0, *dims, pad0, ws2, nb2),
  }

  # ---- the composition on include/stk.h
  z = torch.zeros(N, Cin, Z, Z, device=dev)
  u = torch.empty(N, Cout, U, U, device=dev)
  yc = torch.empty_like(y)
  duc = torch.empty_like(du)
  dz = torch.empty_like(z)
  dxc = torch.empty_like(x)
  dwc = torch.zeros_like(w)
  cd = (N, Z, Z, Cout, U, U, K, K, 1, K - 1)
  shape = (Cin, 0, N, Z, Z, Cout, K, K, 1, K - 1)
  wsf, nbf = ws_for(max(lib.conv2d_fwd_ws_bytes(*shape), 256), dev)
  wsd, nbd = ws_for(max(lib.conv2d_dgrad_ws_bytes(*shape), 256), dev)
  wsw, nbw = ws_for(max(lib.conv2d_wgrad_ws_bytes(Cin, 0, N, Cout, U, U, K, K), 256), dev)
  gp0 = KT - pad0 - 1
  gp1 = U - 2 * H + pad0

  def c_fwd():
    z.zero_()
    z[:, :, ::2, ::2] = x
    call(lib, 'conv2d_fwd_f32', z, Cin, None, 0, w, 0, None, None, 0, None, 1.0, u, *cd, wsf, nbf)
    call(lib, 'upfirdn2d_f32', u, kf, yc, N * Cout, U, U, 1, KT, KT, 1, 1, 1, 1, pad0, pad1, pad0, pad1)

  def c_dgrad():
    call(lib, 'upfirdn2d_f32', dout, kflip, duc, N * Cout, 2 * H, 2 * W, 1, KT, KT, 1, 1, 1, 1, gp0, gp1, gp0, gp1)
    call(lib, 'conv2d_dgrad_f32', duc, w, 0, dz, Cin, 0.0, None, 0, 0.0, 1.0, *cd, wsd, nbd)
    dxc.copy_(dz[:, :, ::2, ::2])

  def c_wgrad():
    call(lib, 'conv2d_wgrad_f32', z, Cin, None, 0, duc, dwc, 0, 1.0, wsw, nbw, *cd)

  comp = {'fwd': c_fwd, 'dgrad': c_dgrad, 'wgrad': c_wgrad}

  # both sides compute the same thing
  for d in ('fwd', 'dgrad', 'wgrad'):
    dw.zero_(); dwc.zero_()
    new[d](); comp[d]()
  torch.cuda.synchronize()
  agree = {'fwd': rel(y, yc), 'dgrad': rel(dx, dxc), 'wgrad': rel(dw, dwc)}
  assert max(agree.values()) < 1e-4, agree

  flops = 2.0 * N * H * W * Cin * Cout * K * K
  for d in ('fwd', 'dgrad', 'wgrad'):
    tn, tc = median_us(new[d], reps), median_us(comp[d], reps)
    out[d] = (tn, tc, flops / tn / 1e6, agree[d])
  return out


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--reps', type=int, default=21)
  ap.add_argument('--out', default='')
  args = ap.parse_args()
  assert args.reps >= 20
  lib = st.engine.lib.load()
  dev = torch.device('cuda:0')
  lines = [f'# tools/upconv_bench.py on {torch.cuda.get_device_name(0)}: median of {args.reps} event-bracketed calls, 3 warm-up',
           f'# K = {K}, FIR {FIR}; TFLOP/s = 2 N H W Cin Cout K^2 / time of the new call; peak {PEAK} (f32-input MFMA)',
           f'{"shape":<26} {"dir":<6} {"new us":>10} {"composition us":>15} {"speed-up":>9} {"TFLOP/s":>8} {"of peak":>8} {"agree":>9}']
  for Cin, Cout, H in SHAPES:
    for N in BATCHES:
      res = bench_shape(lib, N, Cin, Cout, H, args.reps, dev)
      torch.cuda.empty_cache()
      for d, (tn, tc, tf, ag) in res.items():
        lines.append(f'{f"b{N} {Cin}->{Cout} {H}x{H}":<26} {d:<6} {tn:10.1f} {tc:15.1f} {tc / tn:8.2f}x {tf:8.1f} {tf / PEAK:8.1%} {ag:9.1e}')
        print(lines[-1], flush=True)
  text = '\n'.join(lines) + '\n'
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write(text)


if __name__ == '__main__':
  main()
