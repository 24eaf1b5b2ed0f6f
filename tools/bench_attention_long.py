#!/usr/bin/env python
"""Attention-core timings above and at 16 x 16: the short fused kernels (stk_attention_*, T <= 256), the streaming
kernels (include/stk_attention_long.h) and the GEMM + softmax form (stk_gemm_f32 / stk_softmax_*, engine/graph.py
AttentionCore's fallback) on one [B, C, T] problem each.

    python tools/bench_attention_long.py [--batch 128] [--reps 5] [--C 128,256] [--T 256,1024,4096]

One line per (form, direction, shape): average milliseconds (HIP events on the launch stream, whole entry: the |x| passes
and plane splits of the streaming entries included) and the achieved TFLOP/s of the algorithmic count -- 4 B T^2 C per
forward, 8 B T^2 C per backward (recomputed scores not counted).  The GEMM form's [B, T, T] matrices are processed in
batch slices whenever B T^2 would reach 2^31 elements (the ABI's limit per tensor); its time is the sum over the slices.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
  if p not in sys.path:
    sys.path.insert(0, p)

import torch

import soft_truncation_amd as st
from _util import call


def timeit(fn, reps):
  fn()
  torch.cuda.synchronize()
  s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  s.record()
  for _ in range(reps):
    fn()
  e.record()
  torch.cuda.synchronize()
  return s.elapsed_time(e) / reps      # ms


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=128)
  ap.add_argument('--reps', type=int, default=5)
  ap.add_argument('--C', default='128,256')
  ap.add_argument('--T', default='256,1024,4096')
  ap.add_argument('--json', default='', help='also write the rows to this file')
  args = ap.parse_args()
  lib = st.engine.lib.load()
  d = torch.device('cuda')
  B, rows = args.batch, []

  def rec(form, dirn, C, T, ms, flops):
    r = {'form': form, 'dir': dirn, 'B': B, 'C': C, 'T': T, 'ms': round(ms, 4), 'tflops': round(flops / ms * 1e-9, 1)}
    rows.append(r)
    print(f"{form:6s} {dirn:3s} B{B} C{C:<4d} T{T:<5d} {ms:9.3f} ms  {r['tflops']:7.1f} TFLOP/s", flush=True)

  for C in (int(c) for c in args.C.split(',')):
    for T in (int(t) for t in args.T.split(',')):
      q, k, v, do = (torch.randn(B, C, T, device=d) for _ in range(4))
      o, dq, dk, dv = (torch.empty(B, C, T, device=d) for _ in range(4))
      lse, delta, rcd = torch.empty(B, T, device=d), torch.empty(B, T, device=d), torch.zeros(1024, device=d)
      sc = float(C) ** -0.5
      ffl, bfl = 4.0 * B * T * T * C, 8.0 * B * T * T * C
      if int(lib.attention_ok(B, C, T)):
        rec('short', 'fwd', C, T, timeit(lambda: call(lib, 'attention_fwd_f32', q, k, v, C * T, o, lse, rcd, B, C, T, sc), args.reps), ffl)
        rec('short', 'bwd', C, T, timeit(lambda: call(lib, 'attention_bwd_f32', q, k, v, C * T, do, lse, rcd, delta, dq, 0.0, dk, 0.0,
                                                      dv, 0.0, C * T, B, C, T, sc), args.reps), bfl)
      if int(lib.attention_long_ok(B, C, T)):
        wsb = int(lib.attention_long_ws_bytes(B, C, T))
        ws = torch.empty(wsb // 4, device=d)
        rec('long', 'fwd', C, T, timeit(lambda: call(lib, 'attention_long_fwd_f32', q, k, v, C * T, o, lse, rcd, B, C, T, sc, ws, wsb),
                                        args.reps), ffl)
        rec('long', 'bwd', C, T, timeit(lambda: call(lib, 'attention_long_bwd_f32', q, k, v, C * T, o, do, lse, rcd, delta, dq, 0.0,
                                                     dk, 0.0, dv, 0.0, C * T, B, C, T, sc, ws, wsb), args.reps), bfl)
        del ws
      # GEMM form, in batch slices of nb images
      nb = B
      while nb * T * T >= 2 ** 31:
        nb //= 2
      S, Pm = torch.empty(nb, T, T, device=d), torch.empty(nb, T, T, device=d)

      def sl(t, i):
        return t[i:i + nb]

      def gemm_fwd():
        for i in range(0, B, nb):
          qi, ki, vi, oi = sl(q, i), sl(k, i), sl(v, i), sl(o, i)
          call(lib, 'gemm_f32', qi, 1, T, C * T, ki, T, 1, C * T, S, T, 1, T * T, None, 0, T, T, C, nb, 1.0, 0.0)
          call(lib, 'softmax_fwd_f32', S, Pm, nb * T, T, sc)
          call(lib, 'gemm_f32', vi, T, 1, C * T, Pm, 1, T, T * T, oi, T, 1, C * T, None, 0, C, T, T, nb, 1.0, 0.0)

      def gemm_bwd():       # the probabilities of the slice are assumed in Pm (as the engine keeps them from the forward)
        for i in range(0, B, nb):
          qi, ki, vi, doi = sl(q, i), sl(k, i), sl(v, i), sl(do, i)
          call(lib, 'gemm_f32', doi, 1, T, C * T, vi, T, 1, C * T, S, T, 1, T * T, None, 0, T, T, C, nb, 1.0, 0.0)
          call(lib, 'gemm_f32', doi, T, 1, C * T, Pm, T, 1, T * T, sl(dv, i), T, 1, C * T, None, 0, C, T, T, nb, 1.0, 0.0)
          call(lib, 'softmax_bwd_f32', Pm, S, S, nb * T, T, sc)
          call(lib, 'gemm_f32', ki, T, 1, C * T, S, 1, T, T * T, sl(dq, i), T, 1, C * T, None, 0, C, T, T, nb, 1.0, 0.0)
          call(lib, 'gemm_f32', qi, T, 1, C * T, S, T, 1, T * T, sl(dk, i), T, 1, C * T, None, 0, C, T, T, nb, 1.0, 0.0)

      rec('gemm', 'fwd', C, T, timeit(gemm_fwd, args.reps), ffl)
      rec('gemm', 'bwd', C, T, timeit(gemm_bwd, args.reps), bfl)
      del S, Pm, q, k, v, do, o, dq, dk, dv
      torch.cuda.empty_cache()
  if args.json:
    with open(args.json, 'w') as f:
      json.dump({'device': torch.cuda.get_device_name(0), 'rows': rows}, f, indent=1)


if __name__ == '__main__':
  main()
