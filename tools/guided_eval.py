#!/usr/bin/env python
"""Dynamic thresholding and guidance rescale (include/stk_guided.h) measured on the GPU.

At (B, n) = (16, 3 * 256^2) and (128, 3 * 32^2), back-to-back launches between two device events, on ONE set of buffers
(resident in the 256 MB Infinity Cache where it fits) and on a rotation of sets (up to 64, together 1 GiB where that many fit:
every launch from HBM).  Five rounds, the forms alternating inside each round, their order reversed in every second round;
the figure is the median of the five.  TB/s are those of the algorithmic byte count, in bytes per element:

  plain update       stk_dpm_update_f32, second order: read x, score, d_prev, write x, d                              20
  thresholded step   stk_dpm_predict_f32 (8 + 4), stk_abs_select_f32 after it (two levels: 4 + 4),
                     stk_dpm_threshold_update_f32 (read x, d_raw, d_prev, write x, d: 20)                             40
  select alone       stk_abs_select_f32, three levels                                                                 12
  torch step         d = cx x + cs score; torch.quantile(|d|, p, 'higher'); clamp; divide; D; x: counted as the 40 of the
                     thresholded step, whatever torch moves
  plain combine      stk_cfg_combine_f32: read c, u, write out                                                        12
  rescale            stk_cfg_rescale_f32: pass 1 (8 + 4), pass 2 (4 + 4)                                              20
  torch rescale      g = c + w (c - u); two std; f; f g: counted as the 20 of the rescale

Writes profiles/guided_eval.txt.  Sample quality under either remedy is not measured: no class-conditional checkpoint exists.

    python tools/guided_eval.py
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
ap.add_argument('--out', default=os.path.join(E.ROOT, 'profiles', 'guided_eval.txt'))
args = ap.parse_args()
assert torch.cuda.is_available(), 'guided_eval.py measures on the GPU: there is nothing to report without one'
device = torch.device('cuda', 0)
P, FLOOR = 0.995, 1.0
ROW = (1.3, 0.7, 0.45, 0.8, 0.35)          # (cx, cs, g, A, B): a second-order step
W, PHI = 2.0, 0.7
INF = float('inf')


def measure(lib, B, n, lines):
  total = B * n
  per_set = 7 * 4 * total                       # x, score, d_prev, d_raw, c-out, x-out, d-out
  sets = E.set_count(per_set)
  s = torch.cuda.current_stream().cuda_stream
  p = lambda t: t.data_ptr()
  nbytes = int(lib.guided_ws_bytes(B, n))
  ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
  q = torch.empty(B, device=device)
  rank = st.dpm_solver.threshold_rank(P, n)
  cx, cs, g, A, Bc = ROW
  forms = {k: [] for k in ('plain update', 'predict', 'select after predict', 'threshold update', 'thresholded step', 'select alone',
                           'torch step', 'plain combine', 'rescale', 'torch rescale')}
  for _ in range(sets):
    x, sc, dp = (torch.randn(B, n, device=device) * k for k in (1.5, 2.0, 1.0))
    d_raw, xo, do = (torch.empty(B, n, device=device) for _ in range(3))
    predict = lambda x=x, sc=sc, d_raw=d_raw: lib.dpm_predict_f32(p(x), p(sc), cx, cs, p(d_raw), B, n, p(ws), nbytes, s)
    select1 = lambda d_raw=d_raw: lib.abs_select_f32(p(d_raw), B, n, rank, p(q), p(ws), nbytes, 1, s)
    update = lambda x=x, d_raw=d_raw, dp=dp, xo=xo, do=do: lib.dpm_threshold_update_f32(p(x), p(d_raw), p(dp), p(q), FLOOR, g, A, Bc, p(xo),
                                                                                         p(do), B, n, s)

    def step(predict=predict, select1=select1, update=update):
      predict(); select1(); update()

    def torch_step(x=x, sc=sc, dp=dp):
      d = cx * x + cs * sc
      sq = torch.quantile(d.abs(), P, dim=1, interpolation='higher').clamp_min(FLOOR)[:, None]
      d = d.clamp(-sq, sq) / sq
      return A * x + Bc * (d + g * (d - dp)), d

    def torch_rescale(c=x, u=sc):
      gd = c + W * (c - u)
      f = PHI * (c.std(dim=1, unbiased=False, keepdim=True) / gd.std(dim=1, unbiased=False, keepdim=True)) + (1 - PHI)
      return f * gd

    forms['plain update'].append(lambda x=x, sc=sc, dp=dp, xo=xo, do=do: lib.dpm_update_f32(p(x), p(sc), p(dp), cx, cs, g, A, Bc, -INF, INF,
                                                                                             p(xo), p(do), total, s))
    forms['predict'].append(predict)
    forms['select after predict'].append(lambda predict=predict, select1=select1: select1())
    forms['threshold update'].append(update)
    forms['thresholded step'].append(step)
    forms['select alone'].append(lambda d_raw=d_raw: lib.abs_select_f32(p(d_raw), B, n, rank, p(q), p(ws), nbytes, 0, s))
    forms['torch step'].append(torch_step)
    forms['plain combine'].append(lambda x=x, sc=sc, xo=xo: lib.cfg_combine_f32(p(x), p(sc), W, p(xo), total, s))
    forms['rescale'].append(lambda x=x, sc=sc, xo=xo: lib.cfg_rescale_f32(p(x), p(sc), W, PHI, p(xo), B, n, p(ws), nbytes, s))
    forms['torch rescale'].append(torch_rescale)
    predict()                                    # every set's d_raw and the workspace hold a real prediction
  select1()
  per_elem = {'plain update': 20, 'predict': 12, 'select after predict': 8, 'threshold update': 20, 'thresholded step': 40,
              'select alone': 12, 'torch step': 40, 'plain combine': 12, 'rescale': 20, 'torch rescale': 20}
  lines.append(f'  (B, n) = ({B}, {n}), {4 * total / 2 ** 20:.1f} MiB per tensor, {sets} buffer sets in the rotation '
               f'({sets * per_set / 2 ** 20:.0f} MiB), rank {rank} of p = {P}:')
  for label, pick in (('one set (cache-resident where it fits)', lambda c: c[:1]), ('rotating sets', lambda c: c)):
    # "select after predict" times the two levels and the finish on the histogram the last predict pass of ANY set left: the
    # counts are another set's, the streaming work is the same
    rounds = [{k: E.timed(pick(forms[k]), args.reps) for k in (list(forms) if r % 2 == 0 else reversed(list(forms)))}
              for r in range(args.rounds)]
    med = {k: statistics.median(r[k] for r in rounds) for k in forms}
    lines.append(f'    {label}:')
    for k in forms:
      lines.append(f'      {k:22s} {med[k]:9.1f} us = {per_elem[k] * total / (med[k] * 1e-6) / 1e12:5.2f} TB/s of {per_elem[k]} B per element')
    lines.append(f'      thresholded step / plain update {med["thresholded step"] / med["plain update"]:.2f}x (bytes: 2.00x), / torch step '
                 f'{med["thresholded step"] / med["torch step"]:.3f}x;  rescale / plain combine {med["rescale"] / med["plain combine"]:.2f}x '
                 f'(bytes: 1.67x), / torch rescale {med["rescale"] / med["torch rescale"]:.3f}x')


lines = ['guided_eval.py: dynamic thresholding and guidance rescale on one MI355X.',
         f'{args.reps} calls per figure, {args.rounds} alternating rounds, medians.  torch {torch.__version__}.']
lib = st.engine.lib.load()
for spec in args.shapes:
  B, n = (int(v) for v in spec.split(','))
  measure(lib, B, n, lines)
  gc.collect()
  torch.cuda.empty_cache()
lines.append('Sample quality under either remedy is unmeasured: no class-conditional checkpoint exists.')
E.write(lines, args.out)
