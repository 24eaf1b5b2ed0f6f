#!/usr/bin/env python
"""Per-family kernel time per step from a `rocprofv3 --kernel-trace` database (the rocpd SQLite file), split into the fp32
and the fp16 (one-product) symbols of the convolution kernels.  For a trace of tools/fp16_train_step.py, which runs the same
number of steps in each precision (`--steps` = warm-up + timed steps per precision); kernels both precisions launch
(GroupNorm, resampling, attention, optimizer, slab sums) are reported once, per step of either.

    rocprofv3 --kernel-trace -d prof -o trace -- python tools/fp16_train_step.py --workload cifar10 --repeats 1 --steps 5 --warmup 2
    python tools/kernel_families.py prof/trace_results.db --steps 7
"""
import argparse
import collections
import re
import sqlite3

ap = argparse.ArgumentParser()
ap.add_argument('db')
ap.add_argument('--steps', type=int, required=True, help='steps per precision in the trace')
args = ap.parse_args()

FAMILIES = [   # (family, regex on the kernel name), first match wins
  ('wgrad planes x2w::wgrad_kernel', r'x2w::wgrad_kernel'),
  ('wgrad fp32 operands x2::wgemm_kernel', r'x2::wgemm_kernel'),
  ('wgrad fp32 operands x2::wgrad3_kernel', r'x2::wgrad3_kernel'),
  ('fwd planes x2d (halo / gemm)', r'x2d::gemm(_halo)?_kernel<.*?::(EpFwd|EpSlab)\b'),
  ('dgrad planes x2d (halo / gemm)', r'x2d::gemm(_halo)?_kernel<.*?::EpDgrad\b'),
  ('fwd fp32 operands x2::gemm_kernel', r'x2::gemm_kernel<.*?::EpFwd\b'),
  ('dgrad fp32 operands x2::gemm_kernel', r'x2::gemm_kernel<.*?::EpDgrad\b'),
  ('other convolution kernels (f32-input tiles, thin, wprep, slab sums, planes)', r'conv|thin|wprep|wamax|slab|splitk|split_planes|igemm|gemm'),
  ('GroupNorm', r'gn_'),
  ('attention', r'attn'),
  ('everything else', r'.'),
]


def is_f16(name):
  """the one-product symbols: a OneProduct epilogue, hi-plane loaders, or wgrad_kernel's X1_FORM bit (FORM 17 / 18)"""
  return bool(re.search(r'OneProduct|ActLoader16|RowsU16|RowsB16|wgrad_kernel<\d+, 1[78]>', name))


c = sqlite3.connect(args.db)
tot = collections.defaultdict(float)
for name, dur in c.execute('select name, duration from kernels'):
  fam = next(f for f, rx in FAMILIES if re.search(rx, name))
  split = fam.startswith(('wgrad', 'fwd', 'dgrad'))
  mode = ('fp16' if is_f16(name) else 'fp32') if split else 'both'
  tot[(fam, mode)] += dur * 1e-6
print(f'{"family":<78} {"fp32 ms/step":>12} {"fp16 ms/step":>12} {"ratio":>6}')
s32 = s16 = 0.0
for fam, _ in FAMILIES:
  if (fam, 'both') in tot:
    v = tot[(fam, 'both')] / (2 * args.steps)
    s32 += v
    s16 += v
    print(f'{fam:<78} {v:12.3f} {v:12.3f}   (both)')
  elif (fam, 'fp32') in tot or (fam, 'fp16') in tot:
    a, b = tot.get((fam, 'fp32'), 0.0) / args.steps, tot.get((fam, 'fp16'), 0.0) / args.steps
    s32 += a
    s16 += b
    print(f'{fam:<78} {a:12.3f} {b:12.3f} {a / b if b else float("nan"):6.2f}')
print(f'{"sum of kernel durations (both streams)":<78} {s32:12.3f} {s16:12.3f} {s32 / s16:6.2f}')
