#!/usr/bin/env python
"""The non-leaky augmentation (augment.py, include/stk_augment.h) measured on the GPU.

  accuracy   the largest observed error / bound ratio of stk_aug_warp_f32 per case of tests/test_gpu_augment.py (shape x taps:
             the 12 parameter rows of tests/_augment_ref.py against the float64 restatement and the bound derived there)
  launch     stk_aug_warp_f32 at (128, 3, 32, 32) and (128, 3, 64, 64), on one resident buffer set and rotating over enough
             sets that 1 GiB passes between two uses of one; with the draws of training (p = 0.12: most planes take the exact
             path) and with every transform firing (p = 1: every plane is filtered); median of five alternating rounds,
             beside a torch composition of the same definition: reflect padding, op.upfirdn2d 2x upsampling, F.grid_sample
             (bilinear, align_corners=False) at the same coordinates, op.upfirdn2d 2x downsampling.  The composition pads by
             at most H - 1 pixels (what F.pad's reflection allows) and filters every sample, copying the flipped plane over
             the result where the row is the identity; its difference from the kernel is reported over the samples whose
             warp stays inside that padding.
  step       a configs.edm_augment training step beside the configs.edm step of the same checkout (with the keys absent the
             step runs the programs of the parent commit: tests/golden/launch_trace.json) at batch 128, DDPM++ 32 x 32.

Writes profiles/augment_eval.txt.  Sample quality is not measured here or anywhere else: no checkpoint exists.

    python tools/augment_eval.py
"""
import argparse
import ctypes
import gc
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

import _sampler_eval as E
from _sampler_eval import st

sys.path.insert(0, os.path.join(E.ROOT, 'tests'))
import _augment_ref as R

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=200)
ap.add_argument('--steps', type=int, default=10)
ap.add_argument('--batch', type=int, default=128)
ap.add_argument('--skip', nargs='*', default=[], choices=['accuracy', 'launch', 'step'])
ap.add_argument('--out', default=os.path.join(E.ROOT, 'profiles', 'augment_eval.txt'))
args = ap.parse_args()
assert torch.cuda.is_available(), 'augment_eval.py measures on the GPU: there is nothing to report without one'
device = torch.device('cuda', 0)
lib = st.engine.lib.load()
stream = lambda: torch.cuda.current_stream().cuda_stream
FILTERS = {'box2': R.box_filter(2), 'tent4': R.tent4(), 'kaiser12': R.default_filter()}
SHAPES = [(1, 1, 8, 8), (5, 3, 8, 12), (3, 3, 32, 32), (2, 1, 64, 64)]


def taps_of(f):
  return (ctypes.c_float * len(f))(*[float(v) for v in f])


def warp(x, params, taps, T, y):
  B, C, H, W = x.shape
  lib.aug_warp_f32(x.data_ptr(), params.data_ptr(), ctypes.cast(taps, ctypes.c_void_p), T, y.data_ptr(), B, C, H, W, stream())


def accuracy(lines):
  lines.append('Accuracy: largest |kernel - float64 restatement| / bound per case (12 parameter rows each; the bound is below 1e-4 '
               'max|S| throughout, an indexing error is 0.1 max|S|).')
  for shape in SHAPES:
    B, C, H, W = shape
    cells = []
    for fname, f in FILTERS.items():
      rows = R.rows(H, W)
      names = [n for n in rows if not R.is_identity(rows[n])]
      worst, at, exact = 0.0, None, True
      for name in rows:
        x = R.image(1, C, H, W, seed=H + W + len(name))
        p = rows[name][None]
        y = torch.empty(1, C, H, W, device=device)
        warp(torch.from_numpy(x).to(device), torch.from_numpy(p).to(device), taps_of(f), len(f), y)
        got = y.cpu().numpy().astype(np.float64)
        ref = R.apply(x, p, f)
        if R.is_identity(rows[name]):
          exact = exact and np.array_equal(got, ref)
          continue
        ratio = float((np.abs(got - ref) / R.bounds(x, p, f)).max())
        if ratio > worst:
          worst, at = ratio, name
      cells.append(f'{fname} {worst:.3f} ({at}; identity rows {"exact" if exact else "NOT EXACT"})')
    lines.append(f'  {shape}: ' + '; '.join(cells) + f'.  [{len(names)} filtered rows]')


def torch_composition(x, params, f):
  """The definition by torch operators and op.upfirdn2d, for inverse maps that stay within H - 1 pixels of the plane."""
  B, C, H, W = x.shape
  T, h = len(f), len(f) // 2
  m = min(H, W) - 1
  taps = torch.from_numpy(np.asarray(f)).to(x.device)
  k2 = torch.outer(taps, taps)
  xp = F.pad(x, (m, m, m, m), mode='reflect')
  # U[j] = 2 sum_k f[k] Z[j + h - 1 - k] per axis: zero-insertion by 2, h zeros in front, h - 1 behind, gain 4 over both axes
  U = st.op.upfirdn2d(xp, 4 * k2, up=2, pad=(h, h - 1))
  qx = torch.arange(-(h - 1), 2 * W + h - 1, device=x.device, dtype=torch.float32)
  qy = torch.arange(-(h - 1), 2 * H + h - 1, device=x.device, dtype=torch.float32)
  dx = ((qx + 0.5) * 0.5 - W / 2)[None, None, :]
  dy = ((qy + 0.5) * 0.5 - H / 2)[None, :, None]
  a = params[:, :, None, None]
  sx = 2 * (a[:, 2] * dx + a[:, 3] * dy + W / 2 + a[:, 6]) - 0.5 + 2 * m      # index into the padded 2x image
  sy = 2 * (a[:, 4] * dx + a[:, 5] * dy + H / 2 + a[:, 7]) - 0.5 + 2 * m
  UW, UH = U.shape[-1], U.shape[-2]
  grid = torch.stack([(2 * sx + 1) / UW - 1, (2 * sy + 1) / UH - 1], dim=-1)   # align_corners=False: pixel i at (2i + 1)/n - 1
  V = F.grid_sample(U, grid, mode='bilinear', padding_mode='border', align_corners=False)
  return st.op.upfirdn2d(V, k2, down=2, pad=(0, 0))


def flipped(x, params):
  out = torch.where(params[:, 0, None, None, None] != 0, x.flip(3), x)
  return torch.where(params[:, 1, None, None, None] != 0, out.flip(2), out)


def composed_operator(x, params, f):
  """Flip, then the composition -- or, for a row that is the identity exactly, the flipped plane itself (step 5)."""
  b = flipped(x, params)
  eye = torch.tensor([1., 0., 0., 1., 0., 0.], device=x.device)
  exact = (params[:, 2:] == eye).all(dim=1)
  return torch.where(exact[:, None, None, None], b, torch_composition(b, params, f))


def launch(lines):
  f = st.augment.default_filter()
  taps, T = taps_of(f), len(f)
  lines.append(f'Launch: stk_aug_warp_f32 with the default 12 taps, {args.reps} back-to-back launches per figure, median of five '
               f'alternating rounds; "torch" is the composition pad / op.upfirdn2d / F.grid_sample / op.upfirdn2d of the same '
               f'definition (flips included).')
  for shape in ((args.batch, 3, 32, 32), (args.batch, 3, 64, 64)):
    B, C, H, W = shape
    for p in (0.12, 1.0):
      pipe = st.augment.AugmentPipe(p, seed=1)
      params_h, _ = pipe.draw(B, H, W)
      moved = sum(not R.is_identity(r) for r in params_h.numpy())
      per_set = 2 * B * C * H * W * 4
      n_sets = E.set_count(per_set)
      sets = [(torch.randn(shape, device=device), torch.empty(shape, device=device)) for _ in range(n_sets)]
      params = params_h.to(device)
      resident = lambda: warp(sets[0][0], params, taps, T, sets[0][1])
      rotating = E.rotating(lambda s: warp(s[0], params, taps, T, s[1]), sets)
      composed = lambda: composed_operator(sets[0][0], params, f)
      rounds = {'resident': [], 'rotating': [], 'torch': []}
      for r in range(5):
        order = list(rounds) if r % 2 == 0 else list(reversed(list(rounds)))
        for k in order:
          call = {'resident': resident, 'rotating': rotating, 'torch': composed}[k]
          rounds[k].append(E.launches_alone(call, args.reps if k != 'torch' else max(10, args.reps // 10), 1)[0])
      med = {k: float(np.median(v)) for k, v in rounds.items()}
      # the composition against the kernel, on the samples whose warp stays inside the padding it can make
      y = torch.empty(shape, device=device)
      warp(sets[0][0], params, taps, T, y)
      z = composed()
      reach = []
      for b in range(B):
        sx, sy, _, _ = R._coords(params_h[b].numpy(), H, W, T, np.float64, False)
        reach.append(max(-sx.min(), -sy.min(), sx.max() - 2 * W, sy.max() - 2 * H) / 2 + T / 2 + 2 <= min(H, W) - 1)
      inside = torch.tensor(reach, device=device)
      diff = float(((y - z).abs().amax(dim=(1, 2, 3)) * inside).max() / sets[0][0].abs().max())
      lines.append(f'  {shape}, p = {p:g} ({moved} of {B} samples filtered): resident {med["resident"]:.1f} us, rotating over '
                   f'{n_sets} sets {med["rotating"]:.1f} us, torch composition {med["torch"]:.1f} us ({med["torch"] / med["resident"]:.1f}x); '
                   f'largest |kernel - composition| / max|x| over the {int(inside.sum())} samples inside its padding {diff:.2e}.')
      del sets
      gc.collect()
      torch.cuda.empty_cache()


def step(lines):
  B = args.batch
  took = {}
  for name, make in (('edm', st.configs.edm), ('edm_augment', st.configs.edm_augment)):
    cfg = make(st.configs.get_config('cifar10_ddpmpp_nll_st'))
    cfg.device = device
    sde = st.sde_lib.get_sde(cfg, None)
    st.engine.ddp.seed_everything(cfg.seed)
    state, step_fn = E.bench.build_training(st, cfg, sde)
    batch = st.datasets.synthetic_batch(cfg, B, device=device)
    took[name] = (state, step_fn, batch)
  calls = {k: (lambda v=v: v[1](v[0], v[2])) for k, v in took.items()}
  for _ in range(3):
    for c in calls.values():
      c()
  ms = E.wall({k: (lambda c=c: [c() for _ in range(args.steps)]) for k, c in calls.items()}, 5)
  a, b = ms['edm'] / args.steps, ms['edm_augment'] / args.steps
  lines.append(f'Step: DDPM++ CIFAR-10 32x32 at batch {B}, {args.steps} steps per figure, median of five alternating rounds: '
               f'configs.edm {a:.2f} ms, configs.edm_augment (p = 0.12, augment_dim = 9) {b:.2f} ms ({b - a:+.2f} ms, '
               f'{100 * (b / a - 1):+.1f} %).')


lines = ['augment_eval.py: the non-leaky augmentation on one MI355X.']
for name, fn in (('accuracy', accuracy), ('launch', launch), ('step', step)):
  if name not in args.skip:
    fn(lines)
lines.append('Sample quality under augmentation is unmeasured: no checkpoint exists.')
E.write(lines, args.out)
