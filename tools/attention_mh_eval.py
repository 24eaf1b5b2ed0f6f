#!/usr/bin/env python
"""The multi-head attention entries (include/stk_attention_mh.h) timed beside the single-head entries on one MI355X.

Kernels.  For (B, C, T) = (128, 256, 256), (4, 256, 1024) and the batch-1 sampling case (1, 256, 256): the forward and the
backward of stk_attention_mh_* with heads h in {1, 2, 4, 8} (d = 256, 128, 64, 32), each beside the existing single-head
entry at the same (B, C, T) -- stk_attention_* for T <= 256, stk_attention_long_* above.  The algorithmic FLOP count
4 B T^2 C (forward; twice that backward) does not depend on h, so the single-head entry is the comparator of every row; it
is timed twice per round ("single" and "again"), and the ratio of the two series is the same-box run-to-run spread any
difference has to be read against.  Whole entries (|x| passes and plane splits included), HIP events around `reps`
back-to-back calls after a warm-up, `rounds` rounds with the forms alternating; the figure of a form is its median round.

Network.  The CIFAR-10 DDPM++ network (class-conditional, 10 classes) with model.num_heads = 4 beside the same network
with one head: a guided evaluation (classifier-free guidance, one pass at batch 2 B) and a training step, wall time over a
device synchronisation, rounds alternating.

Writes profiles/attention_mh_eval.txt.

    python tools/attention_mh_eval.py
"""
import argparse
import os
import statistics
import time

import torch

import _sampler_eval as E
from _sampler_eval import bench, st

ap = argparse.ArgumentParser()
ap.add_argument('--shapes', nargs='*', default=['128,256,256', '4,256,1024', '1,256,256'], help='B,C,T')
ap.add_argument('--heads', default='1,2,4,8')
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--min-ms', type=float, default=60.0, help='each timed window runs at least this long')
ap.add_argument('--net-batch', type=int, default=16)
ap.add_argument('--net-reps', type=int, default=10)
ap.add_argument('--skip-network', action='store_true')
ap.add_argument('--out', default=os.path.join(E.ROOT, 'profiles', 'attention_mh_eval.txt'))
args = ap.parse_args()
assert torch.cuda.is_available(), 'attention_mh_eval.py measures on the GPU: there is nothing to report without one'
device = torch.device('cuda', 0)
lib = st.engine.lib.load()
assert lib.has_attention_mh, 'the library does not export include/stk_attention_mh.h'
p = lambda t: t.data_ptr()


def window(call, reps):
  """ms per call of `reps` back-to-back calls between two events."""
  e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  e0.record()
  for _ in range(reps):
    call()
  e1.record()
  e1.synchronize()
  return e0.elapsed_time(e1) / reps


def kernels(lines, B, C, T):
  heads = [int(h) for h in args.heads.split(',')]
  q, k, v, do = (torch.randn(B, C, T, device=device) for _ in range(4))
  o, dq, dk, dv = (torch.zeros(B, C, T, device=device) for _ in range(4))
  lse, delta = torch.zeros(B * max(heads) * T, device=device), torch.zeros(B * max(heads) * T, device=device)
  rec = torch.zeros(1024, device=device)
  short = T <= 256
  ws_bytes = 0 if short else int(lib.attention_long_ws_bytes(B, C, T))
  ws = torch.empty(ws_bytes // 4 + 4, device=device)
  s = torch.cuda.current_stream().cuda_stream
  ct = C * T

  def single(direction):
    sc = C ** -0.5
    if short:
      if direction == 'fwd':
        return lambda: lib.attention_fwd_f32(p(q), p(k), p(v), ct, p(o), p(lse), p(rec), B, C, T, sc, s)
      return lambda: lib.attention_bwd_f32(p(q), p(k), p(v), ct, p(do), p(lse), p(rec), p(delta), p(dq), 0.0, p(dk), 0.0, p(dv),
                                           0.0, ct, B, C, T, sc, s)
    if direction == 'fwd':
      return lambda: lib.attention_long_fwd_f32(p(q), p(k), p(v), ct, p(o), p(lse), p(rec), B, C, T, sc, p(ws), ws_bytes, s)
    return lambda: lib.attention_long_bwd_f32(p(q), p(k), p(v), ct, p(o), p(do), p(lse), p(rec), p(delta), p(dq), 0.0, p(dk),
                                              0.0, p(dv), 0.0, ct, B, C, T, sc, p(ws), ws_bytes, s)

  def mh(direction, h):
    sc = (C // h) ** -0.5
    assert lib.attention_mh_ok(B, C, T, h) == 1 and int(lib.attention_mh_ws_bytes(B, C, T, h)) <= ws_bytes
    if direction == 'fwd':
      return lambda: lib.attention_mh_fwd_f32(p(q), p(k), p(v), ct, p(o), p(lse), p(rec), B, C, T, h, sc, p(ws), ws_bytes, s)
    return lambda: lib.attention_mh_bwd_f32(p(q), p(k), p(v), ct, p(o), p(do), p(lse), p(rec), p(delta), p(dq), 0.0, p(dk), 0.0,
                                            p(dv), 0.0, ct, B, C, T, h, sc, p(ws), ws_bytes, s)

  lines.append(f'(B, C, T) = ({B}, {C}, {T}), {"short" if short else "streaming"} form; single-head entry '
               f'{"stk_attention_*" if short else "stk_attention_long_*"}:')
  for direction in ('fwd', 'bwd'):
    forms = [('single', single(direction)), ('again', single(direction))] + [(f'h={h}', mh(direction, h)) for h in heads]
    reps = {}
    for name, call in forms:
      if direction == 'bwd':                     # every backward reads the lse (and the records) of ITS forward
        (single('fwd') if name in ('single', 'again') else mh('fwd', int(name[2:])))()
      for _ in range(3):
        call()
      torch.cuda.synchronize()
      reps[name] = max(3, int(args.min_ms / max(window(call, 3), 1e-3)) + 1)
    ms = {name: [] for name, _ in forms}
    for _ in range(args.rounds):
      for name, call in forms:
        if direction == 'bwd':
          (single('fwd') if name in ('single', 'again') else mh('fwd', int(name[2:])))()
        ms[name].append(window(call, reps[name]))
    med = {name: statistics.median(v) for name, v in ms.items()}
    flops = (4.0 if direction == 'fwd' else 8.0) * B * T * T * C
    spread = max(med['single'], med['again']) / min(med['single'], med['again'])
    lines.append(f'  {direction}: single {med["single"] * 1e3:.1f} us ({flops / med["single"] * 1e-9:.1f} TFLOP/s), again '
                 f'{med["again"] * 1e3:.1f} us (spread {spread:.3f}x; rounds min-max '
                 f'{min(ms["single"] + ms["again"]) * 1e3:.1f}-{max(ms["single"] + ms["again"]) * 1e3:.1f} us)')
    for h in heads:
      m = med[f'h={h}']
      lines.append(f'    heads {h} (d = {C // h}): {m * 1e3:.1f} us ({flops / m * 1e-9:.1f} TFLOP/s), mh / single = '
                   f'{m / med["single"]:.3f}  (rounds {" ".join(f"{x * 1e3:.1f}" for x in ms[f"h={h}"])})')


def wall_ms(call, reps):
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(reps):
    call()
  torch.cuda.synchronize()
  return 1e3 * (time.perf_counter() - t0) / reps


def network(lines):
  mu = st.models.utils
  cfg_name, batch, desc = bench.WORKLOADS['cifar10']
  B = args.net_batch
  guided, steps = {}, {}
  keep = []
  for h in (1, 4):
    cfg = st.configs.get_config(cfg_name)
    cfg.device = device
    cfg.model.num_classes = 10
    if h > 1:
      cfg.model.num_heads = h
    sde = st.sde_lib.get_sde(cfg, None)
    torch.manual_seed(0)
    model = mu.create_model(cfg, sde)
    model.eval()
    with torch.no_grad():
      model.module.class_emb.weight.normal_(0., 0.1)
    shape = (B, cfg.data.num_channels, cfg.data.image_size, cfg.data.image_size)
    score_fn = mu.get_score_fn(cfg, sde, model, train=False, continuous=cfg.training.continuous)
    x = sde.prior_sampling(shape).to(device).contiguous()
    t = torch.ones(B, device=device) * 0.5
    y = st.datasets.synthetic_classes(cfg, B, device=device, generator=None)

    def call(model=model, score_fn=score_fn, x=x, t=t, y=y):
      with mu.class_condition(model, y, 1.5):
        return score_fn(x, t)
    guided[h] = (model, call)
    cfg_t = st.configs.get_config(cfg_name)
    cfg_t.device = device
    if h > 1:
      cfg_t.model.num_heads = h
    torch.manual_seed(0)
    state, step = bench.build_training(st, cfg_t, sde)
    batches = [st.datasets.synthetic_batch(cfg_t, batch, generator=torch.Generator().manual_seed(i)).to(device) for i in range(4)]
    steps[h] = (lambda state=state, step=step, batches=batches, i=[0]: (step(state, batches[i[0] % 4]), i.__setitem__(0, i[0] + 1)))
    keep.append((state, step))
  g_ms, s_ms = {1: [], 4: []}, {1: [], 4: []}
  for h in (1, 4):
    for _ in range(3):
      steps[h]()
  for _ in range(args.rounds):
    for h in (1, 4):
      s_ms[h].append(wall_ms(steps[h], args.net_reps))
  for h in (1, 4):
    model, call = guided[h]
    with mu.sampling_run(model):
      for _ in range(3):
        call()
      for _ in range(args.rounds):
        g_ms[h].append(wall_ms(call, args.net_reps))
  lines.append(f'{desc}, num_classes = 10: {args.rounds} rounds of {args.net_reps} calls per figure after a warm-up, median round '
               f'(all rounds in brackets).')
  for what, ms, b in (('guided evaluation (guidance 1.5, one pass at 2 B)', g_ms, B), ('training step', s_ms, batch)):
    m1, m4 = statistics.median(ms[1]), statistics.median(ms[4])
    lines.append(f'  {what}, batch {b}: 1 head {m1:.2f} ms [{" ".join(f"{v:.2f}" for v in ms[1])}], 4 heads {m4:.2f} ms '
                 f'[{" ".join(f"{v:.2f}" for v in ms[4])}], 4 heads / 1 head = {m4 / m1:.3f}')


lines = ['attention_mh_eval.py: the multi-head attention entries beside the single-head entries on one MI355X ('
         + torch.cuda.get_device_name(0) + f').  Whole entries, HIP events, windows of >= {args.min_ms:.0f} ms, {args.rounds} '
         'rounds with the forms alternating, median round.  "mh / single" is to be read against the spread of "single" / "again".']
for spec in args.shapes:
  B, C, T = (int(v) for v in spec.split(','))
  kernels(lines, B, C, T)
if not args.skip_network:
  network(lines)
E.write(lines, args.out)
