"""The streaming attention core (csrc/attention_long.hip, include/stk_attention_long.h) against a float64 restatement of
models/layerspp.py:95-99 and of its autograd on the CPU (the plain-C checker has no long entries).

Bounds as test_gpu_kernels.test_attention: 1e-4 of max |ref| for o, dq, dk, dv and delta, 1e-5 for lse."""
import pytest
import torch

from _util import rnd

pytestmark = pytest.mark.gpu

EUNSUPPORTED = -3


def ref_attention(q, k, v, do, scale, chunk=2048):
  """float64 o, lse, delta, dq, dk, dv of [B, C, T] inputs; queries in chunks so that no [T, T] matrix is whole."""
  q, k, v, do = (t.double() for t in (q, k, v, do))
  B, C, T = q.shape
  o, lse, delta = torch.zeros_like(q), torch.zeros(B, T, dtype=torch.float64), torch.zeros(B, T, dtype=torch.float64)
  dq, dk, dv = torch.zeros_like(q), torch.zeros_like(q), torch.zeros_like(q)
  for b in range(B):
    for t0 in range(0, T, chunk):
      qs, dos = q[b, :, t0:t0 + chunk], do[b, :, t0:t0 + chunk]              # [C, n]
      s = scale * qs.t() @ k[b]                                                # [n, T]
      ls = torch.logsumexp(s, 1)
      p = torch.exp(s - ls[:, None])
      os_ = v[b] @ p.t()                                                       # [C, n]
      o[b, :, t0:t0 + chunk], lse[b, t0:t0 + chunk] = os_, ls
      de = (dos * os_).sum(0)
      delta[b, t0:t0 + chunk] = de
      dp = dos.t() @ v[b]                                                      # [n, T]
      ds = p * (dp - de[:, None])
      dq[b, :, t0:t0 + chunk] = scale * k[b] @ ds.t()
      dk[b] += scale * qs @ ds
      dv[b] += dos @ p
  return {'o': o, 'lse': lse, 'delta': delta, 'dq': dq, 'dk': dk, 'dv': dv}


def run_long(lib, q, k, v, do, scale, stacked=False, beta=0.0, g0=None, dev='cuda'):
  """Forward + backward on the GPU; g0: initial dq, dk, dv (accumulated into with beta)."""
  B, C, T = q.shape
  ws_bytes = int(lib.attention_long_ws_bytes(B, C, T))
  assert ws_bytes > 0
  ws = torch.empty(ws_bytes // 4 + 4, device=dev)
  o, lse, delta = torch.zeros(B, C, T, device=dev), torch.zeros(B, T, device=dev), torch.zeros(B, T, device=dev)
  rec = torch.zeros(1024, device=dev)
  g0 = g0 if g0 is not None else [torch.zeros(B, C, T)] * 3
  bs = 3 * C * T if stacked else C * T
  if stacked:
    qkv, g = torch.cat([q, k, v], 1).to(dev), torch.cat(g0, 1).to(dev)
    ins = [qkv[0, i * C:].data_ptr() for i in range(3)]
    outs = [g[0, i * C:].data_ptr() for i in range(3)]
  else:
    keep = [q.to(dev), k.to(dev), v.to(dev)] + [t.clone().to(dev) for t in g0]
    ins, outs = [t.data_ptr() for t in keep[:3]], [t.data_ptr() for t in keep[3:]]
  d_o = do.to(dev)
  stream = torch.cuda.current_stream().cuda_stream
  lib.attention_long_fwd_f32(ins[0], ins[1], ins[2], bs, o.data_ptr(), lse.data_ptr(), rec.data_ptr(), B, C, T, scale,
                             ws.data_ptr(), ws_bytes, stream)
  lib.attention_long_bwd_f32(ins[0], ins[1], ins[2], bs, o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), rec.data_ptr(),
                             delta.data_ptr(), outs[0], beta, outs[1], beta, outs[2], beta, bs, B, C, T, scale,
                             ws.data_ptr(), ws_bytes, stream)
  torch.cuda.synchronize()
  if stacked:
    dq, dk, dv = (g[:, i * C:(i + 1) * C].contiguous() for i in range(3))
  else:
    dq, dk, dv = keep[3:]
  return {n: t.cpu() for n, t in (('o', o), ('lse', lse), ('delta', delta), ('dq', dq), ('dk', dk), ('dv', dv))}


def worst(got, ref):
  """max |got - ref| / max |ref| per output"""
  return {n: ((got[n].double() - ref[n]).abs().max() / ref[n].abs().max().clamp_min(1e-300)).item() for n in ref}


def check(got, ref, what, rtol=1e-4, lse_tol=1e-5, names=('o', 'dq', 'dk', 'dv', 'delta')):
  for n in names:
    err = (got[n].double() - ref[n]).abs().max().item()
    bound = rtol * ref[n].abs().max().item()
    assert err <= bound, f'{what}: {n} max err {err:.3e} > {bound:.3e} ({err / max(ref[n].abs().max().item(), 1e-300):.2e} rel)'
  err = (got['lse'].double() - ref['lse']).abs().max().item()
  bound = lse_tol * max(1.0, ref['lse'].abs().max().item())
  assert err <= bound, f'{what}: lse max err {err:.3e} > {bound:.3e}'


def inputs(B, C, T, mags=(1., 1., 1., 1.), seed=1):
  return [rnd(B, C, T, seed=seed + i) * m for i, m in enumerate(mags)]


SHAPES = [
  (2, 128, 1024),
  (2, 256, 1024),
  (1, 256, 4096),
  (2, 192, 2304),      # 48 x 48
  (2, 64, 660),        # not a tile multiple
  (3, 32, 260),
  (1, 64, 16384),      # the longest sequence the entries take (B and C kept small for the float64 reference)
]


@pytest.mark.parametrize('stacked', [False, True], ids=['separate', 'stacked'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'B{s[0]}C{s[1]}T{s[2]}')
def test_attention_long_matches_float64(hip_lib, shape, stacked):
  """o, lse, delta and the three gradients, with beta in {0, 0.5, 1} (the gradients accumulate into random values)."""
  B, C, T = shape
  assert hip_lib.attention_long_ok(B, C, T) == 1
  q, k, v, do = inputs(B, C, T)
  scale = C ** -0.5
  ref = ref_attention(q, k, v, do, scale)
  g0 = [rnd(B, C, T, seed=9 + i) * 0.1 for i in range(3)]
  for beta in (0.0, 0.5, 1.0):
    got = run_long(hip_lib, q, k, v, do, scale, stacked=stacked, beta=beta, g0=g0)
    want = dict(ref)
    for i, n in enumerate(('dq', 'dk', 'dv')):
      want[n] = ref[n] + beta * g0[i].double()
    check(got, want, f'{shape} stacked={stacked} beta={beta}')
  print(f'worst {shape} stacked={stacked}:', {n: f'{e:.2e}' for n, e in worst(got, want).items()})


def test_attention_long_magnitudes_far_apart(hip_lib):
  """Every tensor has its own power-of-two scale: q, k, v, dO of magnitudes 3e3, 2e-3, 5e-4, 1e-6."""
  B, C, T = 2, 128, 1024
  q, k, v, do = inputs(B, C, T, mags=(3e3, 2e-3, 5e-4, 1e-6))
  scale = C ** -0.5
  check(run_long(hip_lib, q, k, v, do, scale), ref_attention(q, k, v, do, scale), 'magnitudes')


def _direction(C, T, gen):
  u = torch.randn(C, generator=gen)
  return u / u.norm()


def test_attention_long_rescale_every_chunk(hip_lib):
  """(a) Row maxima that grow chunk after chunk along the key order: every chunk of 32 keys raises the running maximum
  of every query (scale s[t, t'] ~ t' / 16 plus noise), so the forward rescales its accumulator at every chunk."""
  B, C, T = 2, 64, 1024
  gen = torch.Generator().manual_seed(3)
  u = _direction(C, T, gen)
  q = (u[None, :, None] * 8.0 + 0.05 * torch.randn(B, C, T, generator=gen))
  ramp = torch.arange(T, dtype=torch.float32) / 16.0 * (C ** 0.5) / 8.0
  k = u[None, :, None] * ramp[None, None, :] + 0.05 * torch.randn(B, C, T, generator=gen)
  v, do = rnd(B, C, T, seed=4), rnd(B, C, T, seed=5)
  scale = C ** -0.5
  check(run_long(hip_lib, q, k, v, do, scale), ref_attention(q, k, v, do, scale), 'growing maxima')


def test_attention_long_maximum_in_last_chunk(hip_lib):
  """(b) The largest score of every query sits in the last chunk and exceeds the earlier ones by ~30."""
  B, C, T = 2, 64, 1000
  gen = torch.Generator().manual_seed(6)
  u = _direction(C, T, gen)
  q = u[None, :, None] * 8.0 + 0.02 * torch.randn(B, C, T, generator=gen)
  k = 0.05 * torch.randn(B, C, T, generator=gen)
  k[:, :, T - 3:] += u[None, :, None] * 30.0          # scale * s = 30 / 8 * 8 = 30 above the rest
  v, do = rnd(B, C, T, seed=7), rnd(B, C, T, seed=8)
  scale = C ** -0.5
  check(run_long(hip_lib, q, k, v, do, scale), ref_attention(q, k, v, do, scale), 'last-chunk maximum')


def test_attention_long_peaked_rows(hip_lib):
  """(c) Peaked rows, one-hot within fp32: query t looks along one channel j(t), so scale * s[t, t'] = 1000 k[j(t), t'] is
  a single product (no sum whose rounding would blur the peak) and the top key of a row leads the next by hundreds.

  The forward (o, lse) and dv are checked.  dq and dk are not: with p = 1 - O(e^-100) on the peak, ds = p (dp - delta)
  cancels dp against delta = sum p dp to well below fp32 resolution, so no fp32 evaluation (the short kernels' neither)
  has a relative error of 1e-4 there; they are exercised by the other cases."""
  B, C, T = 2, 64, 1024
  gen = torch.Generator().manual_seed(11)
  scale = C ** -0.5
  j = torch.randint(0, C, (B, T), generator=gen)
  q = torch.zeros(B, C, T).scatter_(1, j[:, None, :], 1.0 / scale)
  k = 1000.0 * torch.randn(B, C, T, generator=gen)
  v, do = rnd(B, C, T, seed=12), rnd(B, C, T, seed=13)
  ref = ref_attention(q, k, v, do, scale)
  gap = ref['lse'] - scale * torch.einsum('bct,bcs->bts', q.double(), k.double()).amax(2)      # log(1 / p_max)
  assert (gap < 2 ** -24).float().mean() > 0.8                                                   # most rows one-hot in fp32
  check(run_long(hip_lib, q, k, v, do, scale), ref, 'peaked', names=('o', 'dv', 'delta'))


def test_attention_long_ds_grows_along_both_streams(hip_lib):
  """Backward rescaling: |ds| grows by 4x per chunk of 32 along the keys (probabilities rising along the key order:
  the stream of the DQ kernel) in one case and along the queries (dO rising: the stream of the DKV kernel) in the other,
  so the per-column ds scale drops at every chunk."""
  B, C, T = 2, 64, 512
  gen = torch.Generator().manual_seed(13)
  u = _direction(C, T, gen)
  scale = C ** -0.5
  # p[t, t'] ~ 4^(t' / 32): scale s = t' ln 4 / 32
  q = u[None, :, None] * 8.0 + 0.01 * torch.randn(B, C, T, generator=gen)
  ramp = torch.arange(T, dtype=torch.float32) * (torch.log(torch.tensor(4.0)) / 32.0)
  k = u[None, :, None] * ramp[None, None, :] + 0.01 * torch.randn(B, C, T, generator=gen)
  v, do = rnd(B, C, T, seed=14), rnd(B, C, T, seed=15)
  check(run_long(hip_lib, q, k, v, do, scale), ref_attention(q, k, v, do, scale), 'ds growing along keys')
  # dO[:, t] ~ 4^(t / 32)
  q, k, v = inputs(B, C, T, seed=16)[:3]
  grow = torch.pow(4.0, (torch.arange(T) // 32).float())
  do = rnd(B, C, T, seed=19) * grow[None, None, :]
  check(run_long(hip_lib, q, k, v, do, scale), ref_attention(q, k, v, do, scale), 'ds growing along queries')


@pytest.mark.parametrize('C', [64, 256])
@pytest.mark.parametrize('T', [64, 256])
def test_attention_long_agrees_with_short_kernels(hip_lib, C, T):
  """Where both families take the shape, the long and the short entries agree to 1e-5 of max |.|."""
  B = 2
  q, k, v, do = inputs(B, C, T, seed=21)
  scale = C ** -0.5
  long_ = run_long(hip_lib, q, k, v, do, scale)
  dev = 'cuda'
  o, lse, delta, rec = (torch.zeros(B, C, T, device=dev), torch.zeros(B, T, device=dev), torch.zeros(B, T, device=dev),
                        torch.zeros(1024, device=dev))
  qd, kd, vd, dod = (t.to(dev) for t in (q, k, v, do))
  dq, dk, dv = (torch.zeros(B, C, T, device=dev) for _ in range(3))
  stream = torch.cuda.current_stream().cuda_stream
  hip_lib.attention_fwd_f32(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), C * T, o.data_ptr(), lse.data_ptr(), rec.data_ptr(),
                            B, C, T, scale, stream)
  hip_lib.attention_bwd_f32(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), C * T, dod.data_ptr(), lse.data_ptr(),
                            rec.data_ptr(), delta.data_ptr(), dq.data_ptr(), 0.0, dk.data_ptr(), 0.0, dv.data_ptr(), 0.0,
                            C * T, B, C, T, scale, stream)
  torch.cuda.synchronize()
  short = {'o': o, 'lse': lse, 'delta': delta, 'dq': dq, 'dk': dk, 'dv': dv}
  for n, t in short.items():
    t = t.cpu()
    err = (long_[n] - t).abs().max().item()
    assert err <= 1e-5 * max(t.abs().max().item(), 1.0 if n == 'lse' else 0.0), f'{n}: {err:.3e}'


def test_attention_long_is_deterministic(hip_lib):
  B, C, T = 2, 128, 1024
  q, k, v, do = inputs(B, C, T, seed=31)
  scale = C ** -0.5
  a = run_long(hip_lib, q, k, v, do, scale, stacked=True)
  b = run_long(hip_lib, q, k, v, do, scale, stacked=True)
  for n in a:
    assert torch.equal(a[n], b[n]), n


def test_attention_long_refuses_unsupported_shapes(hip_lib):
  ok = hip_lib.attention_long_ok
  assert ok(2, 48, 1024) == 0 and ok(2, 512, 1024) == 0 and ok(2, 64, 30) == 0 and ok(1, 64, 16388) == 0
  assert ok(2, 64, 1024) == 1 and ok(1, 64, 16384) == 1
  assert hip_lib.attention_long_ws_bytes(2, 48, 1024) == EUNSUPPORTED
  ws_bytes = int(hip_lib.attention_long_ws_bytes(2, 64, 1024))
  ws = torch.empty(ws_bytes // 4, device='cuda')
  x = torch.zeros(3 * 2 * 512 * 1024 + 4, device='cuda')
  r = torch.zeros(1024, device='cuda')
  fwd = hip_lib.attention_long_fwd_f32.raw

  def call(C, T, bs, base=x.data_ptr()):
    return fwd(base, base, base, bs, x.data_ptr(), r.data_ptr(), r.data_ptr(), 2, C, T, 0.1, ws.data_ptr(), ws_bytes, 0)

  assert call(48, 1024, 48 * 1024) == EUNSUPPORTED
  assert call(512, 1024, 512 * 1024) == EUNSUPPORTED
  assert call(64, 30, 64 * 30) == EUNSUPPORTED
  assert call(64, 16388, 64 * 16388) == EUNSUPPORTED
  assert call(64, 1024, 64 * 1024 + 2) == EUNSUPPORTED             # image stride not a multiple of 4
  assert call(64, 1024, 64 * 1024, base=x.data_ptr() + 4) == EUNSUPPORTED   # q / k / v not 16-byte aligned
  assert fwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), 64 * 1024, x.data_ptr(), r.data_ptr(), r.data_ptr(), 2, 64, 1024,
             0.1, ws.data_ptr(), ws_bytes - 16, 0) == EUNSUPPORTED                   # workspace too small
  d = torch.zeros(2 * 64 * 1024, device='cuda')
  assert hip_lib.attention_long_bwd_f32.raw(x.data_ptr(), x.data_ptr(), x.data_ptr(), 64 * 1024, d.data_ptr(), d.data_ptr(),
                                            r.data_ptr(), r.data_ptr(), r.data_ptr(), d.data_ptr(), 0.0, d.data_ptr(), 0.0,
                                            d.data_ptr(), 0.0, 64 * 1024 + 2, 2, 64, 1024, 0.1, ws.data_ptr(), ws_bytes,
                                            0) == EUNSUPPORTED               # gradient stride not a multiple of 4
