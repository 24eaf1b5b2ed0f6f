"""The multi-head attention entries (include/stk_attention_mh.h; csrc/attention.hip for T <= 256, csrc/attention_long.hip
above) against the float64 restatement of tests/_mh_ref.py.

Bounds as tests/test_gpu_attention_long.py: 1e-4 of max |ref| for o, dq, dk, dv and delta, 1e-5 max(1, max |lse|) for lse.
Every shape runs with three separate tensors and with the stacked [B, 3C, T] projection and its gradient."""
import pytest
import torch

import _mh_ref
from _util import rnd

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3
NAMES = ('o', 'lse', 'delta', 'dq', 'dk', 'dv')


def run_mh(lib, q, k, v, do, heads, stacked=False, beta=0.0, g0=None, want=(True, True, True), scale=None, dev='cuda'):
  """Forward + backward through the mh entries; g0: initial dq, dk, dv (accumulated into with beta); want: which of
  dq, dk, dv are asked for (the others are passed as NULL and come back as their initial values)."""
  B, C, T = q.shape
  scale = (C // heads) ** -0.5 if scale is None else scale
  ws_bytes = int(lib.attention_mh_ws_bytes(B, C, T, heads))
  assert ws_bytes >= 0, ws_bytes
  ws = torch.empty(ws_bytes // 4 + 4, device=dev)
  o, lse, delta = (torch.zeros(B, C, T, device=dev), torch.zeros(B, heads, T, device=dev),
                   torch.zeros(B, heads, T, device=dev))
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
  outs = [p if w else None for p, w in zip(outs, want)]
  d_o = do.to(dev)
  stream = torch.cuda.current_stream().cuda_stream
  lib.attention_mh_fwd_f32(ins[0], ins[1], ins[2], bs, o.data_ptr(), lse.data_ptr(), rec.data_ptr(), B, C, T, heads, scale,
                           ws.data_ptr(), ws_bytes, stream)
  lib.attention_mh_bwd_f32(ins[0], ins[1], ins[2], bs, o.data_ptr(), d_o.data_ptr(), lse.data_ptr(), rec.data_ptr(),
                           delta.data_ptr(), outs[0], beta, outs[1], beta, outs[2], beta, bs, B, C, T, heads, scale,
                           ws.data_ptr(), ws_bytes, stream)
  torch.cuda.synchronize()
  if stacked:
    dq, dk, dv = (g[:, i * C:(i + 1) * C].contiguous() for i in range(3))
  else:
    dq, dk, dv = keep[3:]
  return {n: t.cpu() for n, t in zip(NAMES, (o, lse, delta, dq, dk, dv))}


def check(got, ref, what, rtol=1e-4, lse_tol=1e-5, names=('o', 'dq', 'dk', 'dv', 'delta')):
  msgs = []
  for n in names:
    err = (got[n].double() - ref[n]).abs().max().item()
    bound = rtol * ref[n].abs().max().item()
    msgs.append(f'{n} {err / max(ref[n].abs().max().item(), 1e-300):.2e}')
    assert err <= bound, f'{what}: {n} max err {err:.3e} > {bound:.3e}'
  err = (got['lse'].double() - ref['lse']).abs().max().item()
  bound = lse_tol * max(1.0, ref['lse'].abs().max().item())
  print(f'{what}: rel errors', ', '.join(msgs), f'lse abs {err:.2e}')
  assert err <= bound, f'{what}: lse max err {err:.3e} > {bound:.3e}'


def inputs(B, C, T, mags=(1., 1., 1., 1.), seed=1):
  return [rnd(B, C, T, seed=seed + i) * m for i, m in enumerate(mags)]


_REF = {}


def reference(B, C, heads, T, mags=(1., 1., 1., 1.), seed=1):
  """(inputs, float64 results) of a case, computed once and shared (nobody writes to them)."""
  key = (B, C, heads, T, mags, seed)
  if key not in _REF:
    x = inputs(B, C, T, mags, seed)
    _REF[key] = (x, _mh_ref.attention_with_grads(*x, heads))
  return _REF[key]


# (B, C, heads, T)
SHORT = [
  (2, 64, 2, 16),
  (3, 96, 3, 36),       # odd head count, ragged tile
  (2, 128, 2, 64),
  (2, 256, 8, 132),     # TK = 256, ragged
  (1, 256, 4, 256),     # the shipped block with heads of 64: the straight-line path, (block, half tile) per wave
  (2, 512, 2, 64),      # C above 256
]
STREAMING = [
  (2, 128, 4, 320),
  (2, 192, 3, 260),
  (1, 64, 2, 1024),
]
# further shapes: the other straight-line instantiations (d = 32, 128, 256) and a ragged T above one tile at d = 64
EXTRA = [
  (1, 256, 8, 256),
  (1, 256, 2, 256),
  (1, 512, 2, 256),
  (2, 128, 2, 200),
]


@pytest.mark.parametrize('stacked', [False, True], ids=['separate', 'stacked'])
@pytest.mark.parametrize('shape', SHORT + STREAMING + EXTRA, ids=lambda s: f'B{s[0]}C{s[1]}h{s[2]}T{s[3]}')
def test_attention_mh_matches_float64(hip_lib, shape, stacked):
  B, C, heads, T = shape
  assert hip_lib.attention_mh_ok(B, C, T, heads) == 1
  (q, k, v, do), ref = reference(*shape)
  check(run_mh(hip_lib, q, k, v, do, heads, stacked=stacked), ref, f'{shape} stacked={stacked}')


@pytest.mark.parametrize('shape', [(2, 128, 2, 64), (1, 256, 4, 256), (2, 128, 4, 320)], ids=str)
def test_attention_mh_accumulates_with_beta_1(hip_lib, shape):
  B, C, heads, T = shape
  (q, k, v, do), ref = reference(*shape)
  g0 = [rnd(B, C, T, seed=9 + i) * 0.1 for i in range(3)]
  want = dict(ref)
  for i, n in enumerate(('dq', 'dk', 'dv')):
    want[n] = ref[n] + g0[i].double()
  for stacked in (False, True):
    check(run_mh(hip_lib, q, k, v, do, heads, stacked=stacked, beta=1.0, g0=g0), want, f'{shape} beta=1 stacked={stacked}')


@pytest.mark.parametrize('shape', [(2, 128, 2, 64), (1, 256, 4, 256), (2, 128, 4, 320), (2, 128, 1, 64),
                                   (2, 64, 1, 320)], ids=str)
def test_attention_mh_null_gradients(hip_lib, shape):
  """Each gradient NULL in turn: the other two are those of the full call bit for bit, the missing one is not touched."""
  B, C, heads, T = shape
  (q, k, v, do), ref = reference(*shape)
  g0 = [torch.full((B, C, T), 7.0 + i) for i in range(3)]
  full = run_mh(hip_lib, q, k, v, do, heads, g0=g0)
  for skip in range(3):
    want = tuple(i != skip for i in range(3))
    got = run_mh(hip_lib, q, k, v, do, heads, g0=g0, want=want)
    for i, n in enumerate(('dq', 'dk', 'dv')):
      assert torch.equal(got[n], g0[i] if i == skip else full[n]), (skip, n)
    assert torch.equal(got['o'], full['o']) and torch.equal(got['lse'], full['lse'])
  check(full, ref, f'{shape} full')


@pytest.mark.parametrize('shape', [(2, 128, 2, 64), (1, 256, 4, 256), (2, 128, 4, 320)], ids=str)
def test_attention_mh_magnitudes_far_apart(hip_lib, shape):
  """One power-of-two scale per tensor: q, k, v, dO of magnitudes 3e3, 2e-3, 5e-4, 1e-6."""
  B, C, heads, T = shape
  (q, k, v, do), ref = reference(*shape, mags=(3e3, 2e-3, 5e-4, 1e-6))
  check(run_mh(hip_lib, q, k, v, do, heads), ref, f'{shape} magnitudes')


@pytest.mark.parametrize('shape', [(2, 128, 2, 64), (1, 256, 4, 256), (2, 128, 4, 320)], ids=str)
def test_attention_mh_is_deterministic(hip_lib, shape):
  B, C, heads, T = shape
  (q, k, v, do), _ = reference(*shape)
  a = run_mh(hip_lib, q, k, v, do, heads, stacked=True)
  b = run_mh(hip_lib, q, k, v, do, heads, stacked=True)
  for n in a:
    assert torch.equal(a[n], b[n]), n


def _single_head(lib, q, k, v, do, scale, dev='cuda'):
  """The single-head entries (short for T <= 256, streaming above) on contiguous [B, C, T] tensors."""
  B, C, T = q.shape
  o, lse, delta, rec = (torch.zeros(B, C, T, device=dev), torch.zeros(B, T, device=dev), torch.zeros(B, T, device=dev),
                        torch.zeros(1024, device=dev))
  qd, kd, vd, dod = (t.contiguous().to(dev) for t in (q, k, v, do))
  dq, dk, dv = (torch.zeros(B, C, T, device=dev) for _ in range(3))
  stream = torch.cuda.current_stream().cuda_stream
  if T <= 256:
    lib.attention_fwd_f32(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), C * T, o.data_ptr(), lse.data_ptr(), rec.data_ptr(),
                          B, C, T, scale, stream)
    lib.attention_bwd_f32(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), C * T, dod.data_ptr(), lse.data_ptr(), rec.data_ptr(),
                          delta.data_ptr(), dq.data_ptr(), 0.0, dk.data_ptr(), 0.0, dv.data_ptr(), 0.0, C * T, B, C, T, scale,
                          stream)
  else:
    ws_bytes = int(lib.attention_long_ws_bytes(B, C, T))
    ws = torch.empty(ws_bytes // 4 + 4, device=dev)
    lib.attention_long_fwd_f32(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), C * T, o.data_ptr(), lse.data_ptr(),
                               rec.data_ptr(), B, C, T, scale, ws.data_ptr(), ws_bytes, stream)
    lib.attention_long_bwd_f32(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), C * T, o.data_ptr(), dod.data_ptr(),
                               lse.data_ptr(), rec.data_ptr(), delta.data_ptr(), dq.data_ptr(), 0.0, dk.data_ptr(), 0.0,
                               dv.data_ptr(), 0.0, C * T, B, C, T, scale, ws.data_ptr(), ws_bytes, stream)
  torch.cuda.synchronize()
  return {n: t.cpu() for n, t in zip(NAMES, (o, lse, delta, dq, dk, dv))}


@pytest.mark.parametrize('shape', [(2, 128, 1, 64), (1, 256, 1, 256), (2, 64, 1, 1024)], ids=str)
def test_one_head_through_the_mh_entries_is_the_single_head_entry(hip_lib, shape):
  B, C, heads, T = shape
  q, k, v, do = inputs(B, C, T, seed=21)
  mh = run_mh(hip_lib, q, k, v, do, 1)
  one = _single_head(hip_lib, q, k, v, do, C ** -0.5)
  for n in NAMES:
    assert torch.equal(mh[n].reshape(one[n].shape), one[n]), n


@pytest.mark.parametrize('shape', [(2, 128, 2, 64), (3, 96, 3, 36), (1, 256, 4, 256), (1, 256, 8, 256), (2, 512, 2, 64), (2, 128, 4, 320)],
                         ids=str)
def test_heads_agree_with_the_single_head_entry_on_the_head_view(hip_lib, shape):
  """[B, C, T] contiguous IS [B h, d, T]: the single-head entries on that view, with the head's scale, compute the same
  attention without any head offset.  1e-5 of max |.|, the bound of the long-against-short test."""
  B, C, heads, T = shape
  d = C // heads
  (q, k, v, do), _ = reference(*shape)
  mh = run_mh(hip_lib, q, k, v, do, heads)
  one = _single_head(hip_lib, *(t.reshape(B * heads, d, T) for t in (q, k, v, do)), d ** -0.5)
  for n in NAMES:
    a, b = mh[n].reshape(one[n].shape), one[n]
    err = (a - b).abs().max().item()
    assert err <= 1e-5 * max(b.abs().max().item(), 1.0 if n == 'lse' else 0.0), f'{n}: {err:.3e}'


def test_attention_mh_refusals(hip_lib):
  ok, wsb = hip_lib.attention_mh_ok, hip_lib.attention_mh_ws_bytes
  assert ok(2, 100, 64, 3) == 0 and ok(2, 96, 64, 2) == 0 and ok(2, 64, 64, 4) == 0 and ok(2, 64, 30, 2) == 0
  assert ok(2, 128, 64, 2) == 1 and ok(2, 1024, 64, 4) == 1 and ok(1, 64, 16384, 2) == 1 and ok(1, 64, 16388, 2) == 0
  assert wsb(2, 100, 64, 3) == EINVAL and wsb(2, 96, 64, 2) == EUNSUPPORTED
  x = torch.zeros(3 * 2 * 128 * 320 + 8, device='cuda')
  r = torch.zeros(2048, device='cuda')
  ws_bytes = int(wsb(2, 128, 320, 4))
  assert ws_bytes > 0 and wsb(2, 128, 64, 4) == 0
  ws = torch.empty(ws_bytes // 4, device='cuda')
  fwd, bwd = hip_lib.attention_mh_fwd_f32.raw, hip_lib.attention_mh_bwd_f32.raw

  def f(C, T, heads, bs=None, base=None, wsn=ws_bytes):
    base = x.data_ptr() if base is None else base
    return fwd(base, base, base, C * T if bs is None else bs, x.data_ptr(), r.data_ptr(), r.data_ptr(), 2, C, T, heads, 0.1,
               ws.data_ptr(), wsn, 0)

  assert f(100, 64, 3) == EINVAL                                   # C % heads != 0
  assert f(96, 64, 2) == EUNSUPPORTED                              # d = 48
  assert f(64, 64, 4) == EUNSUPPORTED                              # d = 16
  assert f(64, 30, 2) == EUNSUPPORTED                              # T = 30
  assert f(128, 64, 2, base=x.data_ptr() + 4) == EUNSUPPORTED      # misaligned, short form
  assert f(128, 320, 4, base=x.data_ptr() + 4) == EUNSUPPORTED     # misaligned, streaming form
  assert f(128, 64, 2, bs=128 * 64 + 2) == EUNSUPPORTED            # image stride not a multiple of 4
  assert f(128, 320, 4, wsn=ws_bytes - 16) == EINVAL               # workspace too small
  d = torch.zeros(2 * 128 * 320, device='cuda')

  def b(C, T, heads, gs=None, wsn=ws_bytes):
    return bwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), C * T, d.data_ptr(), d.data_ptr(), r.data_ptr(), r.data_ptr(),
               r.data_ptr(), d.data_ptr(), 0.0, d.data_ptr(), 0.0, d.data_ptr(), 0.0, C * T if gs is None else gs, 2, C, T,
               heads, 0.1, ws.data_ptr(), wsn, 0)

  assert b(100, 64, 3) == EINVAL and b(96, 64, 2) == EUNSUPPORTED and b(64, 30, 2) == EUNSUPPORTED
  assert b(128, 64, 2, gs=128 * 64 + 2) == EUNSUPPORTED and b(128, 320, 4, gs=128 * 320 + 2) == EUNSUPPORTED
  assert b(128, 320, 4, wsn=ws_bytes - 16) == EINVAL
  torch.cuda.synchronize()
