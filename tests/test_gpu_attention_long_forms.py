"""The streaming attention kernels (csrc/attention_long.hip) on every width, length edge and launch form of
tests/_attn_long_cases.py, held per query row and per key column to the float64 bounds of tests/_attn_long_ref.py (the
derivation is there; the numpy model of the arithmetic stays inside half of every bound in
tests/test_attention_long_cases_cpu.py).

Every case runs once through stk_attention_long_fwd_f32 / _bwd_f32 or stk_attention_mh_fwd_f32 / _bwd_f32 with o, lse,
delta, the scale records, the gradient buffers and a workspace of exactly ws_bytes() bytes between sentinels; the workspace
is filled with 0xFF bytes (fp16 NaN: a pad position that split_kernel did not zero would multiply into every score) before
the forward and again before the backward.  Then a second time with another NaN fill: all outputs agree bit for bit.  The
gaps of a padded gradient and the buffer of a NULL gradient keep their bits.  The maximum of each 256-entry scale record is
max |tensor| over the B C T extent exactly (the filler of a padded gap is twice that), do's at rec + 768.  One head through
the MH entries gives the long entries' bits.  Worst err / bound per output are printed with -s
(profiles/attention_long_accuracy.txt)."""
import numpy as np
import pytest
import torch

import _attn_long_cases as lc
import _attn_ref as ar
from _stream_util import Guarded

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', lc.IDS)
def test_attention_long_form_within_float64_bounds(hip_lib, name):
  c = lc.BY_NAME[name]
  want, bnd, _ = lc.reference(name)
  t = lc.inputs(name)
  got = lc.run(hip_lib, c, fill=0xFF)
  again = lc.run(hip_lib, c, fill=0x7E)
  for n in got:
    assert np.array_equal(got[n].view(np.int32), again[n].view(np.int32)), f'{name} {n}: two launches differ'
  if c.entry == 'mh' and c.heads == 1:
    long_ = lc.run(hip_lib, c, entry='long')
    for n in got:
      assert np.array_equal(got[n].view(np.int32), long_[n].view(np.int32)), f'{name} {n}: the MH and the long entry differ'
  for i, n in enumerate(('q', 'k', 'v', 'do')):
    r = got['rec'][i * lc.NPART:(i + 1) * lc.NPART]
    assert np.all(r >= 0), f'{name}: record of {n} holds {r.min()}'
    assert r.max() == np.abs(t[n]).max(), f'{name}: the record of {n} has maximum {r.max()!r}, the tensor {np.abs(t[n]).max()!r}'
  rule = lc.launch_rule(c.B, c.heads, c.C // c.heads, c.T)
  print(f'\n  {name}: grids', ' '.join(f'{k} {v[1]}' for k, v in rule.items()))
  worst = {n: ar.ratio(got[n], want[n], ar.bound_of(bnd, n)).max() for n in lc.checked(c)}
  print('  ATTN_LONG_ACC', name, ' '.join(f'{n}={w:.4f}' for n, w in worst.items()))
  for n in lc.checked(c):
    ar.within(got[n], want[n], ar.bound_of(bnd, n), f'{name} {n}', show=False)
  for i in c.null:
    n = lc.GRAD[i]
    assert np.array_equal(got[n].view(np.int32), t['g0'][i].view(np.int32)), f'{name}: the NULL gradient {n} was touched'


def test_attention_long_forms_refuse_what_they_cannot_run(hip_lib):
  """C = 48 and 512, T = 30 and 16388, a stride that is no multiple of 4 or below C T, misaligned q and d_o, a workspace one
  byte short, and through the MH entry at T = 260 a NULL workspace: refused by the long and the MH entries, and nothing
  written: every output and the workspace stay NaN between their sentinels."""
  dev = 'cuda'
  B, C, T, H = 2, 64, 260, 2
  n = B * 3 * C * T + 64
  x = torch.randn(n, device=dev)
  nan = lambda m: Guarded(np.full(m, np.nan, np.float32), dev)
  nws = int(hip_lib.attention_long_ws_bytes(B, C, T))
  assert nws > 0 and nws == int(hip_lib.attention_mh_ws_bytes(B, C, T, H))
  G = {k: nan(n) for k in ('o', 'dq', 'dk', 'dv')}
  G.update(lse=nan(B * H * T + 64), delta=nan(B * H * T + 64), rec=nan(1024), ws=nan(nws // 4))
  p = {k: g.view.data_ptr() for k, g in G.items()}
  xp = x.data_ptr()
  lo_f, lo_b = hip_lib.attention_long_fwd_f32.raw, hip_lib.attention_long_bwd_f32.raw
  mh_f, mh_b = hip_lib.attention_mh_fwd_f32.raw, hip_lib.attention_mh_bwd_f32.raw

  def fwd(mh, C=C, T=T, bs=None, q=xp, ws=p['ws'], wsb=nws):
    bs = C * T if bs is None else bs
    if mh:
      return mh_f(q, xp, xp, bs, p['o'], p['lse'], p['rec'], B, C, T, H, 0.1, ws, wsb, 0)
    return lo_f(q, xp, xp, bs, p['o'], p['lse'], p['rec'], B, C, T, 0.1, ws, wsb, 0)

  def bwd(mh, C=C, T=T, bs=None, gs=None, do=xp, ws=p['ws'], wsb=nws):
    bs, gs = (C * T if s is None else s for s in (bs, gs))
    if mh:
      return mh_b(xp, xp, xp, bs, xp, do, p['lse'], p['rec'], p['delta'], p['dq'], 0.0, p['dk'], 0.0, p['dv'], 0.0, gs, B, C, T,
                  H, 0.1, ws, wsb, 0)
    return lo_b(xp, xp, xp, bs, xp, do, p['lse'], p['rec'], p['delta'], p['dq'], 0.0, p['dk'], 0.0, p['dv'], 0.0, gs, B, C, T, 0.1,
                ws, wsb, 0)

  U, E = lc.STK_EUNSUPPORTED, lc.STK_EINVAL
  for mh in (False, True):
    w = H if mh else 1
    assert fwd(mh, C=48 * w) == U and bwd(mh, C=48 * w) == U and fwd(mh, C=512 * w) == U and bwd(mh, C=512 * w) == U   # d = 48, 512
    assert fwd(mh, T=16388) == U and bwd(mh, T=16388) == U                                               # T above 16384
    assert fwd(mh, bs=C * T - 4) == U and bwd(mh, bs=C * T - 4) == U and bwd(mh, gs=C * T - 4) == U      # a stride below C T
    assert fwd(mh, bs=C * T + 2) == U and bwd(mh, bs=C * T + 2) == U and bwd(mh, gs=C * T + 2) == U      # no multiple of 4
    assert fwd(mh, q=xp + 4) == U and bwd(mh, do=xp + 4) == U                                            # misaligned
    short = E if mh else U                                                                               # the MH entry: EINVAL
    assert fwd(mh, wsb=nws - 1) == short and bwd(mh, wsb=nws - 1) == short                               # one byte short
    assert fwd(mh, ws=None) == E and bwd(mh, ws=None) == E                                               # NULL workspace
  assert fwd(False, T=30) == U and bwd(False, T=30) == U                                                 # T % 4 (the MH entry: short form)
  assert fwd(True, T=258) == U and bwd(True, T=258) == U
  torch.cuda.synchronize()
  for k, g in G.items():
    g.check(k)
    assert bool(torch.isnan(g.view).all()), f'{k} was written by a refused call'
  for mh in (False, True):                                                                               # and what they do run
    assert fwd(mh, bs=C * T + 28) == lc.STK_OK
    torch.cuda.synchronize()
    assert not torch.isnan(G['o'].view[:B * C * T]).any()
    G['o'].view.fill_(float('nan'))
  torch.cuda.synchronize()
  for k, g in G.items():
    g.check(k)
