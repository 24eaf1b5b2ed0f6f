"""The short-map attention kernels (csrc/attention.hip) on every kernel family and launch form of tests/_attn_cases.py, held
per query row and per key column to the float64 bounds of tests/_attn_ref.py (the derivation is there; the numpy model of
the arithmetic stays inside half of every bound in tests/test_attention_cases_cpu.py).

Every case runs once through stk_attention_fwd_f32 / _bwd_f32 or stk_attention_mh_fwd_f32 / _bwd_f32 with o, lse, delta,
the scale records and the gradient buffers between sentinels, and then a second time: the two runs agree bit for bit.  The
gaps of a padded gradient and the slice of a NULL gradient keep their bits.  The maximum of each 256-entry scale record is
max |tensor| over the B C T extent exactly (the filler of a padded gap is twice that), do's at rec + 768.  Worst err / bound
per output are printed with -s (profiles/attention_accuracy.txt)."""
import numpy as np
import pytest
import torch

import _attn_cases as ac
import _attn_ref as ar
from _stream_util import Guarded

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', ac.IDS)
def test_attention_form_within_float64_bounds(hip_lib, name):
  c = ac.BY_NAME[name]
  want, bnd, _ = ac.reference(name)
  t = ac.inputs(name)
  got = ac.run(hip_lib, c)
  again = ac.run(hip_lib, c)
  for n in got:
    assert np.array_equal(got[n].view(np.int32), again[n].view(np.int32)), f'{name} {n}: two launches differ'
  for i, n in enumerate(('q', 'k', 'v', 'do')):
    r = got['rec'][i * ac.NPART:(i + 1) * ac.NPART]
    assert np.all(r >= 0), f'{name}: record of {n} holds {r.min()}'
    assert r.max() == np.abs(t[n]).max(), f'{name}: the record of {n} has maximum {r.max()!r}, the tensor {np.abs(t[n]).max()!r}'
  print(f'\n  {name}: {ac.family(c)}, grid {ac.grid(c)}')
  worst = {n: ar.ratio(got[n], want[n], ar.bound_of(bnd, n)).max() for n in ac.checked(c)}
  print('  ATTN_ACC', ac.family(c).replace(' ', '_'), name, ' '.join(f'{n}={w:.4f}' for n, w in worst.items()))
  for n in ac.checked(c):
    ar.within(got[n], want[n], ar.bound_of(bnd, n), f'{name} {n}', show=False)
  if c.null is not None:
    n = ('dq', 'dk', 'dv')[c.null]
    assert np.array_equal(got[n].view(np.int32), t['g0'][c.null].view(np.int32)), f'{name}: the NULL gradient {n} was touched'


def test_attention_forms_refuse_what_they_cannot_run(hip_lib):
  """A stride below C T, a stride that is no multiple of 4, a misaligned do, T % 4 != 0, d % 32 != 0: STK_EUNSUPPORTED from
  the single-head and the MH entries, and nothing written: every output stays NaN between its sentinels."""
  dev = 'cuda'
  B, C, T, H = 2, 64, 32, 2
  n = B * 3 * C * T + 64
  x = torch.randn(n, device=dev)
  nan = lambda m: Guarded(np.full(m, np.nan, np.float32), dev)
  G = {k: nan(n) for k in ('o', 'dq', 'dk', 'dv')}
  G.update(lse=nan(B * H * T + 64), delta=nan(B * H * T + 64), rec=nan(1024))
  ws = torch.zeros(4, device=dev)
  p = {k: g.view.data_ptr() for k, g in G.items()}
  xp = x.data_ptr()
  sh_f, sh_b = hip_lib.attention_fwd_f32.raw, hip_lib.attention_bwd_f32.raw
  mh_f, mh_b = hip_lib.attention_mh_fwd_f32.raw, hip_lib.attention_mh_bwd_f32.raw

  def fwd(mh, C=C, T=T, bs=None, q=xp):
    bs = C * T if bs is None else bs
    if mh:
      return mh_f(q, xp, xp, bs, p['o'], p['lse'], p['rec'], B, C, T, H, 0.1, ws.data_ptr(), 0, 0)
    return sh_f(q, xp, xp, bs, p['o'], p['lse'], p['rec'], B, C, T, 0.1, 0)

  def bwd(mh, C=C, T=T, bs=None, gs=None, do=xp):
    bs, gs = (C * T if s is None else s for s in (bs, gs))
    if mh:
      return mh_b(xp, xp, xp, bs, xp, do, p['lse'], p['rec'], p['delta'], p['dq'], 0.0, p['dk'], 0.0, p['dv'], 0.0, gs, B, C, T,
                  H, 0.1, ws.data_ptr(), 0, 0)
    return sh_b(xp, xp, xp, bs, do, p['lse'], p['rec'], p['delta'], p['dq'], 0.0, p['dk'], 0.0, p['dv'], 0.0, gs, B, C, T, 0.1, 0)

  U = ac.STK_EUNSUPPORTED
  for mh in (False, True):
    assert fwd(mh, bs=C * T - 4) == U and bwd(mh, bs=C * T - 4) == U and bwd(mh, gs=C * T - 4) == U      # a stride below C T
    assert fwd(mh, bs=C * T + 6) == U and bwd(mh, bs=C * T + 6) == U and bwd(mh, gs=C * T + 6) == U      # no multiple of 4
    assert bwd(mh, do=xp + 4) == U and fwd(mh, q=xp + 8) == U                                            # misaligned
    assert fwd(mh, T=30) == U and bwd(mh, T=30) == U                                                     # T % 4
    d_bad = 48 * (H if mh else 1)                                                                        # d = 48
    assert fwd(mh, C=d_bad) == U and bwd(mh, C=d_bad) == U
    torch.cuda.synchronize()
    for k, g in G.items():
      assert bool(torch.isnan(g.view).all()), f'{k} was written by a refused call (mh={mh})'
    assert fwd(mh, bs=C * T + 28) == ac.STK_OK                                                           # and what they do run
    torch.cuda.synchronize()
    assert not torch.isnan(G['o'].view[:B * C * T]).any()
    for k in ('o', 'lse', 'rec'):
      G[k].view.fill_(float('nan'))
  torch.cuda.synchronize()
  for k, g in G.items():
    g.check(k)
    assert bool(torch.isnan(g.view).all()), f'{k} was written by a refused call'
