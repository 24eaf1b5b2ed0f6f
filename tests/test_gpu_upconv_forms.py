"""csrc/upconv.hip on every launch form (tests/_upconv_cases.py has the cases, the float64 reference, the bound with its
rounding counts and the restated form rules): per case the forward, the data gradient from dy, the data and the weight
gradient from the du it left, the weight gradient from dy -- every element of y, u, du, dx, dw inside k 2^-24 B + 2^-126,
overwritten outputs and both workspaces NaN-prefilled between sentinel guards, the whole sequence twice bit for bit.

Forms with no kernel-level test before this file: the 128 x 128 forward tiles (all three TAPS), the 128 x 128 data-gradient
tiles (K = 3 and K = 1), the 128-wide weight gradient at K = 1, every multi-slab weight gradient with a short last slab,
the FIR kernel at KT = 1 and KT = 3 and with a partial quad in the forward, H = 1 and W = 1.

Worst measured err / bound per output over the cases (MI355X; profiles/upconv_accuracy.txt has every case):
  u 0.509, y 0.373, du 0.999 at KT = 1 (one product, one rounding: the bound is that rounding) and 0.735 / 0.488 / 0.331 at
  KT = 2 / 3 / 4, dx 0.22, dw 0.151, the weight gradient's sums alone 0.714 (a sum of two pixels).
"""
import pytest
import torch

import _upconv_cases as uc
from _stream_util import Guarded

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
  return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize('name', uc.IDS)
def test_every_element_is_inside_its_bound(hip_lib, name):
  dev = torch.device('cuda:0')
  c = uc.BY_NAME[name]
  first = uc.run(hip_lib, c, dev)
  again = uc.run(hip_lib, c, dev)
  for out, t in first.items():
    assert _bits_equal(t, again[out]), f'{name}: {out} differs between two runs on fresh buffers'
  assert _bits_equal(first['du'], first['du2']), f'{name}: du differs between the two entries that fill it'
  want, mag = uc.reference(name)
  bnd = uc.bounds(c, mag)
  k = uc.counts(c)
  # u is the forward's workspace: the chain alone, Cin ((K+1)/2)^2 roundings.  At K = 1 the three other parities are the
  # memset's zeros: B = 0 there and the bound is 2^-126
  worst = {'u': uc.check(c, 'u', first['u'], want['u'],(k['y'] - c.KT * c.KT - 4) * uc.U * mag['u'] + uc.TINY, show=False)}
  for out in uc.OUTPUTS:
    worst[out] = uc.check(c, out, first[out], want[out], bnd[out], show=False)
  worst['dw_du sums'] = uc.check_sums(c, 'dw_du', first['dw_du'], c.a_dw[0], want, mag, show=False)
  worst['dw_dy sums'] = uc.check_sums(c, 'dw_dy', first['dw_dy'], c.a_dw[1], want, mag, show=False)
  print(f'upconv forms {name}: ' + ' '.join(f'{o.replace(" ", "_")} {r:.3g}' for o, r in worst.items()))


def test_bad_arguments_are_refused_without_a_launch(hip_lib):
  """KT = 5 and K = 2 are unsupported, N = 0, a missing dy or fir at du_valid = 0 and a weight-gradient workspace one byte
  short are invalid: the documented code, and no output, du or workspace element is written."""
  dev = torch.device('cuda:0')
  c = uc.BY_NAME['b2_5to6_6x5_k3_t4_p0']
  t = uc.inputs(c.name)
  d = {k: (None if v is None else v.to(dev)) for k, v in t.items()}
  dims = [c.N, c.H, c.W, c.Cin, c.Cout, c.K, c.KT]
  UH, UW = 2 * c.H - 2 + c.K, 2 * c.W - 2 + c.K
  nb_u, nb_wg = int(hip_lib.upconv2d_ws_bytes(0, *dims)), int(hip_lib.upconv2d_ws_bytes(2, *dims))
  nan = lambda *s: torch.full(s, float('nan'))
  G = {n: Guarded(v, dev) for n, v in (('y', nan(c.N, c.Cout, 2 * c.H, 2 * c.W)), ('du', nan(c.N, c.Cout, UH, UW)), ('dx', nan(c.N, c.Cin, c.H, c.W)),
                                       ('dw', nan(c.Cout, c.Cin, c.K, c.K)), ('ws_u', nan(nb_u // 4)), ('ws_wg', nan(nb_wg // 4)))}
  p = lambda v: None if v is None else v.data_ptr()
  y, du, dx, dw, ws_u, ws_wg = (G[n].view for n in ('y', 'du', 'dx', 'dw', 'ws_u', 'ws_wg'))

  def with_dims(**kw):
    names = ['N', 'H', 'W', 'Cin', 'Cout', 'K', 'KT']
    return [kw.get(n, v) for n, v in zip(names, dims)]

  def fwd(dm):
    return hip_lib.upconv2d_fwd_f32.raw(p(d['x']), p(d['w']), p(d['fir']), p(d['bias']), p(d['res']), c.div, p(y), *dm, c.pad0, p(ws_u), nb_u, 0)

  def dgrad(dm, dy=d['dy'], fir=d['fir'], du_valid=0):
    return hip_lib.upconv2d_dgrad_f32.raw(p(dy), p(d['w']), p(fir), p(du), du_valid, p(dx), 0.0, 1.0, *dm, c.pad0, 0)

  def wgrad(dm, dy=d['dy'], fir=d['fir'], du_valid=0, nb=nb_wg):
    return hip_lib.upconv2d_wgrad_f32.raw(p(d['x']), p(dy), p(fir), p(du), du_valid, p(dw), 1.0, *dm, c.pad0, p(ws_wg), nb, 0)

  for entry in (fwd, dgrad, wgrad):
    assert entry(with_dims(KT=5)) == uc.STK_EUNSUPPORTED, entry.__name__
    assert entry(with_dims(K=2)) == uc.STK_EUNSUPPORTED, entry.__name__
    assert entry(with_dims(N=0)) == uc.STK_EINVAL, entry.__name__
  for entry in (dgrad, wgrad):
    assert entry(dims, dy=None) == uc.STK_EINVAL, entry.__name__
    assert entry(dims, fir=None) == uc.STK_EINVAL, entry.__name__
  assert wgrad(dims, nb=nb_wg - 1) == uc.STK_EINVAL
  for q in (0, 1, 2):
    assert hip_lib.upconv2d_ws_bytes(q, *with_dims(KT=5)) < 0 and hip_lib.upconv2d_ws_bytes(q, *with_dims(K=2)) < 0
    assert hip_lib.upconv2d_ws_bytes(q, *with_dims(N=0)) < 0
  torch.cuda.synchronize()
  for n, g in G.items():
    g.check(f'refusals {n}')
    assert bool(torch.isnan(g.view).all()), f'a refused call wrote into {n}'
