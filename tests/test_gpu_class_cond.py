"""The entries of include/stk_cond.h (csrc/cond.hip) through ctypes against the float64 restatement of tests/_cond_ref.py, on
the device, element by element, each held to k u B (u = 2^-24, B the expression on absolute values):

  forward embed    y = t + e: one rounding, k = 1
  backward embed   gt: beta = 0 bit-equal to gy; beta = 1 one rounding, k = 1
                   table gradient: n_c additions onto the value already there, k = n_c (the class's count in the batch; any
                   order of n_c additions meets it); rows of absent classes bit-identical; two launches bit-identical
  combine          c + w (c - u): the difference, the product and the sum round once each, plus one unit for the second-order
                   terms, k = 4; w = 0 bit-equal to c

Sizes: B in {1, 3, 5} with C in {1, 3}, widths 6 (no multiple of 4: the scalar path), 64 and 384 (more than one block of
256 lanes on the scalar path); n in {5, 64, 768} for the combination.  Each with aligned operands and with operands entered
one element into their buffers (the scalar path at a width that would otherwise take 16-byte accesses).  The index vectors
hold the last real class, the null row and a repeat as soon as B allows it.
"""
import math

import pytest
import torch

import _cond_ref as R
from _stream_util import case_id, place, within

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = -1, -3
BATCHES, CLASSES, WIDTHS = (1, 3, 5), (1, 3), (6, 64, 384)
WEIGHTS = (0.0, -1.0, 1.5, 7.5)


def _stream():
  return torch.cuda.current_stream().cuda_stream


def _indices(B, C):
  """The last real class, the null row, the last real class again, class 0, the null row again: the first B of them."""
  return torch.tensor([C - 1, C, C - 1, 0, C][:B], dtype=torch.float32)


def _operands(B, C, D, seed):
  g = torch.Generator().manual_seed(seed)
  rn = lambda *s: torch.randn(*s, generator=g)
  return dict(t=rn(B, D), table=rn(C + 1, D), gy=rn(B, D), gt=rn(B, D), gtable=rn(C + 1, D), idx=_indices(B, C))


@pytest.fixture(scope='module')
def cases():
  """Host operands per (B, C, D): computed once, never written."""
  return {(B, C, D): _operands(B, C, D, seed=100 * B + 10 * C + D) for B in BATCHES for C in CLASSES for D in WIDTHS}


@pytest.fixture(scope='module')
def lib(hip_lib):
  assert hip_lib.has_cond is True
  return hip_lib


def _fwd(lib, dev, t, table, idx, one_in, in_place=False):
  B, D = t.shape
  C = table.shape[0] - 1
  td, ed, idx_d = place(t, dev, one_in), place(table, dev, one_in), idx.to(dev)
  y = td if in_place else place(torch.full((B, D), float('nan')), dev, one_in)
  lib.class_embed_fwd_f32(td.data_ptr(), ed.data_ptr(), idx_d.data_ptr(), y.data_ptr(), B, C, D, _stream())
  return y


def _bwd(lib, dev, C, gy, idx, gt, beta, gtable, one_in):
  """-> (gt', gtable') device tensors; gt / gtable None: that output is not asked for."""
  B, D = gy.shape
  gyd, idx_d = place(gy, dev, one_in), idx.to(dev)
  gtd = place(gt, dev, one_in) if gt is not None else None
  ged = place(gtable, dev, one_in) if gtable is not None else None
  lib.class_embed_bwd_f32(gyd.data_ptr(), idx_d.data_ptr(), gtd.data_ptr() if gtd is not None else None, beta,
                          ged.data_ptr() if ged is not None else None, B, C, D, _stream())
  return gtd, ged


@pytest.mark.parametrize('one_in', [False, True], ids=case_id)
@pytest.mark.parametrize('D', WIDTHS)
def test_forward_embed(lib, cases, D, one_in):
  dev = torch.device('cuda:0')
  for B in BATCHES:
    for C in CLASSES:
      op = cases[(B, C, D)]
      want, mag = R.embed_fwd(op['t'], op['table'], op['idx'])
      y = _fwd(lib, dev, op['t'], op['table'], op['idx'], one_in)
      within(y, want, mag, 1, f'y B={B} C={C} D={D}')
      assert torch.equal(_fwd(lib, dev, op['t'], op['table'], op['idx'], one_in, in_place=True), y), 'y written over t'


@pytest.mark.parametrize('one_in', [False, True], ids=case_id)
def test_forward_index_out_of_range_takes_the_null_row(lib, cases, one_in):
  """The safe behaviour, not a fault: whatever is no integer in [0, C] reads row C."""
  dev = torch.device('cuda:0')
  bad = [-1.0, 4.0, 0.5, float('nan'), float('inf'), -float('inf'), 1e9, -0.5]
  for D in WIDTHS:
    g = torch.Generator().manual_seed(D)
    t, table = torch.randn(len(bad), D, generator=g), torch.randn(4, D, generator=g)
    idx = torch.tensor(bad, dtype=torch.float32)
    assert R.class_row(idx, 3).tolist() == [3] * len(bad)
    y = _fwd(lib, dev, t, table, idx, one_in)
    null = _fwd(lib, dev, t, table, torch.full((len(bad),), 3.0), one_in)
    assert torch.equal(y, null)
    want, mag = R.embed_fwd(t, table, idx)
    within(y, want, mag, 1, f'null row D={D}')


@pytest.mark.parametrize('one_in', [False, True], ids=case_id)
@pytest.mark.parametrize('D', WIDTHS)
def test_backward_embed(lib, cases, D, one_in):
  dev = torch.device('cuda:0')
  for B in BATCHES:
    for C in CLASSES:
      op = cases[(B, C, D)]
      gy, idx, gt0, g0 = op['gy'], op['idx'], op['gt'], op['gtable']
      what = f'B={B} C={C} D={D}'
      # beta = 0: an exact copy, and gt is not read (NaN there must not show)
      gt, ge = _bwd(lib, dev, C, gy, idx, torch.full_like(gt0, float('nan')), 0.0, g0, one_in)
      assert torch.equal(gt.cpu(), gy), f'gt beta=0 {what}'
      want, mag, count = R.embed_bwd_table(gy, idx, g0)
      k = count.double()[:, None].expand_as(mag)
      within(ge, want, k * mag, 1, f'gtable {what}')
      absent = count == 0
      assert torch.equal(ge.cpu()[absent], g0[absent]), f'rows of absent classes {what}'
      # beta = 1: one rounding; the table gradient is the same bits on a second launch
      gt1, ge1 = _bwd(lib, dev, C, gy, idx, gt0, 1.0, g0, one_in)
      want_t, mag_t = R.embed_bwd_gt(gy, gt0, 1)
      within(gt1, want_t, mag_t, 1, f'gt beta=1 {what}')
      assert torch.equal(ge1, ge), f'two launches {what}'
      # either output alone
      assert torch.equal(_bwd(lib, dev, C, gy, idx, gt0, 1.0, None, one_in)[0], gt1)
      assert torch.equal(_bwd(lib, dev, C, gy, idx, None, 0.0, g0, one_in)[1], ge)


@pytest.mark.parametrize('one_in', [False, True], ids=case_id)
@pytest.mark.parametrize('n', [5, 64, 3 * 16 * 16])
def test_cfg_combine(lib, n, one_in):
  dev = torch.device('cuda:0')
  g = torch.Generator().manual_seed(n)
  c, u = torch.randn(n, generator=g), torch.randn(n, generator=g)
  for w in WEIGHTS:
    assert float(torch.tensor(w, dtype=torch.float32)) == w
    want, mag = R.cfg_combine(c, u, w)
    cd, ud = place(c, dev, one_in), place(u, dev, one_in)
    out = place(torch.full((n,), float('nan')), dev, one_in)
    lib.cfg_combine_f32(cd.data_ptr(), ud.data_ptr(), w, out.data_ptr(), n, _stream())
    within(out, want, mag, 4, f'out n={n} w={w}')
    assert torch.equal(cd.cpu(), c) and torch.equal(ud.cpu(), u), 'an operand was written'
    lib.cfg_combine_f32(cd.data_ptr(), ud.data_ptr(), w, cd.data_ptr(), n, _stream())      # in place on cond
    assert torch.equal(cd, out), f'in place differs from out of place, n={n} w={w}'
    if w == 0.0:
      assert torch.equal(out.cpu(), c), 'w = 0 is not cond bit for bit'


def test_refusals_launch_nothing(lib):
  dev = torch.device('cuda:0')
  a = torch.zeros(8, device=dev)
  p, s = a.data_ptr(), _stream()
  fwd, bwd, comb = lib.class_embed_fwd_f32.raw, lib.class_embed_bwd_f32.raw, lib.cfg_combine_f32.raw
  assert fwd(None, p, p, p, 1, 1, 4, s) == EINVAL and fwd(p, p, p, p, 0, 1, 4, s) == EINVAL
  assert fwd(p, p, p, p, 1, 0, 4, s) == EINVAL and fwd(p, p, p, p, 1 << 16, 1, 1 << 15, s) == EUNSUPPORTED
  assert bwd(p, p, None, 0.0, None, 1, 1, 4, s) == EINVAL and bwd(p, p, p, 0.5, p, 1, 1, 4, s) == EINVAL
  assert bwd(p, p, p, 1.0, p, 1, 1 << 16, 1 << 15, s) == EUNSUPPORTED
  assert comb(p, p, math.inf, p, 4, s) == EINVAL and comb(p, p, math.nan, p, 4, s) == EINVAL
  assert comb(p, None, 1.0, p, 4, s) == EINVAL and comb(p, p, 1.0, p, 0, s) == EINVAL
  assert comb(p, p, 1.0, p, 1 << 31, s) == EUNSUPPORTED
  torch.cuda.synchronize()
  assert float(a.abs().sum()) == 0.0
