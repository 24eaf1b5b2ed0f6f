"""stk_superres_f32 and stk_block_mean_f32 (include/stk_superres.h, csrc/superres.hip) through ctypes against the float64
restatement of tests/_superres_ref.py.

The bound is derived, not tuned: |got - want| <= k 2^-24 B per element, B = |x| + blockmean|x| + |a||low| + |s||z| / r
(_superres_ref.magnitude).  The longest rounding path of stk_superres_f32 runs from an element of x: the d additions of the
block sum, the subtraction known - m_x, the final addition x + delta; 1/P and s/r are exact scalings, and the path from low
(a low, + noise, - m_x, + x) is shorter.  Two units of margin: k = d + 4.  stk_block_mean_f32 has the d additions alone:
k = d + 2.  d is the figure of the kernel's header comment, (r - 1) + log2 r = 2, 5, 10, 19 for r = 2, 4, 8, 16 on both of its
paths (_superres_ref.DEPTH); it can never exceed P - 1.

Worst measured error over the cases below, in units of 2^-24 B (MI355X): 1.88 for stk_superres_f32, 1.69 for
stk_block_mean_f32.
"""
import functools
import itertools

import pytest
import torch

import _stream_util
import _superres_ref as R
from _stream_util import place
from _util import call

pytestmark = pytest.mark.gpu

CASES = [((2, 3, 16, 16), 2), ((2, 3, 16, 16), 4), ((2, 3, 16, 16), 8), ((2, 3, 16, 16), 16),     # every factor; W = r at r = 16
         ((1, 3, 16, 16), 8),                          # 24 items: a partly filled wave around the cross-lane step
         ((3, 1, 8, 24), 4), ((3, 1, 8, 24), 8),       # W not a power of two, odd plane count
         ((1, 2, 4, 6), 2),                            # W % 4 = 2: the scalar path
         ((5, 3, 32, 32), 4)]                          # more than one 256-thread block
case_id = lambda c: 'x'.join(map(str, c[0])) + f'-r{c[1]}'
within = functools.partial(_stream_util.within, show=True)      # every comparison prints its worst ratio


def _operands(shape, r, seed):
  N, C, H, W = shape
  g = torch.Generator().manual_seed(seed)
  lowshape = (N, C, H // r, W // r)
  return dict(x=torch.randn(shape, generator=g), low=torch.randn(lowshape, generator=g), z=torch.randn(lowshape, generator=g),
              a=torch.rand(N, generator=g) + 0.25, s=torch.rand(N, generator=g) * 3 + 0.05)


def _run(lib, o, r, dev, use_z, use_mean, inplace, one_in):
  """One launch on fresh copies of the operands -> (x_out, x_mean or None)."""
  N, C, H, W = o['x'].shape
  xin = place(o['x'], dev, one_in)
  low, z = place(o['low'], dev, one_in), place(o['z'], dev, one_in) if use_z else None
  out = xin if inplace else torch.full(o['x'].shape, float('nan'), device=dev)
  mean = torch.full(o['x'].shape, float('nan'), device=dev) if use_mean else None
  call(lib, 'superres_f32', xin, low, z, o['a'].to(dev), o['s'].to(dev), out, mean, N, C, H, W, r)
  return out, mean


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_matches_float64(hip_lib, case):
  shape, r = case
  dev = torch.device('cuda:0')
  o = _operands(shape, r, seed=sum(shape) * 7 + r)
  f = {k: v.double() for k, v in o.items()}
  k = R.DEPTH[r] + 4
  ref = {use_z: (R.restate(f['x'], f['low'], f['z'] if use_z else None, f['a'], f['s'], r),
                 R.magnitude(f['x'], f['low'], f['z'] if use_z else None, f['a'], f['s'], r)) for use_z in (True, False)}
  worst, first = 0.0, {}
  for use_z, use_mean, inplace, one_in in itertools.product((True, False), (True, False), (False, True), (False, True)):
    want, mag = ref[use_z]
    out, mean = _run(hip_lib, o, r, dev, use_z, use_mean, inplace, one_in)
    what = f'superres {shape} r={r} z={use_z} inplace={inplace} one_in={one_in}'
    worst = max(worst, within(out, want[0], mag, k, what + ' x_out'))
    if use_mean:
      worst = max(worst, within(mean, want[1], mag, k, what + ' x_mean'))
      if not use_z:
        assert torch.equal(out, mean), what + ': z == NULL must give x_out == x_mean bit for bit'
    # one fixed summation order: in place or not, with or without x_mean, on the 16-byte and on the scalar path
    assert torch.equal(out.cpu(), first.setdefault(use_z, out.cpu())), what + ': bits differ from the first run'
    if use_mean:
      assert torch.equal(mean.cpu(), first.setdefault(('mean', use_z), mean.cpu())), what + ': x_mean bits differ'
  again, _ = _run(hip_lib, o, r, dev, True, True, False, False)
  assert torch.equal(again.cpu(), first[True]), 'two runs differ'
  print(f'superres {shape} r={r}: worst over the case {worst:.2f} x 2^-24 B (bound {k})')


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_block_mean_matches_float64(hip_lib, case):
  shape, r = case
  N, C, H, W = shape
  dev = torch.device('cuda:0')
  x = _operands(shape, r, seed=sum(shape) * 11 + r)['x']
  want, mag = R.block_mean(x.double(), r), R.block_mean(x.double().abs(), r)
  k = R.DEPTH[r] + 2
  outs = []
  for one_in in (False, True):
    xin = place(x, dev, one_in)
    out = place(torch.full(want.shape, float('nan')), dev, one_in)
    call(hip_lib, 'block_mean_f32', xin, out, N * C, H, W, r)
    within(out, want, mag, k, f'block_mean {shape} r={r} one_in={one_in}')
    outs.append(out.cpu())
  assert torch.equal(outs[0], outs[1]), 'the 16-byte and the scalar path sum in different orders'
  # the mean stk_superres_f32 takes: with a = 1 and no noise, low = block_mean(x) leaves x as it is up to x + (m - m) = x
  low = outs[0].to(dev)
  one = torch.ones(N, device=dev)
  xin, out = x.to(dev), torch.full(shape, float('nan'), device=dev)
  call(hip_lib, 'superres_f32', xin, low, None, one, one, out, None, N, C, H, W, r)
  assert torch.equal(out, xin), 'stk_block_mean_f32 is not the mean stk_superres_f32 subtracts'


def test_unsupported_arguments_are_refused_and_write_nothing(hip_lib):
  dev = torch.device('cuda:0')
  stream = lambda: torch.cuda.current_stream().cuda_stream

  def refused(dims, r):
    """rc of both entries on small real buffers with the claimed dims; outputs prefilled with 7.0 must stay."""
    t = [torch.randn(2, 3, 16, 16, device=dev) for _ in range(3)]
    ab = torch.ones(2, device=dev)
    out, mean = torch.full((2, 3, 16, 16), 7.0, device=dev), torch.full((2, 3, 16, 16), 7.0, device=dev)
    N, C, H, W = dims
    rc = hip_lib.superres_f32.raw(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), ab.data_ptr(), ab.data_ptr(),
                                  out.data_ptr(), mean.data_ptr(), N, C, H, W, r, stream())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((mean == 7.0).all())
    rc2 = hip_lib.block_mean_f32.raw(t[0].data_ptr(), out.data_ptr(), N * C, H, W, r, stream())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    return rc, rc2

  assert refused((2, 3, 16, 16), 3) == (-3, -3)
  assert refused((2, 3, 16, 16), 32) == (-3, -3)
  assert refused((2, 3, 32, 32), 32) == (-3, -3)                 # r = 32 even where it divides
  assert refused((2, 3, 12, 16), 8) == (-3, -3)                  # H not a multiple of r
  assert refused((2, 3, 16, 12), 8) == (-3, -3)                  # W not a multiple of r
  assert refused((2 ** 15, 2 ** 10, 8, 8), 4) == (-3, -3)        # 2^31 elements
  assert refused((1, 1, 2 ** 16, 2 ** 15), 2) == (-3, -3)
  assert refused((2, 3, 16, 16), 0) == (-3, -3)
