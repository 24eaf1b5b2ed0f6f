"""stk_impute_f32 (include/stk_impute.h, csrc/impute.hip) through ctypes against a float64 restatement of its formulas.

The bound is derived, not tuned.  Every output element is a sum of rounded products: at most 9 for the colour mix, 4 for the
blend, 9 for the return to RGB.  Standard forward analysis bounds the error of such an expression by gamma_k * B, where B is
the same expression evaluated on absolute values (|x|, |data|, |z|, |M|, |inv M|, |a|, |s|; m and 1 - m are not negative)
and k is the number of roundings on the longest path from an operand to the result: 7 for x_mean without the mix
(s z, + mean, known m, + -> v, 1 - m, v (1 - m), +), 13 with it plus one for the fp32 rounding of inv M.  The test holds
k = 8 and k = 32, gamma_k = k 2^-24.

Worst measured error over the cases below, in units of 2^-24 B (MI355X): 2.70 without the mix, 2.21 with it.
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import _stream_util
from _stream_util import place
from _util import call

pytestmark = pytest.mark.gpu

K_PLAIN, K_MIX = 8, 32
SHAPES = [(2, 3, 8, 8), (3, 3, 5, 7), (2, 1, 6, 10), (1, 4, 4, 4)]     # 16-byte path, scalar tail, one channel, four channels
MASK_FORMS = ['NC', '11', 'N1', '1C']
within = functools.partial(_stream_util.within, show=True)      # every comparison prints its worst ratio


def matrices():
  """(M, inv M) in float64 -- the exact inverse of the fp32 matrix -- and the fp32 host arrays the entry takes."""
  import soft_truncation_amd as st
  cg = st.controllable_generation
  m64 = cg.M.double()
  u64 = torch.from_numpy(np.linalg.inv(m64.numpy()))
  host = lambda t: (ctypes.c_float * 9)(*t.reshape(-1).tolist())
  return m64, u64, host(cg.M), host(cg.INV_M)


def restate(x, data, z, mask, a, s, mix=None, unmix=None):
  """The header's formulas on float64 tensors; mask broadcasts.  -> (x_out, x_mean)."""
  times = lambda t, m: t if m is None else torch.einsum('bihw,ij->bjhw', t, m)
  wide = lambda v: v[:, None, None, None]
  u, d = times(x, mix), times(data, mix)
  mean = wide(a) * d
  known = mean if z is None else mean + wide(s) * z
  v = u * (1 - mask) + known * mask
  return times(v, unmix), times(v * (1 - mask) + mean * mask, unmix)


def magnitude(x, data, z, mask, a, s, mix=None, unmix=None):
  """B of the bound: restate() on absolute values."""
  ab = lambda t: None if t is None else t.abs()
  return restate(ab(x), ab(data), ab(z), mask, ab(a), ab(s), ab(mix), ab(unmix))


def _operands(shape, form, soft, seed):
  N, C, H, W = shape
  g = torch.Generator().manual_seed(seed)
  mshape = (N if form[0] == 'N' else 1, C if form[1] == 'C' else 1, H, W)
  mask = torch.rand(mshape, generator=g) if soft else (torch.rand(mshape, generator=g) < 0.5).float()
  return dict(x=torch.randn(shape, generator=g), x2=torch.randn(shape, generator=g), data=torch.randn(shape, generator=g),
              z=torch.randn(shape, generator=g), mask=mask, a=torch.rand(N, generator=g) + 0.25,
              s=torch.rand(N, generator=g) * 3 + 0.05)


def _run(lib, o, dev, use_z, use_mean, inplace, mix, shifted=False, x='x'):
  N, C, H, W = o['x'].shape
  d = {k: v.to(dev) for k, v in o.items()}
  xin = place(o[x], dev, shifted)
  out = xin if inplace else torch.full_like(d['x'], float('nan'))
  mean = torch.full_like(d['x'], float('nan')) if use_mean else None
  call(lib, 'impute_f32', xin, d['data'], d['z'] if use_z else None, d['mask'], d['a'], d['s'],
       ctypes.addressof(mix[0]) if mix else None, ctypes.addressof(mix[1]) if mix else None, out, mean, N, C, H * W,
       o['mask'].shape[0], o['mask'].shape[1])
  return out, mean


@pytest.mark.parametrize('soft', [False, True], ids=['binary', 'soft'])
@pytest.mark.parametrize('form', MASK_FORMS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_matches_float64(hip_lib, shape, form, soft):
  dev = torch.device('cuda:0')
  o = _operands(shape, form, soft, seed=sum(shape) * 7 + MASK_FORMS.index(form) * 2 + soft)
  m64, u64, c_m, c_u = matrices()
  f = {k: v.double() for k, v in o.items()}
  worst = 0.0
  for use_z, use_mean, inplace, mixed, shifted in itertools.product((True, False), (True, False), (False, True),
                                                                    (False, True) if shape[1] == 3 else (False,),
                                                                    (False, True)):
    mats = (m64, u64) if mixed else (None, None)
    want = restate(f['x'], f['data'], f['z'] if use_z else None, f['mask'], f['a'], f['s'], *mats)
    mag = magnitude(f['x'], f['data'], f['z'] if use_z else None, f['mask'], f['a'], f['s'], *mats)
    out, mean = _run(hip_lib, o, dev, use_z, use_mean, inplace, (c_m, c_u) if mixed else None, shifted)
    what = f'impute {shape} mask {form} {"soft" if soft else "binary"} z={use_z} inplace={inplace} mix={mixed} shifted={shifted}'
    k = K_MIX if mixed else K_PLAIN
    worst = max(worst, within(out, want[0], mag[0], k, what + ' x_out'))
    if use_mean:
      worst = max(worst, within(mean, want[1], mag[1], k, what + ' x_mean'))
  print(f'impute {shape} mask {form}: worst over the case {worst:.2f} x 2^-24 B')


@pytest.mark.parametrize('form', MASK_FORMS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_binary_mask_is_exact(hip_lib, shape, form):
  """No mix, mask of zeros and ones: the unknown part is x bit for bit, the known part does not depend on x."""
  dev = torch.device('cuda:0')
  o = _operands(shape, form, False, seed=sum(shape) + MASK_FORMS.index(form))
  m = o['mask'].expand(shape)
  assert 0 < int(m.sum()) < m.numel()
  for shifted, inplace in itertools.product((False, True), (False, True)):
    out1, _ = _run(hip_lib, o, dev, True, True, inplace, None, shifted, x='x')
    out2, _ = _run(hip_lib, o, dev, True, True, inplace, None, shifted, x='x2')
    out1, out2 = out1.cpu(), out2.cpu()
    assert torch.equal(out1[m == 0], o['x'][m == 0]) and torch.equal(out2[m == 0], o['x2'][m == 0])
    assert torch.equal(out1[m == 1], out2[m == 1])
    assert not torch.equal(out1[m == 0], out2[m == 0])


def test_unsupported_arguments_are_refused_and_write_nothing(hip_lib):
  dev = torch.device('cuda:0')
  _, _, c_m, c_u = matrices()
  raw = hip_lib.impute_f32.raw
  mix = (ctypes.addressof(c_m), ctypes.addressof(c_u))

  def refused(shape, mask_n, mask_c, mixed, dims=None):
    N, C, H, W = shape
    t = [torch.randn(shape, device=dev) for _ in range(3)]
    mask = torch.ones(shape, device=dev)
    ab = torch.ones(N, device=dev)
    out, mean = torch.full(shape, 7.0, device=dev), torch.full(shape, 7.0, device=dev)
    rc = raw(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), mask.data_ptr(), ab.data_ptr(), ab.data_ptr(),
             mix[0] if mixed else None, mix[1] if mixed else None, out.data_ptr(), mean.data_ptr(),
             *(dims or (N, C, H * W)), mask_n, mask_c, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((mean == 7.0).all())
    return rc

  assert refused((1, 4, 4, 4), 1, 4, True) == -3                        # the colour mix with C != 3
  assert refused((2, 1, 4, 4), 2, 1, True) == -3
  assert refused((3, 3, 4, 4), 2, 3, False) == -3                       # mask_n neither 1 nor N
  assert refused((3, 3, 4, 4), 3, 2, False) == -3                       # mask_c neither 1 nor C
  assert refused((3, 3, 4, 4), 0, 1, False) == -3
  assert refused((1, 3, 4, 4), 1, 1, False, dims=(2 ** 15, 2 ** 10, 2 ** 6)) == -3      # 2^31 elements
  assert refused((1, 3, 4, 4), 1, 1, True, dims=(2 ** 28, 3, 4)) == -3
  assert refused((1, 3, 4, 4), 1, 1, False, dims=(1, 1, 2 ** 31)) == -3
