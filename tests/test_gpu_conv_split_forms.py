"""The split convolutions (csrc/conv_x2.h, csrc/conv_x2d.h, csrc/conv_pl.h, the split path of csrc/conv.hip) on every launch
form, element by element: the case table of tests/_conv_split_cases.py through the product library.

Every case asserts the form it reaches through the library's own diagnostics, runs on guarded, NaN-prefilled buffers with
scratch of exactly the reported size, launches twice with wp = NULL and once on prepared weights (the f32-operand forward
once more through the record entry), and must repeat bit for bit.  The exact families must then EQUAL the float64
three-term model (instrument A of tests/_conv_split_ref.py); every other family must be within its derived bound element
by element (instrument B; no fitted factor).  tests/test_conv_split_cases_cpu.py holds the model to half of the same bounds
and shows that each way of breaking it is caught.

With the plain-C checker standing in (STK_SELFCHECK, no GPU) the exact families are held to the bound instead: the
checker multiplies the decoded planes in full, lo lo included, which the kernels leave out by design.

STK_CONV_SPLIT_PROFILE=<file>: the worst err / bound per form, direction, entry and family, and the count of bit-equal
exact cases, are written there when the module finishes (profiles/conv_split_accuracy.txt is such a run)."""
import os

import numpy as np
import pytest

import _conv_split_cases as cc
import _conv_split_ref as cr

pytestmark = pytest.mark.gpu

_worst, _exact = {}, {'run': 0, 'equal': 0}


@pytest.fixture(scope='module', autouse=True)
def _profile():
  yield
  path = os.environ.get('STK_CONV_SPLIT_PROFILE')
  if path and (_worst or _exact['run']):
    with open(path, 'w') as f:
      f.write('split convolutions: worst |got - ref| / bound per output element (tests/test_gpu_conv_split_forms.py)\n')
      f.write(f'exact cases bit-equal to the three-term model: {_exact["equal"]} of {_exact["run"]}\n')
      f.write(f'{"form":6s}{"dir":7s}{"entry":7s}{"family":10s}{"cases":>6s}  worst err / bound\n')
      for k in sorted(_worst):
        n, w = _worst[k]
        f.write(f'{k[0]:6s}{k[1]:7s}{k[2]:7s}{k[3]:10s}{n:6d}  {w:.4f}\n')


@pytest.mark.parametrize('name', cc.IDS)
def test_case(hip_lib, name):
  lib = hip_lib
  c = cc.BY_NAME[name]
  r = cc.BY_ROW[c.row]
  cc.assert_form(lib, c)
  got = cc.run(lib, name)
  assert np.isfinite(got).all(), f'{name}: non-finite result'
  if c.fam in cc.EXACT_FAMILIES and lib.is_device:
    want = cc.three_term_of(name)['out']
    _exact['run'] += 1
    off = got.astype(np.float64) != want
    if not off.any():
      _exact['equal'] += 1
    else:
      i = np.unravel_index(int(np.abs(got - want).argmax()), got.shape)
      raise AssertionError(f'{name}: {int(off.sum())} of {off.size} elements differ from the three-term model; the farthest at '
                           f'{tuple(int(j) for j in i)}: got {float(got[i])!r}, want {float(want[i])!r} '
                           f'({(float(got[i]) - float(want[i])) / cr.GRANULE:.3g} granules of 2^-12)')
    return
  ref, b = cc.reference_of(name)
  key = (cc.form_key(r), 'dgrad' if c.d == 'd' else 'fwd', c.entry, c.fam)
  w = float(cr.ratio(got, ref, b['bound']).max())
  n, old = _worst.get(key, (0, 0.0))
  _worst[key] = (n + 1, max(old, w))
  cr.within(got, ref, b['bound'], name)
